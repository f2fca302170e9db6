"""jtk_batch_chunk_prefer, jtk_batch_chunk_levels, jtk_batch_token_cut_levels / Batch.chunk_prefer, chunk_batch(prefer=...):
token-budget chunks that end at paragraph, line, sentence and word boundaries.  Every field is checked against the plain
restatement of the rule (tests/chunk_prefer_ref.py) applied to the byte strings of the oracle's tokens -- or, for the
byte-level custom encoding whose rank map is the 256 single bytes, to the bytes of the text: there every token is one byte, a
cut's lookback spans three tokens and a multi-byte character gives SPLIT cuts.  Every test here needs a real MI355X (`-m gpu`)."""
import ctypes as C
import random

import numpy as np
import pytest

import chunk_prefer_ref as ref
import chunk_ref
import oracle_lib
from test_chunks_gpu import _fuzz_docs, _pack

pytestmark = pytest.mark.gpu

PAD = -7
LONG = 8192            # JTK_CP_LONG_TOKENS of jtk_kernels.h: a document of more tokens (and more than one chunk) gets a workgroup
WALK_N = (1, 2, 3, 4, 7, 63, 64, 65, 255, 256, 257, 512, 2049)
PREFER = (0, 15, 2, 12)


@pytest.fixture(scope="module")
def jt():
    import jtokkit_amd
    return jtokkit_amd


@pytest.fixture(scope="module")
def byte_enc(jt):
    return jt.new_custom_encoding("bytes_only", jt._native.JTK_PATTERN_CL100K, {bytes([i]): i for i in range(256)}, {})


@pytest.fixture(scope="module")
def big(jt):
    """One document of about 40k cl100k tokens (the probe document repeated) and its oracle tokens' byte strings."""
    o = oracle_lib.get("cl100k_base")
    doc = (ref.PROBE * 40).encode("utf-8")
    toks = o.encode_batch(np.frombuffer(doc, dtype=np.uint8), np.array([0, len(doc)], dtype=np.int64), threads=8)[0].tolist()
    assert 40000 < len(toks) < 44000
    return doc, toks, ref.token_bytes(o, toks)


def _byte_tb(doc):
    return [bytes([x]) for x in doc]


def _sized(k, salt=0):
    """A well-formed document of exactly k bytes out of the probe text (rotated by salt characters), padded with 'x'."""
    if k == 0:
        return b""
    rot = salt % len(ref.PROBE)
    src = ((ref.PROBE[rot:] + ref.PROBE[:rot]) * (k // 1500 + 2)).encode("utf-8")
    src = src[:k].decode("utf-8", "ignore").encode("utf-8")            # (drop a character cut in half)
    return src + b"x" * (k - len(src))


def _plane(b, prefer, nt):
    import torch
    out = torch.full((nt + 1,), 99, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()                                          # (the fill runs on torch's stream, the pass on the batch's)
    b.token_cut_levels(prefer, out.data_ptr())
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    assert out[nt] == 99                                              # nothing past the plane
    return out[:nt]


def _expected(tbs, levels, N, ov, mt, doc_off, tok_off):
    """The arrays of chunk_fetch + level for documents with token byte strings tbs[d] (None: no chunks)."""
    f = dict(chunk_off=[0], doc=[], tok_begin=[], n_tok=[], split=[], byte_begin=[], byte_end=[], level=[])
    for d, tb in enumerate(tbs):
        if tb:
            cum = np.concatenate([[0], np.cumsum([len(x) for x in tb])])
            for (s, e, sp, el) in ref.chunks_fast(levels[d], N, ov, mt):
                f["doc"].append(d); f["tok_begin"].append(tok_off[d] + s); f["n_tok"].append(e - s); f["split"].append(sp)
                f["byte_begin"].append(doc_off[d] + cum[s]); f["byte_end"].append(doc_off[d] + cum[e]); f["level"].append(el)
        f["chunk_off"].append(len(f["doc"]))
    return f


def _check_call(b, tokens, tbs, levels, N, ov, mt, prefer, doc_off, tok_off, rows=True):
    """One jtk_batch_chunk_prefer through the Batch methods: count, every record field, the levels and the padded rows."""
    import torch
    nc = b.chunk_prefer(N, ov, mt, prefer)
    f = b.chunk_fetch()
    f["level"] = b.chunk_levels()[0]
    exp = _expected(tbs, levels, N, ov, mt, doc_off, tok_off)
    assert nc == len(exp["doc"]), (N, ov, mt, prefer)
    for k, v in exp.items():
        assert np.array_equal(np.asarray(f[k]).astype(np.int64), np.asarray(v, dtype=np.int64)), (k, N, ov, mt, prefer)
    if rows and nc * N <= 1 << 22:
        r = torch.full((nc * N + 1,), 12345, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()                                      # (as in _plane)
        b.chunk_rows(PAD, r.data_ptr())
        torch.cuda.synchronize()
        r = r.cpu().numpy()
        assert r[-1] == 12345
        r = r[:nc * N].reshape(nc, N)
        col = np.arange(N)[None, :]
        want = np.where(col < f["n_tok"][:, None], tokens[np.minimum(f["tok_begin"][:, None] + col, len(tokens) - 1)], PAD)
        bad = np.flatnonzero((r != want).any(axis=1))
        assert len(bad) == 0, (N, ov, mt, prefer, len(bad), bad[:8].tolist(), r[bad[0]].tolist(), want[bad[0]].tolist(),
                               int(f["tok_begin"][bad[0]]), int(f["n_tok"][bad[0]]))
    return f


# ---- level plane -------------------------------------------------------------------------------------------------------
EDGES = (64, 256, 2048)
PATTERNS = (b".\n\n", b"\r\n\r\n", "。".encode())


def _filler(k, salt):
    words = (b"alpha ", b"beta. ", b"gamma\n", "字".encode(), b"delta! ", b"e? ", b"\n\n", b"zeta\r\n")
    rng = random.Random(salt)
    out = b""
    while len(out) < k:
        out += rng.choice(words)
    out = out[:k].decode("utf-8", "ignore").encode("utf-8")            # (drop a character cut in half)
    return out + b"y" * (k - len(out))


def _edge_batch(pattern, shift):
    """One document whose bytes (= tokens) carry `pattern` from position E - shift on, for every E of EDGES."""
    out = b""
    for E in EDGES:
        at = E - shift
        out += _filler(at - len(out), at) + pattern
    return [out + _filler(40, 7)]


def _doc_edge_batch(shift):
    """Documents that start exactly at E + shift, for every E of EDGES, with "\\n" as the last byte of the one before and the
    first byte of the one after, empty documents in between, and a malformed document (negative status) at the end."""
    docs, total = [], 0
    lead = b""
    for E in EDGES:
        body = lead + _filler(E + shift - total - len(lead) - 1, E) + b"\n"
        docs += [body, b"", b""]
        total += len(body)
        lead = b"\nq"
    docs += [b"\nabc def.\n\nghi", b"", b"ok \xff\xfe bad", b"\n\ntail"]
    return docs


def _check_plane(b, docs, validate=False):
    bs, text, doc_off = _pack(docs)
    b.encode_host(text, doc_off, ordinary=True, validate=validate)
    res = b.fetch()
    ok = [d for d in range(len(bs)) if res.status[d] >= 0]
    for d in ok:
        assert res.doc(d).tolist() == list(bs[d])                     # one token per byte, its id the byte
    for prefer in (15, 0, 8, 5):
        got = _plane(b, prefer, len(res.tokens))
        for d in ok:
            exp = ref.levels(_byte_tb(bs[d]), prefer)
            assert got[res.tok_off[d]:res.tok_off[d + 1]].tolist() == exp, (d, prefer)
    return bs, doc_off, res, ok


def test_level_plane_at_wave_workgroup_and_tile_edges(byte_enc):
    """Byte-level tokens: ".\\n\\n", "\\r\\n\\r\\n" and the three bytes of U+3002 laid across token positions 63/64/65, 255/256/257
    and 2047/2048/2049 of the batch, one shift at a time."""
    b = byte_enc.new_batch()
    for pattern in PATTERNS:
        for shift in range(len(pattern) + 1):
            bs, doc_off, res, _ = _check_plane(b, _edge_batch(pattern, shift))
            for E in EDGES:
                assert bs[0][E - shift:E - shift + len(pattern)] == pattern
    b.close()


def test_level_plane_stops_at_document_starts(byte_enc):
    """Documents that start on (and one token either side of) those edges, "\\n" before and after the boundary, empty documents
    in between: the second document's first cut is LINE, not PARAGRAPH.  A malformed document (JTK_ENCODE_VALIDATE_UTF8) has
    a negative status and gets no chunks."""
    b = byte_enc.new_batch()
    for shift in (-1, 0, 1):
        docs = _doc_edge_batch(shift)
        bs, doc_off, res, ok = _check_plane(b, docs, validate=True)
        assert res.status[len(docs) - 2] < 0 and len(ok) == len(docs) - 1
        for k, E in enumerate(EDGES):
            assert res.tok_off[3 * k + 3] == E + shift
        got = _plane(b, 15, len(res.tokens))
        for d in (3, 6, 9):
            t0 = res.tok_off[d]
            assert bs[d][:1] == b"\n" and bs[d - 3][-1:] == b"\n"
            assert got[t0] == ref.DOC_END_ and got[t0 + 1] == ref.LINE_
        tbs = [_byte_tb(x) if d in ok else None for d, x in enumerate(bs)]
        for prefer, (N, ov, mt) in ((15, (7, 2, 4)), (12, (64, 63, 1))):
            levels = [ref.levels(tb, prefer) if tb else None for tb in tbs]
            f = _check_call(b, res.tokens, tbs, levels, N, ov, mt, prefer, doc_off, res.tok_off)
            d = len(docs) - 2
            assert f["chunk_off"][d] == f["chunk_off"][d + 1]
    b.close()


def test_level_plane_cl100k_fuzz_and_probe(jt):
    enc = jt.get_encoding("cl100k_base")
    o = oracle_lib.get("cl100k_base")
    texts = [t for t in _fuzz_docs(random.Random(5))] + [ref.PROBE]
    bs, text, doc_off = _pack(texts)
    b = enc.new_batch()
    b.encode_host(text, doc_off, ordinary=True)
    res = b.fetch()
    tbs = [ref.token_bytes(o, o.encode_ordinary(x)) for x in bs]
    assert len(tbs[-1]) == 1046
    seen = set()
    for prefer in (15, 0, 2, 12, 9):
        got = _plane(b, prefer, len(res.tokens))
        for d, tb in enumerate(tbs):
            exp = ref.levels(tb, prefer)
            assert got[res.tok_off[d]:res.tok_off[d + 1]].tolist() == exp, (d, prefer)
            seen.update(exp)
    assert seen == set(range(7))
    b.close()


# ---- walk --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", WALK_N)
def test_walk_grid(byte_enc, N):
    """N x overlap {0, 1, N - 1} x min_tokens {1, (N + 1) // 2, N} x prefer {0, 15, 2, 12} on byte-level documents of 0, 1, N and
    N + 1 tokens and on both sides of the long-document threshold (JTK_CP_LONG_TOKENS = 8192 tokens: 8192 is walked by one
    lane, 8193 by a workgroup) and at 3 x it."""
    sizes = [0, 1, N, N + 1, 0, LONG - 1, LONG, LONG + 1, 3 * LONG, 5]
    bs, text, doc_off = _pack([_sized(k, 31 * i) for i, k in enumerate(sizes)])
    b = byte_enc.new_batch()
    b.encode_host(text, doc_off, ordinary=True)
    res = b.fetch()
    assert np.array_equal(res.tok_off, doc_off) and np.array_equal(res.tokens, text)
    tbs = [_byte_tb(x) for x in bs]
    for prefer in PREFER:
        levels = [np.array(ref.levels(tb, prefer), dtype=np.uint8) for tb in tbs]
        for ov in sorted({0, 1, N - 1}):
            if ov >= N:
                continue
            for mt in sorted({1, (N + 1) // 2, N}):
                _check_call(b, res.tokens, tbs, levels, N, ov, mt, prefer, doc_off, res.tok_off)
    b.close()


@pytest.mark.parametrize("N", (7, 64))
def test_walk_40k_token_document(jt, big, N):
    """One cl100k document of about 40k tokens: a workgroup walks a chain of far more than 256 chunks."""
    doc, toks, tb = big
    enc = jt.get_encoding("cl100k_base")
    bs, text, doc_off = _pack([b"short one.\n\nTwo.", doc, b""])
    o = oracle_lib.get("cl100k_base")
    tbs = [ref.token_bytes(o, o.encode_ordinary(bs[0])), tb, []]
    b = enc.new_batch()
    b.encode_host(text, doc_off, ordinary=True)
    res = b.fetch()
    assert res.doc(1).tolist() == toks
    for prefer in (15, 2):
        levels = [np.array(ref.levels(t, prefer), dtype=np.uint8) for t in tbs]
        for ov, mt in ((0, (N + 1) // 2), (1, 1), (N - 1, N)):
            f = _check_call(b, res.tokens, tbs, levels, N, ov, mt, prefer, doc_off, res.tok_off)
            assert f["chunk_off"][2] - f["chunk_off"][1] > 256
    b.close()


# ---- equivalence with jtk_batch_chunk on the device -------------------------------------------------------------------------
def test_prefer_0_min_1_equals_plain_chunk(jt, big):
    enc = jt.get_encoding("cl100k_base")
    texts = [t.encode("utf-8") for t in _fuzz_docs(random.Random(6), 150)] + [big[0]]
    bs, text, doc_off = _pack(texts)
    b = enc.new_batch()
    b.encode_host(text, doc_off, ordinary=False)
    for N, ov in ((1, 0), (2, 1), (3, 0), (7, 2), (64, 0), (64, 63), (512, 64)):
        n0 = b.chunk(N, ov)
        plain = b.chunk_fetch()
        with pytest.raises(jt.EncodingError):
            b.chunk_levels()                                          # a plain chunk call has no levels
        assert b.chunk_prefer(N, ov, 1, 0) == n0
        got = b.chunk_fetch()
        for k in plain:
            assert np.array_equal(plain[k], got[k]), (k, N, ov)
        lv = b.chunk_levels()[0]
        assert ((lv == 6) | (lv == 1) | (lv == 0)).all() and (got["split"][lv == 0] != 0).all()
    b.close()


# ---- surface ---------------------------------------------------------------------------------------------------------------
def test_chunk_batch_prefer_char_unit_and_default_call(jt):
    enc = jt.get_encoding("cl100k_base")
    o = oracle_lib.get("cl100k_base")
    texts = [ref.PARA * 2 + ref.CJK, "été. Ça va?\n\nOui! 🍕🚀 ok", "", "one"]
    for N, ov in ((16, 0), (5, 2)):
        out = enc.chunk_batch(texts, N, ov, prefer="all", unit="char")
        plain = enc.chunk_batch(texts, N, ov)
        for t, chunks, pchunks in zip(texts, out, plain):
            toks = o.encode(t)
            tb = ref.token_bytes(o, toks)
            exp = ref.chunks(ref.levels(tb, 15), N, ov, (N + 1) // 2)
            assert [(c[0], c[3], c[4]) for c in chunks] == [(toks[s:e], sp, el) for (s, e, sp, el) in exp]
            for ctoks, start, end, sp, el in chunks:
                if not sp:
                    assert t[start:end] == o.decode_bytes(ctoks).decode("utf-8")
            # without the new keywords: four fields, the plain rule
            fb = chunk_ref.first_bytes(o, toks)
            assert [(c[0], c[3]) for c in pchunks] == [(toks[s:e], sp) for (s, e, sp) in chunk_ref.chunks(fb, N, ov)]
            assert all(len(c) == 4 for c in pchunks)
    # the forms of `prefer`
    a = enc.chunk_batch(texts, 16, 0, prefer=("line", "paragraph"))
    assert a == enc.chunk_batch(texts, 16, 0, prefer=12) == enc.chunk_batch(texts, 16, 0, prefer=["paragraph", "line"], min_tokens=8)
    assert enc.chunk_batch(texts, 16, 0, prefer="word") == enc.chunk_batch(texts, 16, 0, prefer=1)
    with pytest.raises(ValueError):
        enc.chunk_batch(texts, 16, 0, prefer=("words",))


def test_chunk_batch_device_prefer_equals_host_route(jt):
    import torch
    enc = jt.get_encoding("cl100k_base")
    texts = [t for t in _fuzz_docs(random.Random(7), 80) if "<|" not in t] + [ref.PROBE]
    bs, text, doc_off = _pack(texts)
    d_text = torch.from_numpy(np.ascontiguousarray(text)).cuda()
    d_off = torch.from_numpy(doc_off).cuda()
    for N, ov, mt, prefer in ((32, 4, None, "all"), (7, 0, 2, ("sentence",)), (64, 63, 64, 12)):
        host = enc.chunk_batch([bytes(x) for x in bs], N, ov, prefer=prefer, min_tokens=mt)
        out = enc.chunk_batch_device(d_text, d_off, N, ov, pad_id=PAD, prefer=prefer, min_tokens=mt, unit="char")
        torch.cuda.synchronize()
        assert out["level"].dtype == torch.uint8
        o = {k: v.cpu().numpy() for k, v in out.items()}
        flat = [(d, c) for d, cs in enumerate(host) for c in cs]
        assert len(flat) == len(o["n_tok"]) == o["chunk_off"][-1]
        for i, (d, (toks, s, e, sp, el)) in enumerate(flat):
            assert o["doc"][i] == d and o["rows"][i, :len(toks)].tolist() == toks and (o["rows"][i, len(toks):] == PAD).all()
            assert (o["byte_begin"][i] - doc_off[d], o["byte_end"][i] - doc_off[d], bool(o["split"][i]), o["level"][i]) == (s, e, sp, el)
        plain = enc.chunk_batch_device(d_text, d_off, N, ov, pad_id=PAD)
        assert "level" not in plain


def test_special_literal_before_a_paragraph_break(jt):
    """allowed_special: the literal is one token whose bytes are its text; the cut after "<|endoftext|>\\n\\n" is a PARAGRAPH."""
    enc = jt.get_encoding("cl100k_base")
    o = oracle_lib.get("cl100k_base")
    t = "First part ends here<|endoftext|>\n\nSecond part. It goes on and on for a while longer.\n"
    out = enc.chunk_batch([t], 12, 0, allowed_special="all", prefer="all", min_tokens=2)[0]
    ids = [x for c in out for x in c[0]]
    assert 100257 in ids
    tb = ref.token_bytes(o, ids)
    assert b"".join(tb) == t.encode()
    exp = ref.chunks(ref.levels(tb, 15), 12, 0, 2)
    assert [(c[0], c[3], c[4]) for c in out] == [(ids[s:e], sp, el) for (s, e, sp, el) in exp]
    k = ids.index(100257)
    assert tb[k + 1] == b"\n\n" and out[0][4] == ref.PARAGRAPH_ and out[0][0][-2:] == ids[k:k + 2]


def test_levels_follow_the_decoded_stream_after_encode_pieces(jt):
    """encode_pieces leaves out the bytes no piece covers: the levels are those of the decoded stream, not of the text."""
    enc = jt.get_encoding("cl100k_base")
    o = oracle_lib.get("cl100k_base")
    doc = b"alpha.\n\nbeta gamma"                                      # pieces: "alpha." | "beta" | " gamma": the \n\n is left out
    begins, ends = [0, 8, 12], [6, 12, 18]
    toks = o.encode_pieces(doc, begins, ends)
    tb = ref.token_bytes(o, toks)
    assert b"".join(tb) == b"alpha.beta gamma"
    b = enc.new_batch()
    b.encode_pieces(np.frombuffer(doc, dtype=np.uint8), np.array([0, len(doc)], dtype=np.int64), begins, ends)
    res = b.fetch()
    assert res.tokens.tolist() == toks
    got = _plane(b, 15, len(toks)).tolist()
    assert got == ref.levels(tb, 15) and ref.PARAGRAPH_ not in got and ref.LINE_ not in got
    b.close()


def test_bad_arguments(jt):
    import torch
    N = jt._native
    L = N.lib()
    enc = jt.get_encoding("cl100k_base")
    b = enc.new_batch()
    nc = C.c_int64(0)
    p = C.c_void_p()
    BAD = N.JTK_ERR_INVALID_ARGUMENT
    assert L.jtk_batch_chunk_prefer(b._h, 4, 0, 2, 15, None, C.byref(nc)) == BAD                 # no encode yet
    assert L.jtk_batch_token_cut_levels(b._h, 15, None, None) == BAD
    assert L.jtk_batch_chunk_levels(b._h, None, C.byref(p)) == BAD
    _, text, doc_off = _pack(["some text here.\n\nMore of it", "more"])
    b.encode_host(text, doc_off)
    for n_, ov, mt, pf in ((0, 0, 1, 0), (4, 4, 1, 0), (4, -1, 1, 0), (1 << 31, 0, 1, 0), (4, 0, 0, 15), (4, 0, 5, 15), (4, 0, -1, 15),
                           (4, 0, 2, 16), (4, 0, 2, 31), (4, 0, 2, 1 << 31)):
        assert L.jtk_batch_chunk_prefer(b._h, n_, ov, mt, pf, None, C.byref(nc)) == BAD, (n_, ov, mt, pf)
    lv = torch.zeros(64, dtype=torch.uint8, device="cuda")
    assert L.jtk_batch_token_cut_levels(b._h, 16, lv.data_ptr(), None) == BAD
    assert L.jtk_batch_token_cut_levels(b._h, 15, None, None) == BAD                              # d_level is NULL
    assert L.jtk_batch_chunk_prefer(b._h, 4, 3, 4, 15, None, C.byref(nc)) == N.JTK_OK and nc.value > 0
    assert L.jtk_batch_chunk_levels(b._h, None, C.byref(p)) == N.JTK_OK and p.value
    assert L.jtk_batch_chunk(b._h, 4, 0, None, C.byref(nc)) == N.JTK_OK
    assert L.jtk_batch_chunk_levels(b._h, None, C.byref(p)) == BAD                                # a plain chunk call
    b.encode_host(text, doc_off, count_only=True)
    assert L.jtk_batch_chunk_prefer(b._h, 4, 0, 2, 15, None, C.byref(nc)) == BAD
    assert L.jtk_batch_token_cut_levels(b._h, 15, lv.data_ptr(), None) == BAD
    d_text = torch.from_numpy(np.ascontiguousarray(text)).cuda()
    d_off = torch.from_numpy(doc_off).cuda()
    rows = torch.empty((2, 4), dtype=torch.int32, device="cuda")
    aux = [torch.empty(2, dtype=dt, device="cuda") for dt in (torch.int64, torch.bool, torch.int32)]
    b.encode_device_max_tokens(d_text.data_ptr(), d_off.data_ptr(), 2, len(text), 4, rows.data_ptr(), aux[0].data_ptr(),
                               aux[1].data_ptr(), aux[2].data_ptr())
    assert L.jtk_batch_chunk_prefer(b._h, 4, 0, 2, 15, None, C.byref(nc)) == BAD
    assert L.jtk_batch_token_cut_levels(b._h, 15, lv.data_ptr(), None) == BAD
    with pytest.raises(ValueError):
        enc.chunk_batch_device(d_text, d_off, 4, 4, prefer="all")
    b.close()
