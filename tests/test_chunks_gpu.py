"""jtk_batch_chunk and friends / HipEncoding.chunk_batch, chunk_batch_device: token-budget chunks of the last batch encode,
their byte spans, padded rows and the per-token byte offsets.  Every field is checked against the plain restatement of the
rule (tests/chunk_ref.py) applied to the CPU oracle's tokens.  Every test here needs a real MI355X (`-m gpu`)."""
import ctypes as C
import random
import re

import numpy as np
import pytest

import chunk_ref
import oracle_lib
import regex_crosscheck as rc

pytestmark = pytest.mark.gpu

PAD = -5
GRID = [(1, 0), (2, 1), (3, 0), (4, 3), (7, 2), (64, 0), (64, 63), (512, 64)]


@pytest.fixture(scope="module")
def jt():
    import jtokkit_amd
    return jtokkit_amd


@pytest.fixture(scope="module")
def tabs():
    return chunk_ref.IdTables(oracle_lib.get("cl100k_base"))


def _pack(texts):
    bs = [t if isinstance(t, (bytes, bytearray)) else t.encode("utf-8") for t in texts]
    doc_off = np.zeros(len(bs) + 1, dtype=np.int64)
    np.cumsum([len(x) for x in bs], out=doc_off[1:])
    text = np.frombuffer(b"".join(bs), dtype=np.uint8) if doc_off[-1] else np.zeros(0, dtype=np.uint8)
    return bs, text, doc_off


def _oracle_tokens(o, doc, ordinary, validate=False):
    """The oracle's tokens of one document, or None where the device gives a negative status."""
    if validate:
        try:
            doc.decode("utf-8")
        except UnicodeDecodeError:
            return None
    try:
        return o.encode_ordinary(doc) if ordinary else o.encode(doc)
    except oracle_lib.OracleError:
        return None


def _expected(tabs, toks, N, ov):
    """[(s, e, split, byte_s, byte_e)] of one document by the restatement, byte positions relative to the document."""
    toks = np.asarray(toks, dtype=np.int64)
    cum = np.zeros(len(toks) + 1, dtype=np.int64)
    np.cumsum(tabs.length[toks], out=cum[1:])
    return [(s, e, sp, int(cum[s]), int(cum[e])) for (s, e, sp) in chunk_ref.chunks(tabs.first[toks], N, ov)], cum


def _check_fields(tabs, f, tok_off, doc_off, docs, exp_tokens, N, ov):
    """f: the chunk arrays (host); exp_tokens[d]: the oracle's tokens of document d (None: negative status, no chunks)."""
    co = f["chunk_off"]
    assert co[0] == 0
    for d in docs:
        got = range(co[d], co[d + 1])
        toks = exp_tokens[d]
        if toks is None:
            assert len(got) == 0, d
            continue
        exp, _ = _expected(tabs, toks, N, ov)
        assert len(got) == len(exp), (d, N, ov)
        for c, (s, e, sp, bs, be) in zip(got, exp):
            assert f["doc"][c] == d
            assert (f["tok_begin"][c] - tok_off[d], f["n_tok"][c], bool(f["split"][c])) == (s, e - s, sp), (d, c, N, ov)
            assert (f["byte_begin"][c], f["byte_end"][c]) == (doc_off[d] + bs, doc_off[d] + be), (d, c)


def _fuzz_docs(rng, n=250):
    texts = [rc.random_text(rng, rng.randint(0, 80)) for _ in range(n)]
    texts += ["", "\U0001F355" * 9, "I love \U0001F355\U0001F680 ok", "日本語のテキストを分割する" * 5, "漢字龘靐齉" * 6,
              "हिन्दी भाषा में पाठ " * 4, "a��b", "", "한국어 " * 9, "x <|endoftext|> y", "they'll 1234567 " * 30]
    return texts


def _torch_rows_check(rows, f, tokens, n_chunks, pad):
    rows = rows.reshape(n_chunks, -1)
    for c in range(n_chunks):
        tb, n = int(f["tok_begin"][c]), int(f["n_tok"][c])
        assert rows[c, :n].tolist() == tokens[tb:tb + n].tolist(), c
        assert (rows[c, n:] == pad).all(), c


def test_host_input_fuzz_all_fields(jt, tabs):
    """Host-input encodes, encode() and encodeOrdinary(), the whole (N, overlap) grid: records, rows, token offsets."""
    import torch
    enc = jt.get_encoding("cl100k_base")
    o = oracle_lib.get("cl100k_base")
    bs, text, doc_off = _pack(_fuzz_docs(random.Random(5)))
    b = enc.new_batch()
    for ordinary in (True, False):
        exp_tokens = [_oracle_tokens(o, x, ordinary) for x in bs]
        b.encode_host(text, doc_off, ordinary)
        res = b.fetch()
        for d, t in enumerate(exp_tokens):
            if t is not None:
                assert res.doc(d).tolist() == t
            else:
                assert res.status[d] < 0
        # token offsets (no chunk call yet on this encode: the byte scan runs on its own)
        pos = torch.empty(max(len(res.tokens), 1), dtype=torch.int64, device="cuda")
        b.token_offsets(pos.data_ptr())
        torch.cuda.synchronize()
        pos = pos.cpu().numpy()[:len(res.tokens)]
        for d in range(len(bs)):
            t0, t1 = res.tok_off[d], res.tok_off[d + 1]
            if t1 > t0:
                cum = np.concatenate([[0], np.cumsum(tabs.length[res.tokens[t0:t1]])])[:-1]
                assert (pos[t0:t1] == doc_off[d] + cum).all(), d
        for N, ov in GRID:
            nc = b.chunk(N, ov)
            f = b.chunk_fetch()
            assert nc == len(f["doc"]) == f["chunk_off"][-1]
            _check_fields(tabs, f, res.tok_off, doc_off, range(len(bs)), exp_tokens, N, ov)
            rows = torch.full((nc * N + 1,), 12345, dtype=torch.int32, device="cuda")
            b.chunk_rows(PAD, rows.data_ptr())
            torch.cuda.synchronize()
            r = rows.cpu().numpy()
            assert r[-1] == 12345                                     # nothing past the rows
            _torch_rows_check(r[:nc * N], f, res.tokens, nc, PAD)
            # unflagged chunks decode to their byte span
            for c in range(nc):
                if not f["split"][c]:
                    tb, n = int(f["tok_begin"][c]), int(f["n_tok"][c])
                    piece = o.decode_bytes(res.tokens[tb:tb + n].tolist())
                    assert piece == text[f["byte_begin"][c]:f["byte_end"][c]].tobytes()
                    piece.decode("utf-8")
            # chunk 0 against jtk_batch_truncate(N) on the same batch, where that cut is a byte boundary
            kept, _ = b.truncate(N)
            for d in range(len(bs)):
                if exp_tokens[d] and kept[d] > 0:
                    cut = doc_off[d] + int(tabs.length[res.doc(d)[:kept[d]]].sum())
                    if cut == doc_off[d + 1] or (text[cut] & 0xC0) != 0x80:
                        assert f["n_tok"][f["chunk_off"][d]] == kept[d], (d, N)
        # token offsets again, now from the chunk call's byte scan
        pos2 = torch.empty(max(len(res.tokens), 1), dtype=torch.int64, device="cuda")
        b.token_offsets(pos2.data_ptr())
        torch.cuda.synchronize()
        assert (pos2.cpu().numpy()[:len(res.tokens)] == pos).all()
    b.close()


def test_split_chunks_occur(jt, tabs):
    """Emoji split into byte-level tokens: with N <= 3 some chunks start or end inside a character (split = 1)."""
    enc = jt.get_encoding("cl100k_base")
    out = enc.chunk_batch(["\U0001F355\U0001F9E0\U0001F680" * 5], 2)
    assert any(sp for (_, _, _, sp) in out[0])
    assert [t for (toks, _, _, _) in out[0] for t in toks] == oracle_lib.get("cl100k_base").encode("\U0001F355\U0001F9E0\U0001F680" * 5)


def test_chunk_batch_host_api(jt, tabs):
    enc = jt.get_encoding("cl100k_base")
    o = oracle_lib.get("cl100k_base")
    texts = [t for t in _fuzz_docs(random.Random(9), 60) if "<|" not in t]
    for N, ov in ((3, 1), (16, 0), (64, 8)):
        out = enc.chunk_batch(texts, N, ov)
        for t, chunks in zip(texts, out):
            b = t.encode("utf-8")
            toks = o.encode(t)
            exp, cum = _expected(tabs, toks, N, ov)
            assert [(c[1], c[2], c[3]) for c in chunks] == [(bs_, be_, sp) for (_, _, sp, bs_, be_) in exp]
            assert [c[0] for c in chunks] == [toks[s:e] for (s, e, _, _, _) in exp]
            for toks_c, s, e, sp in chunks:
                if not sp:
                    assert o.decode_bytes(toks_c) == b[s:e]
    with pytest.raises(jt.UnsupportedOperationError):
        enc.chunk_batch(["a <|endoftext|> b"], 8)


def test_custom_pattern_through_host_matcher(jt, tabs):
    enc = jt.get_encoding("cl100k_base")
    o = oracle_lib.get("cl100k_base")
    pat = re.compile(r"\S+|\s+")
    texts = ["hello world, chunks of text", "日本語 テキスト \U0001F355\U0001F355"]
    enc._host_pattern, saved = pat, enc._host_pattern
    try:
        out = enc.chunk_batch(texts, 3, 1)
        with pytest.raises(ValueError):
            import torch
            enc.chunk_batch_device(torch.zeros(16, dtype=torch.uint8, device="cuda"), torch.zeros(2, dtype=torch.int64, device="cuda"), 4)
    finally:
        enc._host_pattern = saved
    for t, chunks in zip(texts, out):
        b = t.encode("utf-8")
        ends = [m.end() for m in pat.finditer(t)]
        begins = [m.start() for m in pat.finditer(t)]
        bb = [len(t[:i].encode()) for i in begins]
        be = [len(t[:i].encode()) for i in ends]
        toks = o.encode_pieces(b, bb, be)
        exp, _ = _expected(tabs, toks, 3, 1)
        assert [c[0] for c in chunks] == [toks[s:e] for (s, e, _, _, _) in exp]


def _device_call(enc, text, doc_off, N, ov, ordinary, pad=PAD):
    import torch
    d_text = torch.from_numpy(np.ascontiguousarray(text)).cuda()
    d_off = torch.from_numpy(np.ascontiguousarray(doc_off)).cuda()
    out = enc.chunk_batch_device(d_text, d_off, N, ov, ordinary=ordinary, pad_id=pad)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _check_device_out(tabs, o, out, bs, text, doc_off, exp_tokens, N, ov, docs=None):
    docs = range(len(bs)) if docs is None else docs
    nc = len(out["n_tok"])
    f = dict(chunk_off=out["chunk_off"], doc=out["doc"], n_tok=out["n_tok"], byte_begin=out["byte_begin"],
             byte_end=out["byte_end"], split=out["split"])
    # tok_begin is not returned by the device call: rebuild it from the document's first token (oracle counts)
    counts = np.array([len(t) if t is not None else 0 for t in exp_tokens], dtype=np.int64)
    tok_off = np.concatenate([[0], np.cumsum(counts)])
    tb = np.zeros(nc, dtype=np.int64)
    for d in docs:
        toks = exp_tokens[d]
        if toks is None:
            assert out["status"][d] < 0 and out["chunk_off"][d + 1] == out["chunk_off"][d]
            continue
        assert out["status"][d] == 0
        exp, _ = _expected(tabs, toks, N, ov)
        for k, c in enumerate(range(out["chunk_off"][d], out["chunk_off"][d + 1])):
            tb[c] = tok_off[d] + exp[k][0] if k < len(exp) else -1
            row = out["rows"][c]
            s, e = exp[k][0], exp[k][1]
            assert row[:e - s].tolist() == toks[s:e] and (row[e - s:] == PAD).all(), (d, c)
            if not out["split"][c]:
                piece = o.decode_bytes(row[:e - s].tolist())
                assert piece == text[out["byte_begin"][c]:out["byte_end"][c]].tobytes()
    f["tok_begin"] = tb
    _check_fields(tabs, f, tok_off, doc_off, docs, exp_tokens, N, ov)


def test_device_input_fuzz(jt, tabs):
    enc = jt.get_encoding("cl100k_base")
    o = oracle_lib.get("cl100k_base")
    bs, text, doc_off = _pack(_fuzz_docs(random.Random(6), 150))
    for ordinary in (True, False):
        exp_tokens = [_oracle_tokens(o, x, ordinary) for x in bs]
        for N, ov in GRID:
            out = _device_call(enc, text, doc_off, N, ov, ordinary)
            _check_device_out(tabs, o, out, bs, text, doc_off, exp_tokens, N, ov)


def test_status_documents_and_validation(jt, tabs):
    """Empty documents, a special literal under encode(), malformed UTF-8 with validation: no chunks."""
    enc = jt.get_encoding("cl100k_base")
    o = oracle_lib.get("cl100k_base")
    bs, text, doc_off = _pack(["", "abc def", "x<|endoftext|>", b"ok \xff\xfe bad", "", "été " * 20, ""])
    b = enc.new_batch()
    b.encode_host(text, doc_off, ordinary=False, validate=True)
    res = b.fetch()
    assert res.status[2] < 0 and res.status[3] < 0
    nc = b.chunk(4, 1)
    f = b.chunk_fetch()
    exp_tokens = [None if res.status[d] < 0 else o.encode(bs[d]) for d in range(len(bs))]
    assert nc == sum(len(_expected(tabs, t, 4, 1)[0]) for t in exp_tokens if t is not None)
    _check_fields(tabs, f, res.tok_off, doc_off, range(len(bs)), exp_tokens, 4, 1)
    b.close()


def test_zero_documents(jt):
    import torch
    enc = jt.get_encoding("cl100k_base")
    b = enc.new_batch()
    b.encode_host(np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.int64))
    assert b.chunk(8) == 0
    f = b.chunk_fetch()
    assert f["chunk_off"].tolist() == [0] and len(f["doc"]) == 0
    b.chunk_rows(PAD, None)
    b.close()
    out = enc.chunk_batch_device(torch.zeros(0, dtype=torch.uint8, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda"), 8)
    torch.cuda.synchronize()
    assert out["rows"].shape == (0, 8) and out["chunk_off"].tolist() == [0]


def test_pipeline_chunks(jt, tabs):
    """A host batch cut into several pipeline chunks (JTK_OPT_HOST_CHUNK_BYTES = 64 KiB)."""
    from jtokkit_amd import corpus
    enc = jt.get_encoding("cl100k_base")
    o = oracle_lib.get("cl100k_base")
    text, doc_off = corpus.mixed(300, mean_bytes=2048, lo=16, hi=8192, seed=12)
    text = np.asarray(text, dtype=np.uint8)
    b = enc.new_batch()
    b.set_option(jt._native.JTK_OPT_HOST_CHUNK_BYTES, 1 << 16)
    b.set_option(jt._native.JTK_OPT_CHUNK_BYTES, 1 << 16)
    b.encode_host(text, doc_off, ordinary=True)
    res = b.fetch()
    exp_tokens = [o.encode_ordinary(text[doc_off[d]:doc_off[d + 1]].tobytes()) for d in range(len(doc_off) - 1)]
    for N, ov in ((5, 2), (256, 0)):
        b.chunk(N, ov)
        _check_fields(tabs, b.chunk_fetch(), res.tok_off, doc_off, range(len(doc_off) - 1), exp_tokens, N, ov)
    b.close()


def test_long_documents_take_the_workgroup_path(jt, tabs):
    """One document of ~3 M tokens (N = 512 and 8192, with and without overlap) and a CJK / emoji document cut at N = 3:
    many chunks per document, on the workgroup path, with misses on the grid."""
    import torch
    from jtokkit_amd import corpus
    enc = jt.get_encoding("cl100k_base")
    o = oracle_lib.get("cl100k_base")
    t1, off1 = corpus.english(3000, mean_bytes=4096, lo=2048, hi=8192, seed=21)
    t2, off2 = corpus.mixed(200, mean_bytes=4096, lo=1024, hi=8192, seed=22)
    big = bytes(np.asarray(t1, dtype=np.uint8)) + bytes(np.asarray(t2, dtype=np.uint8))
    rng = random.Random(3)
    cjk = "".join(rng.choice(["漢字", "龘靐", "\U0001F355", "\U0001F9E0", "日本語", "한국", " "]) for _ in range(40000))
    bs, text, doc_off = _pack([big, "short one", cjk.encode()])
    toks_big = o.encode_batch(np.frombuffer(big, dtype=np.uint8), np.array([0, len(big)], dtype=np.int64), threads=16)[0].tolist()
    assert len(toks_big) > 2_000_000
    exp_tokens = [toks_big, o.encode_ordinary(bs[1]), o.encode_ordinary(bs[2])]
    b = enc.new_batch()
    d_text = torch.from_numpy(np.ascontiguousarray(text)).cuda()
    d_off = torch.from_numpy(doc_off).cuda()
    b.encode_device(d_text.data_ptr(), d_off.data_ptr(), len(bs), len(text), ordinary=True)
    res = b.fetch()
    assert res.doc(0).tolist() == toks_big
    for N, ov in ((512, 0), (512, 64), (8192, 100), (3, 1), (3, 0)):
        b.chunk(N, ov)
        _check_fields(tabs, b.chunk_fetch(), res.tok_off, doc_off, range(3), exp_tokens, N, ov)
    b.close()


def test_200k_documents_sampled(jt, tabs):
    """200,000 corpus.mixed documents through chunk_batch_device; a seeded 1 % sample checked field by field."""
    from jtokkit_amd import corpus
    enc = jt.get_encoding("cl100k_base")
    o = oracle_lib.get("cl100k_base")
    text, doc_off = corpus.mixed(200000, mean_bytes=256, lo=16, hi=4096, seed=31)
    text = np.asarray(text, dtype=np.uint8)
    rng = random.Random(17)
    sample = sorted(rng.sample(range(200000), 2000))
    exp_tokens = [None] * 200000
    for d in sample:
        exp_tokens[d] = o.encode_ordinary(text[doc_off[d]:doc_off[d + 1]].tobytes())
    for N, ov in ((64, 0), (128, 16)):
        out = _device_call(enc, text, doc_off, N, ov, True)
        assert (out["status"] == 0).all()
        _check_device_out(tabs, o, out, [None] * 200000, text, doc_off, exp_tokens, N, ov, docs=sample)


def test_non_default_stream_ordering(jt, tabs):
    """The text is written on a non-default torch stream right before the call on that stream: the chunks see it."""
    import torch
    enc = jt.get_encoding("cl100k_base")
    bs, text, doc_off = _pack(_fuzz_docs(random.Random(8), 100))
    ref = _device_call(enc, text, doc_off, 16, 4, True)
    s = torch.cuda.Stream()
    host = torch.from_numpy(np.ascontiguousarray(text)).pin_memory()
    with torch.cuda.stream(s):
        d_text = torch.empty(len(text), dtype=torch.uint8, device="cuda")
        torch.cuda._sleep(20_000_000)                                    # (the copy lands late on this stream)
        d_text.copy_(host, non_blocking=True)
        d_off = torch.from_numpy(doc_off).to("cuda", non_blocking=True)
        out = enc.chunk_batch_device(d_text, d_off, 16, 4, ordinary=True, pad_id=PAD)
    s.synchronize()
    for k in ref:
        assert np.array_equal(out[k].cpu().numpy(), ref[k]), k


def test_bad_arguments(jt):
    import torch
    N = jt._native
    L = N.lib()
    enc = jt.get_encoding("cl100k_base")
    b = enc.new_batch()
    nc = C.c_int64(0)
    assert L.jtk_batch_chunk(b._h, 4, 0, None, C.byref(nc)) == N.JTK_ERR_INVALID_ARGUMENT      # no encode yet
    _, text, doc_off = _pack(["some text here", "more"])
    b.encode_host(text, doc_off)
    for n_, ov in ((0, 0), (-1, 0), (4, 4), (4, 5), (4, -1), (1 << 31, 0)):
        assert L.jtk_batch_chunk(b._h, n_, ov, None, C.byref(nc)) == N.JTK_ERR_INVALID_ARGUMENT, (n_, ov)
    assert L.jtk_batch_chunk(b._h, 4, 3, None, C.byref(nc)) == N.JTK_OK
    b.encode_host(text, doc_off, count_only=True)
    assert L.jtk_batch_chunk(b._h, 4, 0, None, C.byref(nc)) == N.JTK_ERR_INVALID_ARGUMENT
    assert L.jtk_batch_token_offsets(b._h, None, None) == N.JTK_ERR_INVALID_ARGUMENT
    assert L.jtk_batch_chunk_fetch(b._h, None, None, None, None, None, None, None) == N.JTK_ERR_INVALID_ARGUMENT
    d_text = torch.from_numpy(np.ascontiguousarray(text)).cuda()
    d_off = torch.from_numpy(doc_off).cuda()
    rows = torch.empty((2, 4), dtype=torch.int32, device="cuda")
    aux = [torch.empty(2, dtype=dt, device="cuda") for dt in (torch.int64, torch.bool, torch.int32)]
    b.encode_device_max_tokens(d_text.data_ptr(), d_off.data_ptr(), 2, len(text), 4, rows.data_ptr(), aux[0].data_ptr(),
                               aux[1].data_ptr(), aux[2].data_ptr())
    assert L.jtk_batch_chunk(b._h, 4, 0, None, C.byref(nc)) == N.JTK_ERR_INVALID_ARGUMENT
    with pytest.raises(ValueError):
        enc.chunk_batch_device(d_text, d_off, 4, 4)
    b.close()
