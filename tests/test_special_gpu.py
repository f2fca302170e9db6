"""JTK_ENCODE_ALLOW_SPECIAL / allowed_special=: allowed special-token literals encoded as their ids in batch encodes.  Every
result is checked against the plain restatement tests/special_ref.py (matches by the rule, segments by the CPU oracle's
encodeOrdinary).  Every test here needs a real MI355X (`-m gpu`)."""
import ctypes as C
import os
import random

import numpy as np
import pytest

import golden_util
import oracle_lib
import regex_crosscheck as rc
import special_ref

pytestmark = pytest.mark.gpu

EOT = "<|endoftext|>"


@pytest.fixture(scope="module")
def jt():
    import jtokkit_amd
    return jtokkit_amd


def _pack(texts):
    bs = [t if isinstance(t, (bytes, bytearray)) else t.encode("utf-8") for t in texts]
    doc_off = np.zeros(len(bs) + 1, dtype=np.int64)
    np.cumsum([len(x) for x in bs], out=doc_off[1:])
    text = np.frombuffer(b"".join(bs), dtype=np.uint8) if doc_off[-1] else np.zeros(0, dtype=np.uint8)
    return bs, text, doc_off


def _amap(specials, allowed=None):
    return {k.encode(): v for k, v in specials.items() if allowed is None or k in allowed}


def _check(res, o, bs, specials, allowed=None, ordinary=False, validate=False):
    lits = [k.encode() for k in specials]
    amap = _amap(specials, allowed)
    for d, doc in enumerate(bs):
        if validate:
            try:
                doc.decode("utf-8")
            except UnicodeDecodeError:
                assert res.status[d] == -6, d
                assert res.tok_off[d + 1] == res.tok_off[d]
                continue
        exp = special_ref.encode(o, doc, amap, lits, ordinary)
        if exp is None:
            assert res.status[d] == -2, d
            assert res.tok_off[d + 1] == res.tok_off[d], d
        else:
            assert res.status[d] == 0, (d, doc[:80])
            assert res.doc(d).tolist() == exp, (d, doc[:80])


def _insertions(rng, base, lits):
    """Literals at the start, the end, adjacent, as the whole document, after white space, between digits, inside words,
    next to multi-byte characters."""
    docs = []
    for lit in lits:
        docs += [lit, lit + lit, lit + base, base + lit, base[:len(base) // 2] + lit + base[len(base) // 2:],
                 "  " + lit + "  x", "12" + lit + "345", "foo" + lit + "bar", "日本" + lit + "語", "\U0001F355" + lit,
                 "it" + lit + "'s", "a\n\n" + lit + "\n b", lit + " " + rng.choice(lits) + rng.choice(lits) + "1234567"]
    return docs


def _fuzz(rng, lits, n=150):
    out = []
    for _ in range(n):
        parts = [rc.random_text(rng, rng.randint(0, 40))]
        for _ in range(rng.randint(0, 3)):
            parts.append(rng.choice(lits) + rc.random_text(rng, rng.randint(0, 20)))
        out.append("".join(parts))
    return out


def test_empty_set_equals_call_without_flag(jt):
    """With an empty allowed set the flag changes nothing: tokens, offsets, status, host and device input, both encodes."""
    import torch
    enc = jt.get_encoding("cl100k_base")
    rng = random.Random(1)
    lits = list(oracle_lib.ENCODINGS["cl100k_base"]["specials"])
    texts = [r[0] for r in golden_util.load_rows("cl100k_base")] + _fuzz(rng, lits) + _insertions(rng, "hello world", lits)
    from jtokkit_amd import corpus
    t2, o2 = corpus.mixed(40, mean_bytes=1500, seed=4)
    texts += [t2[o2[d]:o2[d + 1]].tobytes() for d in range(40)]
    bs, text, doc_off = _pack(texts)
    b = enc.new_batch()
    b.set_allowed_special([])
    d_text, d_off = torch.from_numpy(text.copy()).cuda(), torch.from_numpy(doc_off).cuda()
    for ordinary in (False, True):
        b.encode_host(text, doc_off, ordinary)
        ref = b.fetch()
        assert (ref.status == -2).any() or ordinary
        b.encode_host(text, doc_off, ordinary, allow_special=True)
        got = b.fetch()
        assert np.array_equal(got.tokens, ref.tokens) and np.array_equal(got.tok_off, ref.tok_off)
        assert np.array_equal(got.status, ref.status)
        b.encode_device(d_text.data_ptr(), d_off.data_ptr(), len(bs), len(text), ordinary, allow_special=True)
        got = b.fetch()
        assert np.array_equal(got.tokens, ref.tokens) and np.array_equal(got.status, ref.status)
    b.close()


@pytest.mark.parametrize("name", golden_util.ENCODING_NAMES)
def test_all_allowed_four_encodings(jt, name):
    enc = jt.get_encoding(name)
    o = oracle_lib.get(name)
    specials = oracle_lib.ENCODINGS[name]["specials"]
    lits = list(specials)
    rng = random.Random(len(name))
    rows = [r[0] for r in golden_util.load_rows(name)]
    texts = list(rows)
    for base in rows[:25]:
        texts += _insertions(rng, base, lits)
    texts += _fuzz(rng, lits)
    bs, text, doc_off = _pack(texts)
    for ordinary in (False, True):
        res = enc.encode_batch(bs, ordinary=ordinary, allowed_special="all")
        _check(res, o, bs, specials, ordinary=ordinary)
    assert (np.diff(res.tok_off) > 0).sum() > len(bs) // 2
    for d in range(0, len(bs), 7):
        assert enc.decode_bytes(res.doc(d).tolist()) == bs[d]
    # one document at a time
    assert enc.encode_with_special_tokens("foo  " + EOT) == special_ref.encode(o, ("foo  " + EOT).encode(), _amap(specials))
    if name == "cl100k_base":
        assert enc.encode_with_special_tokens("foo  " + EOT) == [8134, 256, 100257]
        assert enc.encode_with_special_tokens("it" + EOT + "'s") == [275, 100257, 596]


def test_invalid_bytes_with_validate(jt):
    enc = jt.get_encoding("cl100k_base")
    o = oracle_lib.get("cl100k_base")
    specials = oracle_lib.ENCODINGS["cl100k_base"]["specials"]
    e = EOT.encode()
    docs = [b"ab\x80" + e + b"cd", b"\xe6\x97" + e, e + b"\x97\xa5", b"ok " + e + b" fine", b"\xff", e + b"\xe6\x97\xa5" + e,
            b"x" + e + b"\xc3", b"\xc3" + e + b"\xa9"]
    bs, text, doc_off = _pack(docs)
    b = enc.new_batch()
    b.set_allowed_special(None)
    b.encode_host(text, doc_off, ordinary=False, validate=True, allow_special=True)
    _check(b.fetch(), o, bs, specials, validate=True)
    b.close()


def test_subset_allowed(jt):
    enc = jt.get_encoding("cl100k_base")
    o = oracle_lib.get("cl100k_base")
    specials = oracle_lib.ENCODINGS["cl100k_base"]["specials"]
    rng = random.Random(3)
    texts = _fuzz(rng, list(specials), 300) + ["a<|fim_prefix|>b" + EOT, EOT + "<|endofprompt|>", "<|endoftext<|endofprompt|>|>"]
    bs = [t.encode() for t in texts]
    for allowed in ([EOT], ["<|fim_prefix|>", "<|endofprompt|>"]):
        for ordinary in (False, True):
            res = enc.encode_batch(bs, ordinary=ordinary, allowed_special=allowed)
            _check(res, o, bs, specials, allowed=allowed, ordinary=ordinary)
            if not ordinary:
                assert (res.status == -2).any()
    with pytest.raises(jt.UnsupportedOperationError):
        enc.encode_with_special_tokens("x<|fim_prefix|>" + EOT, allowed_special=[EOT])
    assert enc.encode_with_special_tokens("x<|fim_prefix|>" + EOT, allowed_special=[EOT], ordinary=True) == \
        o.encode_ordinary(b"x<|fim_prefix|>") + [100257]


def _custom(jt, specials):
    from jtokkit_amd.encoding import HipEncoding
    with open(os.path.join(oracle_lib.DATA_DIR, "cl100k_base.tiktoken"), "rb") as f:
        data = f.read()
    return HipEncoding("cl100k_custom", 1, data, specials)


@pytest.mark.parametrize("sets", [("aa", "aaa", "a"), ("<a>", "<a>b"), ("日本", "日"), ("xyx", "yxy", "x")])
def test_custom_overlapping_literals(jt, sets):
    specials = {lit: 100300 + i for i, lit in enumerate(sets)}
    enc = _custom(jt, specials)
    o = oracle_lib.get("cl100k_base")
    rng = random.Random(len(sets[0]))
    alphabet = sorted({c for x in sets for c in x}) + [" ", "<", "z", "1"]
    texts = ["".join(rng.choice(alphabet + list(sets)) for _ in range(rng.randint(0, 60))) for _ in range(400)]
    bs = [t.encode() for t in texts]
    b = enc.new_batch()
    for allowed in (None, [sets[0]], list(sets[1:])):
        ids = [specials[x] for x in allowed] if allowed is not None else None
        b.set_allowed_special(ids)
        for ordinary in (True, False):
            _, text, doc_off = _pack(bs)
            b.encode_host(text, doc_off, ordinary, allow_special=True)
            _check(b.fetch(), o, bs, specials, allowed=allowed, ordinary=ordinary)
    b.close()
    enc.close()


def test_count_only_to_host_and_device_stream(jt):
    import torch
    enc = jt.get_encoding("p50k_edit")
    o = oracle_lib.get("p50k_edit")
    specials = oracle_lib.ENCODINGS["p50k_edit"]["specials"]
    rng = random.Random(9)
    bs, text, doc_off = _pack(_fuzz(rng, list(specials), 500))
    b = enc.new_batch()
    b.set_allowed_special(None)
    b.encode_host(text, doc_off, False, allow_special=True)
    ref = b.fetch()
    _check(ref, o, bs, specials)
    b.encode_host(text, doc_off, False, count_only=True, allow_special=True)
    counts, status = b.fetch_counts()
    assert np.array_equal(counts, np.diff(ref.tok_off)) and np.array_equal(status, ref.status)
    assert enc.count_tokens_batch(bs, ordinary=True, allowed_special="all") == \
        [len(special_ref.encode(o, x, _amap(specials), ordinary=True)) for x in bs]
    b.encode_host(text, doc_off, False, to_host=True, allow_special=True)
    h = b.host_result()
    assert np.array_equal(h.tokens, ref.tokens) and np.array_equal(h.tok_off, ref.tok_off) and np.array_equal(h.status, ref.status)
    # device input on a caller's stream: the text is written on that stream just before the encode
    s = torch.cuda.Stream()
    pinned = torch.from_numpy(text.copy()).pin_memory()
    d_text = torch.zeros(len(text) + 64, dtype=torch.uint8, device="cuda")
    d_off = torch.from_numpy(doc_off).cuda()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        d_text[:len(text)].copy_(pinned, non_blocking=True)
    nt = b.encode_device(d_text.data_ptr(), d_off.data_ptr(), len(bs), len(text), False, stream=s.cuda_stream, allow_special=True)
    assert nt == len(ref.tokens)
    got = b.fetch()
    assert np.array_equal(got.tokens, ref.tokens) and np.array_equal(got.status, ref.status)
    b.encode_device(d_text.data_ptr(), d_off.data_ptr(), len(bs), len(text), False, stream=s.cuda_stream, allow_special=True,
                    count_only=True)
    counts, _ = b.fetch_counts()
    assert np.array_equal(counts, np.diff(ref.tok_off))
    b.close()


def test_multi_chunk_equals_one_chunk(jt, ):
    import torch
    from jtokkit_amd import corpus, _native as N
    enc = jt.get_encoding("cl100k_base")
    text, doc_off = corpus.mixed(300, mean_bytes=3000, seed=12)
    rng = random.Random(12)
    docs = [text[doc_off[d]:doc_off[d + 1]].tobytes() for d in range(len(doc_off) - 1)]
    docs = [x[:rng.randint(0, len(x))] + EOT.encode() * rng.randint(0, 3) + x[len(x) // 2:] for x in docs]
    bs, text, doc_off = _pack(docs)
    assert len(text) > 4 * 65536
    big = enc.new_batch()
    big.encode_host(text, doc_off, False, allow_special=True)
    ref = big.fetch()
    assert int((ref.tokens == 100257).sum()) > 200 and (ref.status == 0).all()
    for d in range(0, len(bs), 5):
        assert enc.decode_bytes(ref.doc(d).tolist()) == bs[d]
    small = enc.new_batch()
    small.set_option(N.JTK_OPT_CHUNK_BYTES, 65536)
    small.set_option(N.JTK_OPT_HOST_CHUNK_BYTES, 65536)
    for to_host in (False, True):
        small.encode_host(text, doc_off, False, to_host=to_host, allow_special=True)
        got = small.host_result() if to_host else small.fetch()
        assert np.array_equal(got.tokens, ref.tokens) and np.array_equal(got.tok_off, ref.tok_off)
    d_text, d_off = torch.from_numpy(text.copy()).cuda(), torch.from_numpy(doc_off).cuda()
    small.encode_device(d_text.data_ptr(), d_off.data_ptr(), len(bs), len(text), False, allow_special=True)
    got = small.fetch()
    assert np.array_equal(got.tokens, ref.tokens) and np.array_equal(got.status, ref.status)
    big.close()
    small.close()


def test_headline_documents_with_literals(jt):
    """200k headline documents with literals sprinkled in (device input), sampled against the restatement."""
    import torch
    from jtokkit_amd import corpus
    enc = jt.get_encoding("cl100k_base")
    o = oracle_lib.get("cl100k_base")
    specials = oracle_lib.ENCODINGS["cl100k_base"]["specials"]
    text, doc_off = corpus.mixed(200000, seed=3)
    text = np.array(text, dtype=np.uint8)
    rng = np.random.default_rng(5)
    # overwrite ~1 position per 4 KB with a literal (inside documents that are long enough)
    lit = EOT.encode()
    starts = np.sort(rng.choice(len(text) - 64, size=len(text) // 4096, replace=False))
    for p in starts:
        text[p:p + len(lit)] = np.frombuffer(lit, dtype=np.uint8)
    d_text, d_off = torch.from_numpy(text).cuda(), torch.from_numpy(np.asarray(doc_off)).cuda()
    b = enc.new_batch()
    b.set_allowed_special(None)
    b.encode_device(d_text.data_ptr(), d_off.data_ptr(), len(doc_off) - 1, len(text), True, allow_special=True)
    res = b.fetch()
    n_special = int((res.tokens == 100257).sum())
    assert n_special > len(starts) // 2
    sample = random.Random(2).sample(range(len(doc_off) - 1), 300)
    for d in sample:
        doc = text[doc_off[d]:doc_off[d + 1]].tobytes()
        try:
            exp = special_ref.encode(o, doc, _amap(specials), ordinary=True)
        except oracle_lib.OracleError:                     # (a literal cut a character: malformed segment for the oracle)
            continue
        assert res.doc(d).tolist() == exp, d
    b.close()


def test_consecutive_and_shard(jt):
    enc = jt.get_encoding("cl100k_base")
    o = oracle_lib.get("cl100k_base")
    specials = oracle_lib.ENCODINGS["cl100k_base"]["specials"]
    res = enc.encode_batch([EOT * 100000, "x" + EOT * 3 + "y"], allowed_special=[EOT])
    assert res.doc(0).tolist() == [100257] * 100000 and res.status.tolist() == [0, 0]
    assert res.doc(1).tolist() == special_ref.encode(o, ("x" + EOT * 3 + "y").encode(), _amap(specials, [EOT]))
    from jtokkit_amd import corpus
    text, off = corpus.english(2000, seed=6)
    shard = EOT.encode().join(text[off[d]:off[d + 1]].tobytes() for d in range(2000))
    res = enc.encode_batch([shard], allowed_special=[EOT])
    assert res.status[0] == 0
    assert res.doc(0).tolist() == special_ref.encode(o, shard, _amap(specials, [EOT]))
    assert int((res.tokens == 100257).sum()) == 1999


def test_chunks_and_offsets_after_allow_special(jt):
    import torch
    enc = jt.get_encoding("cl100k_base")
    specials = oracle_lib.ENCODINGS["cl100k_base"]["specials"]
    rng = random.Random(21)
    bs, text, doc_off = _pack(_fuzz(rng, list(specials), 200) + [EOT * 5, "日" + EOT + "本"])
    b = enc.new_batch()
    b.set_allowed_special(None)
    b.encode_host(text, doc_off, True, allow_special=True)
    res = b.fetch()
    id2lit = {v: k.encode() for k, v in specials.items()}
    pos = torch.empty(max(len(res.tokens), 1), dtype=torch.int64, device="cuda")
    b.token_offsets(pos.data_ptr())
    torch.cuda.synchronize()
    pos = pos.cpu().numpy()[:len(res.tokens)]
    n_sp = 0
    for t, tid in enumerate(res.tokens.tolist()):
        if tid in id2lit:
            lit = id2lit[tid]
            assert text[pos[t]:pos[t] + len(lit)].tobytes() == lit, t
            n_sp += 1
    assert n_sp > 100
    nc = b.chunk(1, 0)
    f = b.chunk_fetch()
    assert nc == len(res.tokens)
    for c in range(nc):
        tid = int(res.tokens[f["tok_begin"][c]])
        if tid in id2lit:
            assert text[f["byte_begin"][c]:f["byte_end"][c]].tobytes() == id2lit[tid]
            assert not f["split"][c]
    with pytest.raises(jt.encoding.EncodingError) as ei:
        b.truncate(4)
    assert ei.value.code == -1
    b.close()
    # the wrappers
    out = enc.chunk_batch(["a" + EOT + "b"], 1, allowed_special="all")
    assert [(t, s, e) for (t, s, e, _) in out[0]][1] == ([100257], 1, 1 + len(EOT))
    d_text = torch.from_numpy(np.frombuffer(("a" + EOT + "b").encode(), dtype=np.uint8).copy()).cuda()
    d_off = torch.tensor([0, len(EOT) + 2], dtype=torch.int64, device="cuda")
    dev = enc.chunk_batch_device(d_text, d_off, 2, allowed_special="all")
    assert dev["rows"].cpu().tolist()[0] == [64, 100257]


def test_rejections(jt):
    from jtokkit_amd import _native as N
    L = N.lib()
    enc = jt.get_encoding("cl100k_base")
    b = enc.new_batch()
    A = N.JTK_ENCODE_ALLOW_SPECIAL
    text = b"a" + EOT.encode()
    off = np.array([0, len(text)], dtype=np.int64)
    pb, pe = np.array([0], dtype=np.int64), np.array([1], dtype=np.int64)
    nt = C.c_int64(0)
    assert L.jtk_batch_encode_pieces(b._h, text, off.ctypes.data, 1, pb.ctypes.data, pe.ctypes.data, 1, A, C.byref(nt)) == -1
    toks = np.zeros(64, dtype=np.int64)
    i32 = np.zeros(64, dtype=np.int32)
    u8 = np.zeros(64, dtype=np.uint8)
    assert L.jtk_batch_encode_max_tokens(b._h, text, off.ctypes.data, 1, A, 4, i32.ctypes.data, toks.ctypes.data, u8.ctypes.data,
                                         i32.ctypes.data) == -1
    tr = C.c_int(0)
    assert L.jtk_encode(b._h, text, len(text), A, -1, i32.ctypes.data, 64, C.byref(nt), C.byref(tr)) == -1
    svc = enc._service()
    assert L.jtk_service_encode(svc, text, len(text), A, -1, i32.ctypes.data, 64, C.byref(nt), C.byref(tr)) == -1
    with pytest.raises(jt.encoding.EncodingError):
        b.set_allowed_special([5])                          # an ordinary id
    with pytest.raises(ValueError):
        enc.encode_batch(["x"], allowed_special=["<|nope|>"])
    with pytest.raises(ValueError):
        enc.encode_batch(["x"], allowed_special="none")
    import torch
    d = torch.zeros(64, dtype=torch.uint8, device="cuda")
    d_off = torch.tensor([0, 1], dtype=torch.int64, device="cuda")
    rows = torch.zeros(8, dtype=torch.int32, device="cuda")
    k = torch.zeros(1, dtype=torch.int64, device="cuda")
    st = torch.zeros(1, dtype=torch.int32, device="cuda")
    tr8 = torch.zeros(1, dtype=torch.uint8, device="cuda")
    assert L.jtk_batch_encode_device_max_tokens(b._h, d.data_ptr(), d_off.data_ptr(), 1, 1, A, 4, -1, rows.data_ptr(), k.data_ptr(),
                                                tr8.data_ptr(), st.data_ptr(), None) == -1
    import regex
    ranks = {bytes([i]): i for i in range(256)}
    penc = jt.new_custom_encoding("hostpat", 1, ranks, {EOT: 300}, host_pattern=regex.compile(r"\w+|\s+|[^\w\s]+"))
    with pytest.raises(ValueError):
        penc.encode_batch(["x"], allowed_special="all")
    penc.close()
    b.close()
