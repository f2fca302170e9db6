"""Compact token ids on the device and over the link: jtk_batch_compact (the post-pass), JTK_ENCODE_COMPACT_IDS with
JTK_ENCODE_TO_HOST (the host pipeline), jtk_batch_host_result_compact, jtk_widen_ids and the Python surface over them.  The
yardstick is always the plain int32 result of the same batch -- which the parity tests pin to the CPU oracle --, restated as
planes by tests/compact_ref.py; no result of the compact route is compared with another.  Every comparison is exact.  Every test
here needs a real MI355X (`-m gpu`)."""
import ctypes as C

import numpy as np
import pytest

import compact_ref
import golden_util

pytestmark = pytest.mark.gpu

EOT = "<|endoftext|>"
GUARD = -2            # fills the device planes before a pass; the entries behind a plane must keep it


@pytest.fixture(scope="module")
def jt():
    import jtokkit_amd
    return jtokkit_amd


def _pack(texts):
    bs = [t if isinstance(t, (bytes, bytearray)) else t.encode("utf-8") for t in texts]
    doc_off = np.zeros(len(bs) + 1, dtype=np.int64)
    if bs:
        np.cumsum([len(x) for x in bs], out=doc_off[1:])
    text = np.frombuffer(b"".join(bs), dtype=np.uint8) if doc_off[-1] else np.zeros(0, dtype=np.uint8)
    return text, doc_off


def _same_planes(lo, hi, ids, hb):
    exp_lo, exp_hi = compact_ref.compact(ids, hb)
    assert lo.dtype == np.uint16 and np.array_equal(lo, exp_lo)
    if hb == 0:
        assert hi is None or len(hi) == 0
    else:
        assert hi.dtype == np.uint32 and np.array_equal(hi, exp_hi)


def _post_pass(b, hb, shift=0):
    """jtk_batch_compact of the batch's last encode into guarded torch buffers; returns (lo, hi) as numpy planes.  shift = 1:
    the planes start one entry into the allocation (2 and 4 bytes past a 16-byte boundary: the pass without 16-byte accesses)."""
    import torch
    nt = b.result()[0]
    nw = compact_ref.hi_words(nt, hb)
    lo_t = torch.full((nt + 16 + shift,), GUARD, dtype=torch.int16, device="cuda")
    hi_t = torch.full((nw + 8 + shift,), GUARD, dtype=torch.int32, device="cuda")
    assert lo_t.data_ptr() % 16 == 0 and hi_t.data_ptr() % 16 == 0
    torch.cuda.synchronize()              # (the fills run on torch's stream, the pass on the batch's own: no order between them)
    b.compact(lo_t.data_ptr() + 2 * shift, hi_t.data_ptr() + 4 * shift if hb else None)
    torch.cuda.synchronize()
    lo = lo_t.cpu().numpy()
    hi = hi_t.cpu().numpy()
    assert (lo[:shift] == GUARD).all() and (hi[:shift] == GUARD).all()    # nothing before the planes
    lo, hi = lo[shift:], hi[shift:]
    assert (lo[nt:] == GUARD).all() and (hi[nw:] == GUARD).all()          # nothing behind the planes
    if hb == 0:
        assert (hi == GUARD).all()
    return lo[:nt].view(np.uint16), (hi[:nw].view(np.uint32) if hb else None)


def _check_post_pass(b, hb):
    before = b.fetch()
    for shift in (0, 1):
        lo, hi = _post_pass(b, hb, shift)
        _same_planes(lo, hi, before.tokens, hb)
    after = b.fetch()
    assert np.array_equal(after.tokens, before.tokens) and np.array_equal(after.tok_off, before.tok_off)
    assert np.array_equal(after.status, before.status)
    return before


# ---- the post-pass ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", golden_util.ENCODING_NAMES)
def test_post_pass_equals_the_reference_planes(jt, name):
    from jtokkit_amd import corpus
    enc = jt.get_encoding(name)
    hb = enc.id_bits - 16
    assert enc.id_bits == (17 if name == "cl100k_base" else 16)
    b = enc.new_batch()
    prompts = [p for (p, _, _) in golden_util.load_rows(name)]
    text, doc_off = _pack(prompts)
    b.encode_host(text, doc_off, ordinary=True)
    res = _check_post_pass(b, hb)
    assert len(res.tokens) > 1000
    if hb:
        assert res.tokens.max() >= 65536                # the high plane is not all zero
    mtext, moff = corpus.mixed(600, mean_bytes=2048, lo=16, hi=16384)
    b.encode_host(mtext, moff, ordinary=True)
    res = _check_post_pass(b, hb)
    assert len(res.tokens) > 100000
    # a device-input encode with special tokens allowed
    import torch
    stext, soff = _pack(["a" + EOT + "b", EOT * 40, "", "plain text " * 30, "x" + EOT])
    d_text = torch.zeros(len(stext) + 32, dtype=torch.uint8, device="cuda")
    d_text[:len(stext)] = torch.from_numpy(stext.copy()).cuda()
    d_off = torch.from_numpy(soff).cuda()
    torch.cuda.synchronize()
    b.set_allowed_special("all")
    b.encode_device(d_text.data_ptr(), d_off.data_ptr(), len(soff) - 1, len(stext), ordinary=False, allow_special=True)
    res = _check_post_pass(b, hb)
    assert (res.tokens == enc.special_ids([EOT])[0]).sum() == 42                   # 1 + 40 + 1 literals
    b.close()


def test_post_pass_edges(jt):
    enc = jt.get_encoding("cl100k_base")
    b = enc.new_batch()
    cases = [[], ["", "", ""], [EOT, "x" + EOT + "y", EOT * 3], ["a"], ["", "a", ""]]
    for k, texts in enumerate(cases):
        text, doc_off = _pack(texts)
        nt = b.encode_host(text, doc_off, ordinary=False)            # encode(): a special literal refuses the document
        res = _check_post_pass(b, 1)
        if k == 2:
            assert (res.status < 0).all()            # (every document refused; the planes follow the id buffer as it is)
        if k in (3, 4):
            assert nt == 1
        # with nothing to write the planes may be NULL
        if nt == 0:
            b.compact(None, None)
    b.close()


# ---- the host pipeline --------------------------------------------------------------------------------------------------

def _plain_then_compact(jt, b, text, doc_off, hb, pieces=None, **kw):
    """The same input through the plain to_host route and the compact one on the same batch; the compact result widened must
    equal the plain one, and fetch / chunk / pack after it what they give after the plain encode.  Returns the plain result."""
    def run(compact):
        if pieces is not None:
            nt = b.encode_pieces(text, doc_off, pieces[0], pieces[1], to_host=True, compact=compact, **kw)
        else:
            nt = b.encode_host(text, doc_off, to_host=True, compact=compact, **kw)
        after = {}
        f = b.fetch()
        after["fetch"] = (f.tokens.copy(), f.tok_off.copy(), f.status.copy())
        b.chunk(37, 5)
        after["chunk"] = b.chunk_fetch()
        b.pack(64, -1)
        after["pack"] = b.pack_fetch(-1)
        return nt, after

    nt_p, after_p = run(False)
    plain = b.host_result()
    p_tok, p_off, p_st = plain.tokens[:nt_p].copy(), plain.tok_off.copy(), plain.status.copy()
    assert np.array_equal(after_p["fetch"][0], p_tok)
    nt_c, after_c = run(True)
    assert nt_c == nt_p
    with pytest.raises(jt.EncodingError) as e:
        b.host_result()
    assert e.value.code == jt._native.JTK_ERR_INVALID_ARGUMENT and "jtk_batch_host_result_compact" in str(e.value)
    r = b.host_result_compact()
    assert r.id_bits == 16 + hb and len(r) == len(doc_off) - 1
    assert np.array_equal(r.tok_off, p_off) and np.array_equal(r.status, p_st)
    _same_planes(r.lo, r.hi, p_tok, hb)
    assert np.array_equal(r.widen(), p_tok)
    for d in {0, len(r) // 2, len(r) - 1} if len(r) else ():
        assert np.array_equal(r.doc(d), p_tok[p_off[d]:p_off[d + 1]])
    for a, c in zip(after_p["fetch"], after_c["fetch"]):
        assert np.array_equal(a, c)
    for key in ("chunk", "pack"):
        assert after_p[key].keys() == after_c[key].keys()
        for k2 in after_p[key]:
            assert np.array_equal(after_p[key][k2], after_c[key][k2]), (key, k2)
    return p_tok, p_off, p_st


def _chunk_starts(doc_off, cb):
    """First documents of the host chunks, by the plan of jtk_batch_encode."""
    n_bytes = int(doc_off[-1])
    starts, nxt = [0], cb
    for d in range(len(doc_off) - 1):
        if doc_off[d] >= nxt and d > starts[-1] and n_bytes - doc_off[d] > cb // 4:
            starts.append(d)
            nxt = int(doc_off[d]) + cb
    return starts


@pytest.mark.parametrize("in_flight", [1, 2, 3, 4])
def test_pipeline_of_many_chunks_with_ragged_token_boundaries(jt, in_flight):
    from jtokkit_amd import corpus
    enc = jt.get_encoding("cl100k_base")
    text, doc_off = corpus.mixed(1500, mean_bytes=2048, lo=16, hi=16384, seed=11)
    cb = 64 << 10
    b = enc.new_batch()
    b.set_option(jt._native.JTK_OPT_HOST_CHUNK_BYTES, cb)
    b.set_option(jt._native.JTK_OPT_CHUNKS_IN_FLIGHT, in_flight)
    p_tok, p_off, _ = _plain_then_compact(jt, b, text, doc_off, 1, ordinary=True)
    starts = _chunk_starts(doc_off, cb)
    bounds = [int(p_off[d]) for d in starts[1:]]
    assert len(bounds) >= 24                                            # dozens of chunks ...
    assert sum(1 for t in bounds if t % 32) >= len(bounds) * 3 // 4     # ... that start inside a word of the high plane
    assert len(set(bounds)) == len(bounds) and p_tok.max() >= 65536
    b.close()


def test_pinned_planes_grow_in_mid_job(jt):
    import random
    enc = jt.get_encoding("cl100k_base")
    rng = random.Random(21)
    dense = ["😀", "🤖", "🧪", "\x01", "\x7f", "1,", "²", "\u0601", "🀄", "𝔘"]
    docs = ["".join(rng.choice(dense) for _ in range(rng.randint(1, 400))).encode("utf-8") for _ in range(6000)]
    text, doc_off = _pack(docs)
    assert len(text) > 2.5e6
    b = enc.new_batch()                                                 # (a fresh batch: its pinned buffers start at the guess)
    b.set_option(jt._native.JTK_OPT_HOST_CHUNK_BYTES, 256 << 10)
    nt = b.encode_host(text, doc_off, ordinary=True, to_host=True, compact=True)
    assert nt * 2 > len(text)                                          # more than one token per two bytes: the guess is too small
    r = b.host_result_compact()
    lo, hi = r.lo.copy(), r.hi.copy()
    f = b.fetch()
    _same_planes(lo, hi, f.tokens, 1)
    _plain_then_compact(jt, b, text, doc_off, 1, ordinary=True)
    from jtokkit_amd import corpus
    t2, o2 = corpus.english(3000)
    _plain_then_compact(jt, b, t2, o2, 1, ordinary=True)            # a sparse text right after on the grown buffers
    b.close()


@pytest.mark.parametrize("name", ["cl100k_base", "r50k_base"])
def test_small_and_tiny_jobs(jt, name):
    from jtokkit_amd import corpus
    enc = jt.get_encoding(name)
    hb = enc.id_bits - 16
    b = enc.new_batch()
    for n_docs, mean in ((1, 64), (27, 200), (60, 1500), (300, 2500)):          # < 128 KiB twice, then < 1 MiB twice
        text, doc_off = corpus.mixed(n_docs, mean_bytes=mean, lo=1, hi=8 * mean, seed=n_docs)
        assert len(text) <= 1 << 20
        p_tok, _, _ = _plain_then_compact(jt, b, text, doc_off, hb, ordinary=True)
        assert len(p_tok) > 0
    assert len(text) > 128 << 10
    _plain_then_compact(jt, b, *_pack([]), hb, ordinary=True)
    _plain_then_compact(jt, b, *_pack(["", ""]), hb, ordinary=True)
    _plain_then_compact(jt, b, *_pack(["a"]), hb, ordinary=True)
    b.close()


def test_allow_special_and_a_document_full_of_literals(jt):
    from jtokkit_amd import corpus
    enc = jt.get_encoding("cl100k_base")
    text, doc_off = corpus.english(400)
    docs = [text[doc_off[d]:doc_off[d + 1]].tobytes() for d in range(len(doc_off) - 1)]
    docs[3] = (EOT + "<|fim_prefix|>") * 500
    docs[100] = b"head " + EOT.encode() + b" tail"
    docs[399] = docs[399] + EOT.encode()
    stext, soff = _pack(docs)
    b = enc.new_batch()
    b.set_allowed_special("all")
    for cb in (64 << 10, 32 << 20):
        b.set_option(jt._native.JTK_OPT_HOST_CHUNK_BYTES, cb)
        p_tok, p_off, _ = _plain_then_compact(jt, b, stext, soff, 1, ordinary=False, allow_special=True)
        assert p_tok[p_off[3]:p_off[4]].tolist() == [100257, 100258] * 500
        # without a literal in the batch the flag runs the plain pipeline: compact there too
        _plain_then_compact(jt, b, text, doc_off, 1, ordinary=False, allow_special=True)
    # a tiny one
    _plain_then_compact(jt, b, *_pack([EOT, "x", EOT + EOT]), 1, ordinary=False, allow_special=True)
    b.close()


def test_encode_pieces(jt):
    from jtokkit_amd import corpus
    enc = jt.get_encoding("cl100k_base")
    text, doc_off = corpus.english(800)
    begin, end = [], []
    for d in range(len(doc_off) - 1):                       # pieces of up to 9 bytes, every fourth one left out
        for k, p in enumerate(range(int(doc_off[d]), int(doc_off[d + 1]), 9)):
            if k % 4 != 3:
                begin.append(p)
                end.append(min(p + 9, int(doc_off[d + 1])))
    pieces = (np.array(begin, dtype=np.int64), np.array(end, dtype=np.int64))
    b = enc.new_batch()
    for cb in (64 << 10, 32 << 20):
        b.set_option(jt._native.JTK_OPT_HOST_CHUNK_BYTES, cb)
        _plain_then_compact(jt, b, text, doc_off, 1, pieces=pieces, ordinary=True)
    b.close()


def test_python_surface(jt):
    from jtokkit_amd import corpus
    import torch
    enc = jt.get_encoding("cl100k_base")
    text, doc_off = corpus.mixed(200, mean_bytes=1024, lo=16, hi=8192)
    plain = enc.encode_batch_packed(text, doc_off, ordinary=True)
    r = enc.encode_batch_packed(text, doc_off, ordinary=True, compact=True)
    assert isinstance(r, jt.CompactBatchResult) and r.id_bits == enc.id_bits == 17 and len(r) == len(plain)
    _same_planes(r.lo, r.hi, plain.tokens, 1)
    assert np.array_equal(r.widen(), plain.tokens) and np.array_equal(r.doc(7), plain.doc(7))
    assert np.array_equal(r.tok_off, plain.tok_off) and np.array_equal(r.status, plain.status)
    d_text = torch.from_numpy(text.copy()).cuda()
    d_off = torch.from_numpy(doc_off).cuda()
    lo, hi, tok_off, status = enc.compact_batch_device(d_text, d_off, ordinary=True)
    torch.cuda.synchronize()
    assert lo.dtype == torch.uint16 and hi.dtype == torch.int32
    _same_planes(lo.cpu().numpy(), hi.cpu().numpy().view(np.uint32), plain.tokens, 1)
    assert np.array_equal(tok_off.cpu().numpy(), plain.tok_off) and np.array_equal(status.cpu().numpy(), plain.status)
    r50 = jt.get_encoding("r50k_base")
    p50 = r50.encode_batch_packed(text, doc_off, ordinary=True)
    lo, hi, _, _ = r50.compact_batch_device(d_text, d_off, ordinary=True)
    torch.cuda.synchronize()
    assert hi is None and r50.id_bits == 16 and np.array_equal(lo.cpu().numpy().astype(np.int32), p50.tokens)


# ---- custom encodings with wide special ids ---------------------------------------------------------------------------------

@pytest.mark.parametrize("top_id,hb", [((1 << 17) + 5, 2), ((1 << 20) + 7, 8), ((1 << 24) + 9, 16)])
def test_custom_encoding_with_wide_special_ids(jt, top_id, hb):
    ranks = {bytes([i]): i for i in range(256)}
    ranks.update({b"ab": 256, b"abc": 257, b" t": 258, b"he": 259})
    specials = {"<|wide|>": top_id, "<|low|>": 300, "<|mid|>": 70000}
    enc = jt.new_custom_encoding("wide%d" % hb, jt._native.JTK_PATTERN_CL100K, ranks, specials)
    assert enc.id_bits == 16 + hb
    docs = ["abc <|wide|> the<|low|>", "<|wide|>" * 77, "", "no specials here abcab", "<|mid|>x<|wide|>y<|low|>" * 40, "<|wide|>"]
    text, doc_off = _pack(docs * 30)
    b = enc.new_batch()
    b.set_allowed_special("all")
    for cb in (64 << 10, 32 << 20):
        b.set_option(jt._native.JTK_OPT_HOST_CHUNK_BYTES, cb)
        p_tok, p_off, p_st = _plain_then_compact(jt, b, text, doc_off, hb, ordinary=False, allow_special=True)
        assert (p_st == 0).all() and p_tok.max() == top_id and (p_tok == top_id).sum() == 30 * (1 + 77 + 40 + 1)
        for d in (0, 1, 4, 5):                               # the wide id decodes to its literal
            assert enc.decode_bytes(p_tok[p_off[d]:p_off[d + 1]].tolist()) == docs[d].encode("utf-8")
        assert enc.decode_batch([p_tok[p_off[d]:p_off[d + 1]].tolist() for d in range(6)]) == [x.encode("utf-8") for x in docs]
        _check_post_pass(b, hb)
    big, big_off = _pack(docs * 3000)                        # several host chunks
    assert len(big) > 1 << 20
    b.set_option(jt._native.JTK_OPT_HOST_CHUNK_BYTES, 64 << 10)
    _plain_then_compact(jt, b, big, big_off, hb, ordinary=False, allow_special=True)
    _check_post_pass(b, hb)
    r = enc.encode_batch_packed(text, doc_off, allowed_special="all", compact=True)
    assert np.array_equal(r.widen(), p_tok) and r.id_bits == 16 + hb
    b.close()
    enc.close()


# ---- argument errors ----------------------------------------------------------------------------------------------------

def test_argument_errors(jt):
    import torch
    N = jt._native
    L = N.lib()
    enc = jt.get_encoding("cl100k_base")
    b = enc.new_batch()
    text, doc_off = _pack(["hello world", "x"])
    nt = C.c_int64(0)
    # the flag without JTK_ENCODE_TO_HOST
    for flags in (N.JTK_ENCODE_COMPACT_IDS, N.JTK_ENCODE_COMPACT_IDS | N.JTK_ENCODE_ORDINARY):
        assert L.jtk_batch_encode(b._h, text.ctypes.data, doc_off.ctypes.data, 2, flags, C.byref(nt)) == N.JTK_ERR_INVALID_ARGUMENT
    pb, pe = np.array([0], dtype=np.int64), np.array([5], dtype=np.int64)
    assert L.jtk_batch_encode_pieces(b._h, text.ctypes.data, doc_off.ctypes.data, 2, pb.ctypes.data, pe.ctypes.data, 1,
                                     N.JTK_ENCODE_COMPACT_IDS, C.byref(nt)) == N.JTK_ERR_INVALID_ARGUMENT
    with pytest.raises(jt.EncodingError):
        b.encode_host(text, doc_off, compact=True)
    # the flag on device input, with and without JTK_ENCODE_TO_HOST
    d_text = torch.zeros(64, dtype=torch.uint8, device="cuda")
    d_off = torch.from_numpy(doc_off).cuda()
    for flags in (N.JTK_ENCODE_COMPACT_IDS, N.JTK_ENCODE_COMPACT_IDS | N.JTK_ENCODE_TO_HOST):
        assert L.jtk_batch_encode_device(b._h, d_text.data_ptr(), d_off.data_ptr(), 2, len(text), flags, None,
                                         C.byref(nt)) == N.JTK_ERR_INVALID_ARGUMENT
    # the single-document entry point keeps the plain path
    out = np.zeros(16, dtype=np.int32)
    assert L.jtk_encode(b._h, text.ctypes.data, 5, N.JTK_ENCODE_COMPACT_IDS, -1, out.ctypes.data, 16, C.byref(nt), None) == N.JTK_ERR_INVALID_ARGUMENT
    # no result yet: neither accessor nor post-pass
    b2 = enc.new_batch()
    lo_t = torch.zeros(64, dtype=torch.int16, device="cuda")
    hi_t = torch.zeros(64, dtype=torch.int32, device="cuda")
    assert L.jtk_batch_compact(b2._h, lo_t.data_ptr(), hi_t.data_ptr(), None) == N.JTK_ERR_INVALID_ARGUMENT
    with pytest.raises(jt.EncodingError):
        b2.host_result_compact()
    b2.close()
    # host_result() after a compact encode names the other accessor; host_result_compact() after a plain one fails
    b.encode_host(text, doc_off, to_host=True, compact=True)
    with pytest.raises(jt.EncodingError) as e:
        b.host_result()
    assert e.value.code == N.JTK_ERR_INVALID_ARGUMENT and "jtk_batch_host_result_compact" in str(e.value)
    b.encode_host(text, doc_off, to_host=True)
    with pytest.raises(jt.EncodingError):
        b.host_result_compact()
    b.host_result()
    # compact() after count_only; NULL planes with tokens to write; misaligned planes
    b.encode_host(text, doc_off, count_only=True)
    with pytest.raises(jt.EncodingError) as e:
        b.compact(lo_t.data_ptr(), hi_t.data_ptr())
    assert e.value.code == N.JTK_ERR_INVALID_ARGUMENT
    b.encode_host(text, doc_off)
    assert L.jtk_batch_compact(b._h, None, hi_t.data_ptr(), None) == N.JTK_ERR_INVALID_ARGUMENT
    assert L.jtk_batch_compact(b._h, lo_t.data_ptr(), None, None) == N.JTK_ERR_INVALID_ARGUMENT
    assert L.jtk_batch_compact(b._h, lo_t.data_ptr() + 1, hi_t.data_ptr(), None) == N.JTK_ERR_INVALID_ARGUMENT
    # a count-only compact encode: offsets and status, no planes
    b.encode_host(text, doc_off, to_host=True, compact=True, count_only=True)
    r = b.host_result_compact()
    assert len(r.lo) == 0 and r.tok_off.tolist() == [0, 2, 3]
    # widening: bad id_bits, bad ranges
    lo = np.zeros(4, dtype=np.uint16)
    hi = np.zeros(1, dtype=np.uint32)
    for bits in (0, 15, 19, 33):
        assert L.jtk_widen_ids(lo.ctypes.data, hi.ctypes.data, bits, 0, 4, out.ctypes.data) == N.JTK_ERR_INVALID_ARGUMENT
    assert L.jtk_widen_ids(lo.ctypes.data, None, 17, 0, 4, out.ctypes.data) == N.JTK_ERR_INVALID_ARGUMENT
    assert L.jtk_widen_ids(lo.ctypes.data, hi.ctypes.data, 17, -1, 4, out.ctypes.data) == N.JTK_ERR_INVALID_ARGUMENT
    assert L.jtk_widen_ids(lo.ctypes.data, None, 16, 0, 4, out.ctypes.data) == N.JTK_OK
    b.close()


def test_new_symbols_are_declared_exported_and_bound(jt):
    """The convention of test_header_symbols_are_exported, for the symbols of this feature."""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "jtokkit_amd.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(jtk_[a-z_0-9]+)\s*\(", hdr))
    for name in ("jtk_encoding_id_bits", "jtk_batch_compact", "jtk_batch_host_result_compact", "jtk_widen_ids"):
        assert name in declared and name in jt._native.SIGNATURES and hasattr(jt._native.lib(), name)
    assert re.search(r"JTK_ENCODE_COMPACT_IDS\s*=\s*32u", hdr) and jt._native.JTK_ENCODE_COMPACT_IDS == 32
