"""jtk_batch_pack / jtk_batch_pack_write / jtk_batch_pack_fetch and HipEncoding.pack_batch, pack_batch_device: the last batch
encode packed into rows of seq_len tokens -- one concatenated stream or next-fit of whole documents -- with per-cell positions
and flash-attention's varlen segments.  Every field is checked against the plain restatement of the rule (tests/pack_ref.py)
applied to the CPU oracle's tokens.  Every test here needs a real MI355X (`-m gpu`)."""
import ctypes as C
import random
import re

import numpy as np
import pytest

import golden_util
import oracle_lib
import pack_ref
import regex_crosscheck as rc
import special_ref

pytestmark = pytest.mark.gpu

EOT = "<|endoftext|>"
EOT_ID = 100257
PAD = -3
LS = (1, 7, 128, 2048)
MODES = [(-1, False, False, False), (-1, False, False, True), (-1, False, True, False),
         (EOT_ID, False, False, False), (EOT_ID, False, False, True), (EOT_ID, False, True, False),
         (EOT_ID, True, False, False), (EOT_ID, True, False, True), (EOT_ID, True, True, False)]   # (sep, sep_first, whole, drop)


@pytest.fixture(scope="module")
def jt():
    import jtokkit_amd
    return jtokkit_amd


@pytest.fixture(scope="module")
def o():
    return oracle_lib.get("cl100k_base")


def _pack(texts):
    bs = [t if isinstance(t, (bytes, bytearray)) else t.encode("utf-8") for t in texts]
    doc_off = np.zeros(len(bs) + 1, dtype=np.int64)
    np.cumsum([len(x) for x in bs], out=doc_off[1:])
    text = np.frombuffer(b"".join(bs), dtype=np.uint8) if doc_off[-1] else np.zeros(0, dtype=np.uint8)
    return bs, text, doc_off


def _oracle(o, bs, ordinary):
    """The oracle's tokens per document ([] where the device gives a negative status) and the statuses."""
    docs, status = [], []
    for x in bs:
        try:
            docs.append(o.encode_ordinary(x) if ordinary else o.encode(x))
            status.append(0)
        except oracle_lib.OracleError:
            docs.append([])
            status.append(-1)
    return docs, status


def _same(got, exp, what):
    for k in ("rows", "positions", "cu_seqlens", "seg_doc"):
        g = np.asarray(got[k])
        assert g.shape == exp[k].shape and np.array_equal(g, exp[k]), (k, what)
    assert got["max_seqlen"] == exp["max_seqlen"], what


def _fetch(b, L, sep, sep_first, whole, drop, stream=None):
    nr, ns, mx = b.pack(L, sep, whole, sep_first, drop, stream)
    f = b.pack_fetch(PAD)
    assert f["rows"].shape == (nr, L) and len(f["cu_seqlens"]) == ns + 1
    f["max_seqlen"] = mx
    return f


def _all_modes(b, docs, status, Ls=LS):
    for L in Ls:
        for sep, sf, whole, drop in MODES:
            exp = pack_ref.pack(docs, status, L, sep, sf, whole, drop, PAD)
            _same(_fetch(b, L, sep, sf, whole, drop), exp, (L, sep, sf, whole, drop))


def _fuzz_docs(rng, n=200):
    texts = [rc.random_text(rng, rng.randint(0, 80)) for _ in range(n)]
    texts += ["", "\U0001F355" * 9, "日本語のテキスト" * 5, "", "they'll 1234567 " * 30, "x <|endoftext|> y"]
    return texts


def test_golden_and_fuzz_host_input(jt, o):
    """Golden prompts and fuzz documents with encode() (a literal refuses its document) and encodeOrdinary(): every L, both
    modes, EOS / BOS / no separator, drop_last."""
    enc = jt.get_encoding("cl100k_base")
    texts = [r[0] for r in golden_util.load_rows("cl100k_base")] + _fuzz_docs(random.Random(3))
    bs, text, doc_off = _pack(texts)
    b = enc.new_batch()
    for ordinary in (True, False):
        b.encode_host(text, doc_off, ordinary)
        res = b.fetch()
        docs, status = _oracle(o, bs, ordinary)
        assert [s < 0 for s in res.status] == [s < 0 for s in status]
        assert ordinary or min(status) < 0
        _all_modes(b, docs, status)
    b.close()


def test_empty_and_refused_documents(jt, o):
    enc = jt.get_encoding("cl100k_base")
    bs, text, doc_off = _pack(["", "abc def", "x<|endoftext|>", "", "été " * 20, ""])
    b = enc.new_batch()
    b.encode_host(text, doc_off, ordinary=False)
    docs, status = _oracle(o, bs, False)
    assert b.fetch().status[2] < 0 and status[2] < 0
    _all_modes(b, docs, status, Ls=(1, 7))
    _, t2, off2 = _pack(["a<|endoftext|>", "<|endoftext|>"])           # every document refused: no rows
    b.encode_host(t2, off2)
    for whole in (False, True):
        assert b.pack(4, EOT_ID, whole) == (0, 0, 0)
        f = b.pack_fetch(PAD)
        assert f["rows"].shape == (0, 4) and f["cu_seqlens"].tolist() == [0]
    b.close()


def test_device_input_and_host_api(jt, o):
    """pack_batch_device (device-input encode, CUDA tensors) and pack_batch (host strings)."""
    import torch
    enc = jt.get_encoding("cl100k_base")
    bs, text, doc_off = _pack(_fuzz_docs(random.Random(4), 150))
    docs, status = _oracle(o, bs, True)
    d_text = torch.from_numpy(np.ascontiguousarray(text)).cuda()
    d_off = torch.from_numpy(doc_off).cuda()
    for L in (7, 128):
        for sep, sf, whole, drop in MODES:
            out = enc.pack_batch_device(d_text, d_off, L, sep=None if sep < 0 else EOT, sep_first=sf, whole_docs=whole,
                                        drop_last=drop, pad_id=PAD, ordinary=True)
            torch.cuda.synchronize()
            got = {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in out.items()}
            assert got["rows"].dtype == np.int32 and got["seg_doc"].dtype == np.int64 and isinstance(got["max_seqlen"], int)
            assert (got["status"] == 0).all()
            _same(got, pack_ref.pack(docs, status, L, sep, sf, whole, drop, PAD), (L, sep, sf, whole, drop))
    h = enc.pack_batch(bs, 128, sep=EOT_ID, whole_docs=True, pad_id=PAD, ordinary=True)
    _same(h, pack_ref.pack(docs, status, 128, EOT_ID, False, True, False, PAD), "pack_batch")


def test_to_host_and_custom_pattern_encodes(jt, o):
    """JTK_ENCODE_TO_HOST encodes and a custom-pattern (pieces) encode feed the pack as any other."""
    enc = jt.get_encoding("cl100k_base")
    bs, text, doc_off = _pack(_fuzz_docs(random.Random(5), 100))
    docs, status = _oracle(o, bs, True)
    b = enc.new_batch()
    b.encode_host(text, doc_off, ordinary=True, to_host=True)
    _all_modes(b, docs, status, Ls=(7, 128))
    b.close()
    pat = re.compile(r"\S+|\s+")
    texts = ["hello world, packed rows", "日本語 テキスト \U0001F355\U0001F355", "a b c d e f g"]
    enc._host_pattern, saved = pat, enc._host_pattern
    try:
        got = enc.pack_batch(texts, 5, sep=EOT, pad_id=PAD, ordinary=True)
    finally:
        enc._host_pattern = saved
    exp_docs = []
    for t in texts:
        spans = [(len(t[:m.start()].encode()), len(t[:m.end()].encode())) for m in pat.finditer(t)]
        exp_docs.append(o.encode_pieces(t.encode(), [s for s, _ in spans], [e for _, e in spans]))
    _same(got, pack_ref.pack(exp_docs, [0] * len(texts), 5, EOT_ID, pad_id=PAD), "pieces")


def test_allowed_special_inside_documents(jt, o):
    """<|endoftext|> inside documents encoded as its id (allowed_special), packed with the same id as separator."""
    import torch
    enc = jt.get_encoding("cl100k_base")
    texts = ["a" + EOT + "b", EOT, "plain text here", "x " + EOT + EOT + " y", ""]
    amap = {k.encode(): v for k, v in enc._specials.items()}
    docs = [special_ref.encode(o, t.encode(), amap) for t in texts]
    for L, whole in ((4, False), (4, True), (7, True)):
        got = enc.pack_batch(texts, L, sep=EOT, whole_docs=whole, pad_id=PAD, allowed_special="all")
        _same(got, pack_ref.pack(docs, [0] * len(docs), L, EOT_ID, whole=whole, pad_id=PAD), (L, whole))
        assert (got["rows"] == EOT_ID).sum() == len(texts) + 4
    _, text, doc_off = _pack(texts)
    out = enc.pack_batch_device(torch.from_numpy(text.copy()).cuda(), torch.from_numpy(doc_off).cuda(), 4, sep=EOT,
                                sep_first=True, pad_id=PAD, allowed_special="all")
    torch.cuda.synchronize()
    got = {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in out.items()}
    _same(got, pack_ref.pack(docs, [0] * len(docs), 4, EOT_ID, sep_first=True, pad_id=PAD), "device, BOS")


def test_documents_longer_than_a_row(jt, o):
    """Documents of ~55k tokens among short ones: cut into full rows in whole mode, across rows in concat mode."""
    from jtokkit_amd import corpus
    enc = jt.get_encoding("cl100k_base")
    t1, _ = corpus.english(60, mean_bytes=4096, lo=2048, hi=8192, seed=21)
    big = bytes(np.asarray(t1, dtype=np.uint8))
    bs, text, doc_off = _pack([b"short", big, b"tail doc", big[:5000], b"x"])
    docs, status = _oracle(o, bs, True)
    assert len(docs[1]) > 2 * 2048
    b = enc.new_batch()
    b.encode_host(text, doc_off, ordinary=True)
    _all_modes(b, docs, status, Ls=(128, 2048))
    b.close()


def test_200k_documents(jt, o):
    """200,000 corpus.mixed documents through pack_batch_device: the counts, cu_seqlens and seg_doc checked in full against
    the restatement on the oracle's tokens, and a seeded sample of rows and positions."""
    import torch
    from jtokkit_amd import corpus
    enc = jt.get_encoding("cl100k_base")
    text, doc_off = corpus.mixed(200000, mean_bytes=256, lo=16, hi=4096, seed=31)
    text = np.ascontiguousarray(text, dtype=np.uint8)
    doc_off = np.ascontiguousarray(doc_off, dtype=np.int64)
    tokens, tok_off = o.encode_batch(text, doc_off, threads=16)
    n = len(doc_off) - 1
    lens = np.diff(tok_off) + 1                                      # EOS units (no document is empty)
    U = tok_off[:-1] + np.arange(n)
    S = np.insert(tokens, tok_off[1:], EOT_ID).astype(np.int64)
    d_text, d_off = torch.from_numpy(text).cuda(), torch.from_numpy(doc_off).cuda()
    rng = random.Random(17)
    for L, whole in ((2048, False), (2048, True), (128, True), (8192, True)):
        out = enc.pack_batch_device(d_text, d_off, L, sep=EOT, whole_docs=whole, pad_id=PAD, ordinary=True)
        torch.cuda.synchronize()
        a = pack_ref.row_starts(lens.tolist(), L, whole)
        cu, sd, mx = pack_ref.segments(U, np.arange(n), a, L)
        assert out["rows"].shape == (len(a) - 1, L), (L, whole)
        assert np.array_equal(out["cu_seqlens"].cpu().numpy(), cu), (L, whole)
        assert np.array_equal(out["seg_doc"].cpu().numpy(), sd), (L, whole)
        assert out["max_seqlen"] == mx
        rows = out["rows"]
        pos = out["positions"]
        for r in sorted(rng.sample(range(len(a) - 1), 300)) + [len(a) - 2]:
            ids, p = pack_ref.row(S, U, a, r, L, PAD)
            assert np.array_equal(rows[r].cpu().numpy(), ids), (L, whole, r)
            assert np.array_equal(pos[r].cpu().numpy(), p), (L, whole, r)


def test_non_default_stream_ordering(jt, o):
    """The text is written on a non-default torch stream right before the call on that stream: the pack sees it."""
    import torch
    enc = jt.get_encoding("cl100k_base")
    _, text, doc_off = _pack(_fuzz_docs(random.Random(8), 100))
    ref = enc.pack_batch_device(torch.from_numpy(np.ascontiguousarray(text)).cuda(), torch.from_numpy(doc_off).cuda(), 16,
                                sep=EOT, whole_docs=True, ordinary=True, pad_id=PAD)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    host = torch.from_numpy(np.ascontiguousarray(text)).pin_memory()
    with torch.cuda.stream(s):
        d_text = torch.empty(len(text), dtype=torch.uint8, device="cuda")
        torch.cuda._sleep(20_000_000)                                    # (the copy lands late on this stream)
        d_text.copy_(host, non_blocking=True)
        d_off = torch.from_numpy(doc_off).to("cuda", non_blocking=True)
        out = enc.pack_batch_device(d_text, d_off, 16, sep=EOT, whole_docs=True, ordinary=True, pad_id=PAD)
    s.synchronize()
    for k in ref:
        if k == "max_seqlen":
            assert out[k] == ref[k]
        else:
            assert torch.equal(out[k].cpu(), ref[k].cpu()), k


def test_null_outputs_and_pack_chunk_independence(jt, o):
    """pack_write with NULL optional outputs; pack and chunk results both stay valid after the other call; a new encode
    drops the pack."""
    import torch
    N = jt._native
    enc = jt.get_encoding("cl100k_base")
    bs, text, doc_off = _pack(_fuzz_docs(random.Random(7), 60))
    docs, status = _oracle(o, bs, True)
    b = enc.new_batch()
    b.encode_host(text, doc_off, ordinary=True)
    exp = pack_ref.pack(docs, status, 16, EOT_ID, pad_id=PAD)
    nr, ns, mx = b.pack(16, EOT_ID)
    rows = torch.full((nr * 16 + 1,), 777, dtype=torch.int32, device="cuda")
    b.pack_write(PAD, rows.data_ptr())
    cu = torch.full((ns + 2,), 777, dtype=torch.int32, device="cuda")
    pos = torch.full((nr * 16 + 1,), 777, dtype=torch.int32, device="cuda")
    b.pack_write(PAD, rows.data_ptr(), None, cu.data_ptr(), None)
    b.pack_write(PAD, rows.data_ptr(), pos.data_ptr(), None, None)
    torch.cuda.synchronize()
    r, c, p = rows.cpu().numpy(), cu.cpu().numpy(), pos.cpu().numpy()
    assert r[-1] == 777 and c[-1] == 777 and p[-1] == 777
    assert np.array_equal(r[:-1].reshape(nr, 16), exp["rows"]) and np.array_equal(c[:-1], exp["cu_seqlens"])
    assert np.array_equal(p[:-1].reshape(nr, 16), exp["positions"])
    # chunk after pack, pack after chunk: both results stay
    b.chunk(8)
    chunks = b.chunk_fetch()
    f = b.pack_fetch(PAD)
    f["max_seqlen"] = mx
    _same(f, exp, "pack after chunk")
    b.pack(5, -1, whole_docs=True)
    for k, v in b.chunk_fetch().items():
        assert np.array_equal(v, chunks[k]), k
    f = b.pack_fetch(PAD)
    assert np.array_equal(f["rows"], pack_ref.pack(docs, status, 5, whole=True, pad_id=PAD)["rows"])
    # a new encode drops the pack
    b.encode_host(text, doc_off, ordinary=True)
    assert N.lib().jtk_batch_pack_write(b._h, PAD, rows.data_ptr(), None, None, None, None) == N.JTK_ERR_INVALID_ARGUMENT
    b.close()


def test_bad_arguments(jt):
    import torch
    N = jt._native
    L = N.lib()
    enc = jt.get_encoding("cl100k_base")
    b = enc.new_batch()
    nr, ns, mx = C.c_int64(0), C.c_int64(0), C.c_int32(0)
    INV = N.JTK_ERR_INVALID_ARGUMENT

    def pk(seq_len, sep=-1, flags=0):
        return L.jtk_batch_pack(b._h, seq_len, sep, flags, None, C.byref(nr), C.byref(ns), C.byref(mx))

    assert pk(4) == INV                                                     # no encode yet
    assert L.jtk_batch_pack_fetch(b._h, PAD, None, None, None, None) == INV
    _, text, doc_off = _pack(["some text here", "more"])
    b.encode_host(text, doc_off)
    for seq_len in (0, -1, 1 << 31, 1 << 40):
        assert pk(seq_len) == INV, seq_len
    assert "2^31" in L.jtk_last_error().decode()
    assert pk((1 << 31) - 1) == N.JTK_OK and nr.value == 1                  # one row of 2^31 - 1 cells: the largest allowed
    for sep in (-2, -100, 100256, 100261, 1 << 30):                         # not a rank id nor a special id of cl100k
        assert pk(4, sep) == INV, sep
    for sep in (0, 100255, EOT_ID, 100276):
        assert pk(4, sep) == N.JTK_OK, sep
    for flags in (8, 16, N.JTK_PACK_WHOLE_DOCS | N.JTK_PACK_DROP_LAST, 7):
        assert pk(4, -1, flags) == INV, flags
    assert pk(4) == N.JTK_OK
    assert L.jtk_batch_pack_write(b._h, PAD, None, None, None, None, None) == INV   # rows are not optional
    b.encode_host(text, doc_off, count_only=True)
    assert pk(4) == INV
    d_text = torch.from_numpy(np.ascontiguousarray(text)).cuda()
    d_off = torch.from_numpy(doc_off).cuda()
    rows = torch.empty((2, 4), dtype=torch.int32, device="cuda")
    aux = [torch.empty(2, dtype=dt, device="cuda") for dt in (torch.int64, torch.bool, torch.int32)]
    b.encode_device_max_tokens(d_text.data_ptr(), d_off.data_ptr(), 2, len(text), 4, rows.data_ptr(), aux[0].data_ptr(),
                               aux[1].data_ptr(), aux[2].data_ptr())
    assert pk(4) == INV
    with pytest.raises(ValueError):
        enc.pack_batch_device(d_text, d_off, 4, whole_docs=True, drop_last=True)
    with pytest.raises(ValueError):
        enc.pack_batch_device(d_text, d_off, 4, sep="<|not a token|>")
    with pytest.raises(jt.EncodingError):
        enc.pack_batch(["abc"], 4, sep=100256)
    b.close()
