"""jtk_batch_encode_device_max_tokens on the batches of tests/maxtok_cases.py -- whose reach of the kernels' edges (gather
alignments, mask-word, scan-step and lane edges of k_mt_decide, its wave sums, the plan blocks of later rounds, k_mt_special's
blocks and workgroups) and whose power to tell wrong rules from the right one the CPU tier (tests/test_maxtok_cases_cpu.py)
asserts.  For every batch, through HipEncoding.encode_batch_max_tokens_device: every document's (row[:kept], kept, truncated,
status) equals the CPU oracle on the WHOLE document, or the special-token reference (status -2, kept 0, not truncated); every
cell past kept is the pad; and every field equals the host call jtk_batch_encode_max_tokens on the same bytes.  No document is
skipped: the CPU tier asserts that the oracle refuses none but the special references.  Every test here needs a real MI355X
(`-m gpu`)."""
import numpy as np
import pytest

import maxtok_cases as mc
import maxtok_ref as ref
import merge_ref

pytestmark = pytest.mark.gpu

PAD = -7
CASES = {c.name: c for c in mc.cases()}
_expected = {}


@pytest.fixture(scope="module")
def jt():
    import jtokkit_amd
    import torch
    torch.zeros(1, device="cuda:0")
    torch.cuda.synchronize()
    for name in sorted({c.enc for c in CASES.values()} - {mc.CUSTOM["name"]}):   # (the runtime starts and the tables go down here, not in a test)
        jtokkit_amd.get_encoding(name)
    return jtokkit_amd


@pytest.fixture(scope="module")
def custom(jt):
    enc = jt.new_custom_encoding(mc.CUSTOM["name"], mc.CUSTOM["kind"], merge_ref.load_ranks(mc.CUSTOM["file"].split(".")[0]),
                                 mc.CUSTOM["specials"])
    yield enc
    enc.close()


def _expect(c, ordinary):
    """The oracle's answer for every document, once per module: (rows [n, mx] padded, kept, truncated, status)."""
    if (c.name, ordinary) not in _expected:
        exp = ref.expected(mc.oracle(c.enc), c.docs, c.max_tokens, ordinary, mc.literals(c.enc))
        rows = np.full((len(c.docs), c.max_tokens), PAD, dtype=np.int32)
        for d, (ids, kept, _, _) in enumerate(exp):
            assert kept == len(ids) <= c.max_tokens
            rows[d, :kept] = ids
        _expected[(c.name, ordinary)] = (rows, np.array([e[1] for e in exp], dtype=np.int64), np.array([e[2] for e in exp], dtype=bool),
                                         np.array([e[3] for e in exp], dtype=np.int32))
    return _expected[(c.name, ordinary)]


def _pack(docs):
    doc_off = np.zeros(len(docs) + 1, dtype=np.int64)
    np.cumsum([len(d) for d in docs], out=doc_off[1:])
    return np.frombuffer(b"".join(docs), dtype=np.uint8), doc_off


def _device(enc, text, doc_off, mx, ordinary, offset):
    """The call on a text that lies `offset` bytes into a larger tensor -> numpy (rows, kept, truncated, status)."""
    import torch
    dev = torch.device("cuda:0")
    big = torch.zeros(len(text) + 80, dtype=torch.uint8, device=dev)
    big[offset:offset + len(text)] = torch.from_numpy(text.copy()).to(dev)
    d_text = big[offset:offset + len(text)]
    assert d_text.data_ptr() % 16 == offset
    d_off = torch.from_numpy(doc_off).to(dev)
    rows, kept, tr, st = enc.encode_batch_max_tokens_device(d_text, d_off, mx, ordinary=ordinary, pad_id=PAD)
    torch.cuda.synchronize()
    return rows.cpu().numpy(), kept.cpu().numpy(), tr.cpu().numpy().astype(bool), st.cpu().numpy()


def _same(what, got, exp, docs):
    bad = np.flatnonzero((got != exp).reshape(len(docs), -1).any(axis=1)) if len(docs) else []
    assert len(bad) == 0, (what, [(int(d), docs[d][:48], got[d].tolist(), exp[d].tolist()) for d in bad[:4]])


def _run(jt, enc, host_enc, c):
    text, doc_off = _pack(c.docs)
    for ordinary in c.modes:
        exp = _expect(c, ordinary)
        b = host_enc.new_batch()
        h_rows, h_kept, h_tr, h_st = b.encode_max_tokens(text, doc_off, c.max_tokens, ordinary)
        b.close()
        live = np.arange(c.max_tokens)[None, :] < exp[1][:, None]
        for offset in c.offsets:
            rows, kept, tr, st = _device(enc, text, doc_off, c.max_tokens, ordinary, offset)
            what = (c.name, "ordinary" if ordinary else "encode", offset)
            _same(what + ("status",), st, exp[3], c.docs)
            _same(what + ("kept",), kept, exp[1], c.docs)
            _same(what + ("truncated",), tr, exp[2], c.docs)
            _same(what + ("rows and pad",), rows, exp[0], c.docs)             # the ids, then the pad to the row's end
            # the host call, field for field (its rows carry nothing behind kept)
            assert np.array_equal(st, h_st) and np.array_equal(kept, h_kept) and np.array_equal(tr, h_tr.astype(bool)), what
            assert np.array_equal(np.where(live, rows, 0), np.where(live, h_rows, 0)), what
        if not ordinary:
            assert (exp[3] == ref.UNSUPPORTED_SPECIAL).sum() == sum(ref.special_docs(c.docs, mc.literals(c.enc))) > 0


def _plain(jt, name):
    c = CASES[name]
    assert c.chunk_bytes is None
    enc = jt.get_encoding(c.enc)
    _run(jt, enc, enc, c)


def _chunked(jt, name):
    """JTK_OPT_CHUNK_BYTES on an encoding of its own, closed afterwards; the host call runs on the shared one."""
    c = CASES[name]
    assert c.chunk_bytes == mc.MIN_CHUNK
    enc = jt.new_encoding(c.enc)
    try:
        enc._b().set_option(jt._native.JTK_OPT_CHUNK_BYTES, c.chunk_bytes)
        _run(jt, enc, jt.get_encoding(c.enc), c)
    finally:
        enc.close()


def test_gather_alignments(jt):
    """Every source alignment x destination alignment x length, at tensor offsets 0, 1, 7 and 15, under both calls."""
    _plain(jt, "gather")


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c.kind == "scan" and c.chunk_bytes is None])
def test_scan_edges_in_a_single_chunk_job(jt, name):
    _plain(jt, name)


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c.kind == "scan" and c.chunk_bytes is not None])
def test_scan_edges_in_the_second_chunk(jt, name):
    _chunked(jt, name)


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c.kind == "trap"])
def test_traps(jt, name):
    """Texts on which a scan that takes a start inside the margin, or one inside a white-space run, returns wrong tokens."""
    _plain(jt, name)


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c.kind == "sum"])
def test_token_sums(jt, name):
    """max_tokens 63..129 (and 2: the back-off down to keep == 0): the wave sums and the row write, 64 at a time."""
    _plain(jt, name)


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c.kind == "round"])
def test_plan_blocks_of_later_rounds(jt, name):
    _plain(jt, name)


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c.kind == "special"])
def test_special_literals(jt, custom, name):
    """Literals on block, workgroup, document and text edges at tensor offsets 0, 3 and 15; encodeOrdinary flags nothing."""
    c = CASES[name]
    enc = custom if c.enc == mc.CUSTOM["name"] else jt.get_encoding(c.enc)
    _run(jt, enc, enc, c)
