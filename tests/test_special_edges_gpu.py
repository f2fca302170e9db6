"""JTK_ENCODE_ALLOW_SPECIAL on the batches of tests/special_cases.py -- whose reach of the kernels' edges (k_sp_find's lanes, waves
and workgroups, its two scan bounds and its document lookup, chains across the launch blocks of k_sp_resolve / k_sp_walk, the
empty slots of k_sp_subs, k_sp_gather's workgroups, rounds and keep-j shortcut) and whose power to tell wrong batch logic from
the right one the CPU tier (tests/test_special_cases_cpu.py) asserts.  For every batch, allowed set, encode() and
encodeOrdinary(), host input and device input: every document's tokens and status and the whole tok_off equal the restatement
tests/special_ref.py, and the two inputs give identical arrays.  No document is skipped: the CPU tier asserts that the oracle
refuses no segment.  Every test here needs a real MI355X (`-m gpu`)."""
import os

import numpy as np
import pytest

import oracle_lib
import special_cases as sc

pytestmark = pytest.mark.gpu

CASES = sc.cases()
BY_NAME = sc.by_name()
_expected = {}


@pytest.fixture(scope="module")
def encs():
    """Every encoding of the case set, and the first HIP context: built here, not in a test."""
    import jtokkit_amd
    import torch
    from jtokkit_amd.encoding import HipEncoding
    torch.zeros(1, device="cuda:0")
    torch.cuda.synchronize()
    with open(os.path.join(oracle_lib.DATA_DIR, "cl100k_base.tiktoken"), "rb") as f:
        data = f.read()
    out = {sc.CL100K: jtokkit_amd.get_encoding(sc.CL100K)}
    for name, sp in sc.CUSTOM.items():
        out[name] = HipEncoding(name, 1, data, {k.decode(): v for k, v in sp.items()})
    for enc in out.values():                                       # (and every kernel once)
        enc.encode_batch([b"warm <|endoftext|> up"], ordinary=True, allowed_special="all")
    yield out
    for name in sc.CUSTOM:
        out[name].close()


def _expect(c, allowed, ordinary):
    """The restatement's answer, once per module: (tokens, tok_off, status)."""
    key = (c.name, allowed, ordinary)
    if key not in _expected:
        exp = sc.expected(c, allowed, ordinary)
        tok_off = np.zeros(len(exp) + 1, dtype=np.int64)
        np.cumsum([len(t) for _, t in exp], out=tok_off[1:])
        tokens = np.array([t for _, toks in exp for t in toks], dtype=np.int32)
        _expected[key] = (tokens, tok_off, np.array([s for s, _ in exp], dtype=np.int32))
    return _expected[key]


def _ids(c, allowed):
    return None if allowed is None else [sc.specials(c.enc)[x] for x in allowed]


def _text(c):
    text, doc_off = sc._pack(c.docs)
    return np.frombuffer(text, dtype=np.uint8), doc_off


def _device_text(raw, n, tail=b""):
    """n bytes of text in a 16-byte aligned tensor that extends to the next multiple of 16 plus 16 bytes: `tail`, then zeros."""
    import torch
    size = (n + 15) // 16 * 16 + 16
    host = np.zeros(size, dtype=np.uint8)
    host[:n] = raw[:n]
    t = np.frombuffer(tail, dtype=np.uint8)[:size - n]
    host[n:n + len(t)] = t
    d = torch.from_numpy(host).to("cuda:0")
    assert d.data_ptr() % 16 == 0 and d.numel() == size
    return d


def _same(what, res, exp, c):
    tokens, tok_off, status = exp
    assert np.array_equal(res.status, status), (what, "status", np.flatnonzero(res.status != status)[:8].tolist())
    if not np.array_equal(res.tok_off, tok_off):
        d = int(np.flatnonzero(res.tok_off != tok_off)[0]) - 1
        assert False, (what, "tok_off", d, c.docs[d][:60], res.tokens[res.tok_off[d]:res.tok_off[d + 1]].tolist()[:24], tokens[tok_off[d]:tok_off[d + 1]].tolist()[:24])
    if not np.array_equal(res.tokens, tokens):
        t = int(np.flatnonzero(res.tokens != tokens)[0])
        d = int(np.searchsorted(tok_off, t, side="right")) - 1
        assert False, (what, "tokens", t, d, c.docs[d][:60], res.tokens[t:t + 8].tolist(), tokens[t:t + 8].tolist())


def _run(encs, c, poison=False):
    """Host input and device input of every allowed set and mode against the restatement, and against each other."""
    import torch
    enc = encs[c.enc]
    text, doc_off = _text(c)
    n = len(text)
    d_text = _device_text(text, n, (c.pad + sc.EOT * 3) if poison else b"")
    d_off = torch.from_numpy(doc_off).to("cuda:0")
    b = enc.new_batch()
    try:
        for allowed in c.allowed:
            b.set_allowed_special(_ids(c, allowed))
            for ordinary in c.modes:
                exp = _expect(c, allowed, ordinary)
                what = (c.name, allowed if allowed is None else [x[:16] for x in allowed], "ordinary" if ordinary else "encode")
                b.encode_host(text, doc_off, ordinary, validate=c.validate, allow_special=True)
                host = b.fetch()
                _same(what + ("host",), host, exp, c)
                nt = b.encode_device(d_text.data_ptr(), d_off.data_ptr(), len(c.docs), n, ordinary, allow_special=True, validate=c.validate)
                dev = b.fetch()
                _same(what + ("device",), dev, exp, c)
                assert nt == len(exp[0])
                assert np.array_equal(host.tokens, dev.tokens) and np.array_equal(host.tok_off, dev.tok_off)
                assert np.array_equal(host.status, dev.status)
    finally:
        b.close()


def _group(kind):
    return [c for c in CASES if c.kind == kind]


def test_find_lane_and_wave_edges(encs):
    for c in _group("find/lane") + _group("find/wave"):
        _run(encs, c)


BLOCK_CASES = _group("find/block")


@pytest.mark.parametrize("part", range(3))
def test_find_block_edges(encs, part):
    """(the 25 batches of the group in three parts, a few seconds each)"""
    for c in BLOCK_CASES[part::3]:
        _run(encs, c)


def test_find_document_boundary_inside_a_literal(encs):
    c = BY_NAME["find_doc_boundary"]
    _run(encs, c)
    st = _expect(c, (sc.EOT,), False)[2]
    assert (st == -2).sum() == 11                                  # `<|e` whole in the first document of ten pairs, and the last but one


def test_find_batch_end_at_every_remainder(encs):
    for c in _group("find/batch-end"):
        _run(encs, c)


def test_poisoned_tail_behind_the_batch(encs):
    """Device input: the bytes behind n_bytes complete the cut literal (and go on with further literals)."""
    cut = [c for c in _group("find/batch-end") if c.pad]
    assert len(cut) == 16
    for c in cut:
        _run(encs, c, poison=True)


def test_stale_tail_of_the_last_host_text(encs):
    """Host input: the batch object has just encoded the longer text that completes the literal; then its prefix."""
    for c in _group("find/batch-end"):
        if not c.pad:
            continue
        enc = encs[c.enc]
        text, doc_off = _text(c)
        longer = np.concatenate([text, np.frombuffer(c.pad + sc.EOT, dtype=np.uint8)])
        long_off = doc_off.copy()
        long_off[-1] = len(longer)
        fresh, used = enc.new_batch(), enc.new_batch()
        try:
            for ordinary in c.modes:
                used.encode_host(longer, long_off, ordinary, allow_special=True)
                assert int((used.fetch().tokens == 100257).sum()) == 2
                used.encode_host(text, doc_off, ordinary, allow_special=True)
                got = used.fetch()
                fresh.encode_host(text, doc_off, ordinary, allow_special=True)
                ref = fresh.fetch()
                assert np.array_equal(got.tokens, ref.tokens) and np.array_equal(got.tok_off, ref.tok_off)
                assert np.array_equal(got.status, ref.status)
                _same((c.name, ordinary, "stale"), got, _expect(c, None, ordinary), c)
        finally:
            fresh.close()
            used.close()


def test_documents_empty_runs_counts_and_aligned_offsets(encs):
    for c in _group("docs/empties"):
        _run(encs, c)


def test_chains(encs):
    for c in _group("chains"):
        _run(encs, c)


def test_stitch_totals_rounds_runs_and_refusals(encs):
    for c in _group("stitch"):
        _run(encs, c)


def test_stitch_count_only(encs):
    import torch
    for c in _group("stitch"):
        enc = encs[c.enc]
        text, doc_off = _text(c)
        d_text = _device_text(text, len(text))
        d_off = torch.from_numpy(doc_off).to("cuda:0")
        b = enc.new_batch()
        try:
            for allowed in c.allowed:
                b.set_allowed_special(_ids(c, allowed))
                for ordinary in c.modes:
                    _, tok_off, status = _expect(c, allowed, ordinary)
                    b.encode_host(text, doc_off, ordinary, validate=c.validate, count_only=True, allow_special=True)
                    counts, st = b.fetch_counts()
                    assert np.array_equal(counts, np.diff(tok_off)) and np.array_equal(st, status), (c.name, allowed, ordinary)
                    b.encode_device(d_text.data_ptr(), d_off.data_ptr(), len(c.docs), len(text), ordinary, allow_special=True,
                                    validate=c.validate, count_only=True)
                    counts, st = b.fetch_counts()
                    assert np.array_equal(counts, np.diff(tok_off)) and np.array_equal(st, status), (c.name, allowed, ordinary)
        finally:
            b.close()


@pytest.mark.parametrize("name", ["chains_two_chunks", "docs_two_chunks"])
def test_smallest_chunks(encs, name):
    """JTK_OPT_CHUNK_BYTES and JTK_OPT_HOST_CHUNK_BYTES at their smallest: the pipeline runs on the sub-documents in two chunks,
    cut behind the slot of the literal that lies across the chunk edge (the CPU tier asserts where)."""
    import torch
    from jtokkit_amd import _native as N
    c = BY_NAME[name]
    enc = encs[c.enc]
    text, doc_off = _text(c)
    d_text = _device_text(text, len(text))
    d_off = torch.from_numpy(doc_off).to("cuda:0")
    b = enc.new_batch()
    try:
        b.set_option(N.JTK_OPT_CHUNK_BYTES, sc.MIN_CHUNK)
        b.set_option(N.JTK_OPT_HOST_CHUNK_BYTES, sc.MIN_CHUNK)
        for allowed in c.allowed:
            b.set_allowed_special(_ids(c, allowed))
            for ordinary in c.modes:
                exp = _expect(c, allowed, ordinary)
                b.encode_host(text, doc_off, ordinary, allow_special=True)
                _same((name, allowed, ordinary, "host, two chunks"), b.fetch(), exp, c)
                b.encode_host(text, doc_off, ordinary, to_host=True, allow_special=True)
                _same((name, allowed, ordinary, "host to host, two chunks"), b.host_result(), exp, c)
                b.encode_device(d_text.data_ptr(), d_off.data_ptr(), len(c.docs), len(text), ordinary, allow_special=True)
                _same((name, allowed, ordinary, "device, two chunks"), b.fetch(), exp, c)
    finally:
        b.close()
