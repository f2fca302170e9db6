"""Batch decode on the device (jtk_decode.hip: k_dec_mark, k_dec_count, k_dec_scan, k_dec_scatter, k_dec_offsets) against the
plain reference tests/decode_ref.py, on the inputs of tests/decode_cases.py that are built for the kernels' own edges: tiles on
both sides of the LDS stage limit, every word alignment of a tile's bytes, sequence starts and runs of empty sequences on tile,
mask-word and lane edges, ids without an entry in every position.  n_bytes, every output byte, every byte_off entry and every
status entry are compared exactly, through every entry point.  tests/test_decode_ref_cpu.py shows the reference equal to the
CPU oracle on the same inputs.  Every test here needs a real MI355X (`-m gpu`)."""
import ctypes as C

import numpy as np
import pytest

import decode_cases as dc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def jt():
    import jtokkit_amd
    return jtokkit_amd


@pytest.fixture(scope="module")
def encs(jt):
    kind, ranks, specials = dc.custom_spec()
    custom = jt.new_custom_encoding("decode_custom", kind, ranks, specials)
    yield {name: custom if name == "custom" else jt.get_encoding(name) for name in dc.TABLES}
    custom.close()


def _same(what, got, exp):
    """got = (n_bytes, out uint8[], byte_off, status) of the device; exp = decode_ref's (bytes, byte_off, status)."""
    nb, out, byte_off, status = got
    e_out, e_off, e_status = exp
    assert nb == len(e_out), what
    assert np.array_equal(status, e_status), (what, "status", np.flatnonzero(status != e_status)[:5])
    assert np.array_equal(byte_off, e_off), (what, "byte_off", np.flatnonzero(byte_off != e_off)[:5])
    e = np.frombuffer(e_out, dtype=np.uint8)
    assert len(out) == len(e), what
    assert np.array_equal(out, e), (what, "first wrong byte", int(np.flatnonzero(out != e)[0]))


def _host(b, ids, seq_off):
    nb = b.decode_host(ids, seq_off)
    return (nb,) + b.decode_fetch()


class _Dev:
    def __init__(self, ptr, n, typestr):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": typestr, "data": (ptr, False), "version": 2}


def _device_result(b, nb, n_seqs):
    """jtk_batch_decode_device_result of the last decode, read back through torch."""
    import torch
    from jtokkit_amd import _native as N
    p = [C.c_void_p() for _ in range(3)]
    assert N.lib().jtk_batch_decode_device_result(b._h, *(C.byref(x) for x in p)) == N.JTK_OK
    view = lambda ptr, n, ts, dt: torch.as_tensor(_Dev(ptr.value, n, ts), device="cuda").cpu().numpy() if n else np.zeros(0, dtype=dt)
    return nb, view(p[0], nb, "|u1", np.uint8), view(p[1], n_seqs + 1, "<i8", np.int64), view(p[2], n_seqs, "<i4", np.int32)


@pytest.mark.parametrize("name", dc.TABLES)
def test_host_entry_every_case(encs, name):
    """Batch.decode_host + decode_fetch == the reference, case after case on one batch."""
    b = encs[name].new_batch()
    exp = dc.expected(name)
    for cname, ids, seq_off in dc.cases(name):
        _same(cname, _host(b, ids, seq_off), exp[cname])
    b.close()


@pytest.mark.parametrize("mode", ["batch_stream", "side_stream", "ids_4_byte_aligned"])
@pytest.mark.parametrize("name", dc.TABLES)
def test_device_entry_every_case(encs, name, mode):
    """Batch.decode_device on torch tensors: on the batch's stream, on a non-default torch stream, and with d_ids at an
    address that is a multiple of 4 but not of 16; decode_fetch and jtk_batch_decode_device_result both give the reference."""
    import torch
    b = encs[name].new_batch()
    exp = dc.expected(name)
    side = torch.cuda.Stream()
    for cname, ids, seq_off in dc.cases(name):
        n, ns = len(ids), len(seq_off) - 1
        d_off = torch.from_numpy(np.array(seq_off)).cuda()
        if mode == "ids_4_byte_aligned":
            buf = torch.zeros(n + 1, dtype=torch.int32, device="cuda")
            buf[1:] = torch.from_numpy(np.array(ids))
            d_ids = buf[1:]
            assert n == 0 or d_ids.data_ptr() % 16 == 4
        else:
            d_ids = torch.from_numpy(np.array(ids)).cuda()
        torch.cuda.synchronize()                                           # (the library's streams do not wait for torch's)
        nb = b.decode_device(d_ids.data_ptr() if n else None, d_off.data_ptr(), ns, n,
                             stream=side.cuda_stream if mode == "side_stream" else None)
        _same((cname, "fetch"), (nb,) + b.decode_fetch(), exp[cname])
        _same((cname, "device_result"), _device_result(b, nb, ns), exp[cname])
    b.close()


def test_device_entry_without_sequences(encs):
    """n_seqs = 0 through the device entry, before and after a decode that left sequences behind: no bytes, byte_off = [0]."""
    import torch
    b = encs["cl100k_base"].new_batch()
    d_off = torch.zeros(1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    for _ in range(2):
        assert b.decode_device(None, d_off.data_ptr(), 0, 0) == 0
        out, byte_off, status = b.decode_fetch()
        assert len(out) == 0 and byte_off.tolist() == [0] and len(status) == 0
        assert _device_result(b, 0, 0)[2].tolist() == [0]
        cname, ids, seq_off = dc.cases("cl100k_base")[-1]
        _same(cname, _host(b, ids, seq_off), dc.expected("cl100k_base")[cname])
    b.close()


@pytest.mark.parametrize("name", dc.TABLES)
def test_per_call_decode_on_fuzz_sequences(encs, name):
    """enc.decode_bytes (jtk_decode) of every sequence of the fuzz cases: the reference's bytes, or an error where the
    reference's status is JTK_ERR_UNKNOWN_TOKEN."""
    enc = encs[name]
    exp = dc.expected(name)
    n_ok = n_bad = 0
    for cname, ids, seq_off in dc.cases(name):
        if not dc.is_fuzz(cname):
            continue
        out, byte_off, status = exp[cname]
        for q in range(len(status)):
            toks = ids[seq_off[q]:seq_off[q + 1]]
            if status[q] == 0:
                assert enc.decode_bytes(toks) == out[byte_off[q]:byte_off[q + 1]], (cname, q)
                n_ok += 1
            else:
                with pytest.raises(ValueError):
                    enc.decode_bytes(toks)
                n_bad += 1
    assert n_ok > 100 and n_bad > 10


@pytest.mark.parametrize("name", dc.TABLES)
def test_decode_batch_strict_and_lenient(jt, encs, name):
    """decode_batch(strict=True) raises and names the first list with an id that has no entry; strict=False returns the
    reference's bytes for every list."""
    enc = encs[name]
    exp = dc.expected(name)
    n_raised = n_clean = 0
    for cname, ids, seq_off in dc.cases(name):
        if not (dc.is_fuzz(cname) or cname in ("id_classes", "count_65_short_seqs", "no_ids_300_seqs")):
            continue
        out, byte_off, status = exp[cname]
        lists = [ids[seq_off[q]:seq_off[q + 1]].tolist() for q in range(len(status))]
        want = [out[byte_off[q]:byte_off[q + 1]] for q in range(len(status))]
        assert enc.decode_batch(lists, strict=False) == want, cname
        if (status != 0).any():
            with pytest.raises(jt.EncodingError) as ei:
                enc.decode_batch(lists)
            assert ei.value.code == -3 and "(list %d)" % int(np.flatnonzero(status != 0)[0]) in str(ei.value), cname
            n_raised += 1
        else:
            assert enc.decode_batch(lists) == want, cname
            n_clean += 1
    assert n_raised >= 5 and n_clean >= 2


def _by_name(name):
    return {c[0]: c for c in dc.cases(name)}


@pytest.mark.parametrize("name", ["cl100k_base", "custom"])
def test_batch_reused_for_shorter_decodes(encs, name):
    """The largest case, one token, no ids, the largest again on one batch: the scratch the longer call left (sequence-start
    offsets, mask, status) does not enter the shorter one."""
    cs, exp = _by_name(name), dc.expected(name)
    big = max(dc.cases(name), key=lambda c: (len(c[1]), len(c[2])))[0]
    b = encs[name].new_batch()
    for cname in (big, "count_1_one_seq", "no_ids_1_seq", big, "no_ids_300_seqs", "one_seq_per_token", "count_1_one_seq"):
        _same(cname, _host(b, cs[cname][1], cs[cname][2]), exp[cname])
    b.close()


def test_encode_then_decode_on_one_batch(encs):
    """A decode on the batch of an encode leaves the encode's result as it was."""
    from jtokkit_amd import corpus
    text, doc_off = corpus.english(50)
    cs, exp = _by_name("cl100k_base"), dc.expected("cl100k_base")
    b = encs["cl100k_base"].new_batch()
    b.encode_host(text, doc_off, ordinary=True)
    r1 = b.fetch()
    t1, o1, s1 = r1.tokens.copy(), r1.tok_off.copy(), r1.status.copy()
    for cname in ("stage_%d_between_staged" % (dc.S + 1), "fuzz_3"):
        _same(cname, _host(b, cs[cname][1], cs[cname][2]), exp[cname])
    r2 = b.fetch()
    assert np.array_equal(r2.tokens, t1) and np.array_equal(r2.tok_off, o1) and np.array_equal(r2.status, s1)
    nb = b.decode_host(t1, o1)
    out, byte_off, status = b.decode_fetch()
    assert nb == len(text) and np.array_equal(out, text) and np.array_equal(byte_off, doc_off) and (status == 0).all()
    b.close()


def test_argument_checks_of_the_host_entry(encs):
    """Malformed offsets and a missing id array are refused by jtk_batch_decode (the device entry trusts its offsets and gets
    none of these), decode_fetch needs a decode and a large enough buffer; the next valid decode is right after each."""
    from jtokkit_amd import _native as N
    L = N.lib()
    cs, exp = _by_name("cl100k_base"), dc.expected("cl100k_base")
    cname, ids, seq_off = cs["fuzz_1"]
    b = encs["cl100k_base"].new_batch()
    nb = C.c_int64(-7)
    out = np.zeros(16, dtype=np.uint8)
    assert L.jtk_batch_decode_fetch(b._h, out.ctypes.data, 16, None, None) == N.JTK_ERR_INVALID_ARGUMENT       # no decode yet
    _same(cname, _host(b, ids, seq_off), exp[cname])

    def refused(ids_ptr, off):
        off = np.array(off, dtype=np.int64)
        assert L.jtk_batch_decode(b._h, ids_ptr, off.ctypes.data, len(off) - 1, C.byref(nb)) == N.JTK_ERR_INVALID_ARGUMENT
        assert nb.value == -7
        _same(cname, _host(b, ids, seq_off), exp[cname])

    some = np.array(ids[:8])
    refused(some.ctypes.data, [1, 4, 8])                                   # seq_off[0] != 0
    refused(some.ctypes.data, [0, 5, 4, 8])                                # decreasing
    refused(None, [0, 3, 8])                                               # ids = NULL with n_ids > 0
    total = b.decode_host(ids, seq_off)
    assert total == len(exp[cname][0]) > 1
    small = np.full(total, 0xEE, dtype=np.uint8)
    assert L.jtk_batch_decode_fetch(b._h, small.ctypes.data, total - 1, None, None) == N.JTK_ERR_CAPACITY
    assert (small == 0xEE).all()
    assert L.jtk_batch_decode_fetch(b._h, small.ctypes.data, total, None, None) == N.JTK_OK
    assert small.tobytes() == exp[cname][0]
    _same(cname, _host(b, ids, seq_off), exp[cname])
    b.close()
