"""CPU tier: the host-compilable primitives of jtokkit_amd/csrc/jtk_device_prims.h, run through the shim tests/prims_sim.
The two searches against numpy.searchsorted (side='right' for "first a[k] > x", side='left' for "first a[k] >= x") on arrays
with runs of equal values -- empty documents -- at the front, in the middle and at the end, n = 0, 1, 2, and x below the first
entry, equal to entries, and at or above the last; the token length at the table's edges with both unknown-length arguments;
the document lookups of the kernels, written in the shim exactly as the kernels call the shared search, against brute-force
loops, out-of-range x included; and mutants of the searches and of two lookups, each of which these same cases must reject."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT32_MAX = 2 ** 31 - 1

# non-decreasing arrays; equal neighbours are empty documents
ARRAYS = [
    [],
    [0],
    [5],
    [0, 0],
    [0, 3],
    [3, 3],
    [0, 0, 0, 4, 9, 12],              # a run at the front
    [0, 2, 7, 7, 7, 7, 11, 15],       # ... in the middle
    [0, 1, 6, 10, 10, 10],            # ... at the end
    [0, 0, 0, 5, 5, 8, 13, 13, 13],   # ... at all three
    [4, 4, 6, 6, 6, 9, 20, 20],       # does not start at 0
    [7] * 9,                          # nothing but one run
    list(range(0, 70, 3)),            # no run, more than 16 entries
]


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("prims_sim") / "libprims_sim.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-o", out,
                           os.path.join(ROOT, "tests", "prims_sim", "prims_sim.cpp")])
    L = C.CDLL(out)
    i64, p = C.c_int64, C.c_void_p
    for name, args in (("sim_first_gt", [p, i64, i64, i64]), ("sim_first_ge", [p, i64, i64, i64]),
                       ("sim_first_gt_mutant", [C.c_int, p, i64, i64, i64]), ("sim_first_ge_mutant", [C.c_int, p, i64, i64, i64]),
                       ("sim_find_doc", [p, i64, i64, i64]), ("sim_sp_find_doc", [p, i64, i64]), ("sim_sp_find_doc_mutant", [p, i64, i64]),
                       ("sim_mt_doc_of", [p, i64, i64, i64]), ("sim_ck_doc_of", [p, i64, i64]), ("sim_lb_doc_of", [p, i64, i64]),
                       ("sim_ck_doc_of_mutant", [p, i64, i64])):
        getattr(L, name).restype = i64
        getattr(L, name).argtypes = args
    L.sim_tok_len.restype = C.c_uint32
    L.sim_tok_len.argtypes = [p, C.c_uint32, C.c_int32, C.c_uint32]
    L.sim_blocks_for.restype = C.c_uint32
    L.sim_blocks_for.argtypes = [i64, C.c_int]
    return L


def _xs(a):
    """Below the first entry, every entry and its two neighbours, at and above the last."""
    if not a:
        return [-1, 0, 1]
    return sorted({v + d for v in a for d in (-1, 0, 1)} | {a[0] - 5, a[-1] + 5})


def _buf(a):
    # one guard entry on each side that no search may read as part of its range: chosen to derail it if it does
    return np.array([10 ** 9] + list(a) + [-10 ** 9], dtype=np.int64)


def _search_cases():
    for a in ARRAYS:
        buf = _buf(a)
        base = buf.ctypes.data + 8
        for lo, hi in {(0, len(a)), (min(1, len(a)), len(a)), (0, max(len(a) - 1, 0))}:
            for x in _xs(a):
                yield a, buf, base, lo, hi, x


def _failures(fn_gt, fn_ge):
    bad_gt = bad_ge = 0
    for a, buf, base, lo, hi, x in _search_cases():
        sub = np.asarray(a[lo:hi], dtype=np.int64)
        bad_gt += fn_gt(base, lo, hi, x) != lo + int(np.searchsorted(sub, x, side="right"))
        bad_ge += fn_ge(base, lo, hi, x) != lo + int(np.searchsorted(sub, x, side="left"))
    return bad_gt, bad_ge


def test_searches_match_searchsorted(sim):
    assert _failures(sim.sim_first_gt, sim.sim_first_ge) == (0, 0)


@pytest.mark.parametrize("kind", [0, 1, 2, 3])
def test_first_gt_mutants_are_caught(sim, kind):
    bad, _ = _failures(lambda *a: sim.sim_first_gt_mutant(kind, *a), sim.sim_first_ge)
    assert bad > 0


@pytest.mark.parametrize("kind", [0, 1])
def test_first_ge_mutants_are_caught(sim, kind):
    _, bad = _failures(sim.sim_first_gt, lambda *a: sim.sim_first_ge_mutant(kind, *a))
    assert bad > 0


def test_token_length_at_the_table_edges(sim):
    lens = [3, 1, 0, 7, 2]                                    # (an absent id inside the table: empty)
    tab = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    n = len(lens)
    for unknown in (0, 1):
        got = [sim.sim_tok_len(tab.ctypes.data, n, i, unknown) for i in (-1, 0, n - 1, n, INT32_MAX)]
        assert got == [unknown, lens[0], lens[n - 1], unknown, unknown]
        assert sim.sim_tok_len(tab.ctypes.data, n, -INT32_MAX - 1, unknown) == unknown
        assert [sim.sim_tok_len(tab.ctypes.data, n, i, unknown) for i in range(n)] == lens
        assert sim.sim_tok_len(tab.ctypes.data, 0, 0, unknown) == unknown      # an empty table


def test_blocks_for_is_at_least_one(sim):
    assert [sim.sim_blocks_for(n, 256) for n in (0, 1, 255, 256, 257, 2 ** 33)] == [1, 1, 1, 1, 2, 2 ** 25]
    assert sim.sim_blocks_for(0, 1024) == 1 and sim.sim_blocks_for(-3, 256) == 1


# ---- the kernels' document lookups: offsets arrays off[0 .. n_docs] (the ARRAYS with at least one entry), brute force beside
def _last_le(off, upto, x):
    """The last k in [0, upto) with off[k] <= x, -1 without one (a plain loop)."""
    r = -1
    for k in range(upto):
        if off[k] <= x:
            r = k
    return r


def _offset_cases():
    for a in ARRAYS:
        if a:
            buf = _buf(a)
            yield a, len(a) - 1, buf, buf.ctypes.data + 8


def test_find_doc_matches_brute_force(sim):
    for off, n_docs, buf, base in _offset_cases():
        for text_base in (0, off[len(off) // 2]):
            for x in _xs(off):
                assert sim.sim_find_doc(base, n_docs, text_base, x - text_base) == _last_le(off, n_docs, x)


def test_sp_find_doc_matches_brute_force(sim):
    caught = 0
    for off, n_docs, buf, base in _offset_cases():
        if n_docs == 0:
            continue                                          # (the find pass does not run without documents)
        for x in _xs(off):
            exp = min(max(_last_le(off, n_docs + 1, x), 0), n_docs - 1)
            assert 0 <= exp < n_docs and sim.sim_sp_find_doc(base, n_docs, x) == exp
            caught += sim.sim_sp_find_doc_mutant(base, n_docs, x) != exp
    assert caught > 0


def test_mt_doc_of_matches_brute_force(sim):
    for off, n_docs, buf, base in _offset_cases():
        for x in _xs(off):
            for ln in (0, 1, 3):
                d = _last_le(off, n_docs, x)
                exp = d if d >= 0 and x + ln <= off[d + 1] else -1
                assert sim.sim_mt_doc_of(base, n_docs, x, ln) == exp


def test_token_doc_lookups_match_brute_force(sim):
    caught = 0
    for off, n_docs, buf, base in _offset_cases():
        for x in _xs(off):
            exp = max(_last_le(off, n_docs, x), 0)            # (a valid index whatever t is; n_docs == 0 gives 0 as well)
            assert sim.sim_ck_doc_of(base, n_docs, x) == exp
            assert sim.sim_lb_doc_of(base, n_docs, x) == exp
            if off[0] <= x < off[-1]:                         # a token of the batch: its document is not empty
                assert off[exp] <= x < off[exp + 1]
            caught += sim.sim_ck_doc_of_mutant(base, n_docs, x) != exp
    assert caught > 0
