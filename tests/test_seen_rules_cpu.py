"""CPU tier of the seen set (jtk_seen_set_*, jtk_batch_seen_mark): the rule header jtokkit_amd/csrc/jtk_seen_rules.h through the
shim tests/seen_sim against the plain restatement tests/seen_ref.py -- the key, position packing and its bounds, the capacity
rule, claim with wrap-around and the (min, +) merge.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import lines_ref as lr
import seen_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("seen_sim") / "libseen_sim.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas", "-o", out,
                           os.path.join(ROOT, "tests", "seen_sim", "seen_sim.cpp")])
    L = C.CDLL(out)
    p, i64, u64, i32, u32 = C.c_void_p, C.c_int64, C.c_uint64, C.c_int32, C.c_uint32
    for name, res, args in (("sim_sn_docs_ok", C.c_int, [u64, i64]),
                            ("sim_sn_key", u64, [u64, i32]), ("sim_sn_finish", u64, [u64, u64]), ("sim_sn_threshold", u32, [i32]),
                            ("sim_sn_breaks", C.c_int, [u32, u32]), ("sim_sn_pos", u64, [u64, i64, i64]), ("sim_sn_max_doc_units", i64, []),
                            ("sim_sn_capacity", i64, [i64, i64]), ("sim_sn_add_entries", i64, [p, i64, p, p, p, i64, p])):
        getattr(L, name).restype, getattr(L, name).argtypes = res, args
    return L


@pytest.mark.parametrize("unit", [sr.LINE, sr.PARAGRAPH, sr.DOCUMENT])
def test_key_and_threshold(sim, unit):
    for seed in (0, 1, 0xDEADBEEF, lr.M64):
        key = sim.sim_sn_key(seed, unit)
        assert key == sr.key_of(seed, unit) and key != lr.key_of(seed, min(unit, 1))
        for data in (b"a", b"the same line", bytes(range(256))):
            assert sim.sim_sn_finish(lr.horner(data), key) == lr.k_of(data, key)
    thr = unit + 1
    assert sim.sim_sn_threshold(unit) == thr
    assert [sim.sim_sn_breaks(s, thr) for s in range(4)] == [int(s == 3 or s >= thr) for s in range(4)]       # (3: no ink yet)


def test_position_packing_and_bounds(sim):
    assert sim.sim_sn_max_doc_units() == 1 << 24
    for base, d, u in ((0, 0, 0), (5, 7, 9), ((1 << 40) - 8, 7, (1 << 24) - 1), (123456789, 0, 1 << 23)):
        assert sim.sim_sn_pos(base, d, u) == sr.pos_of(base + d, u)
    assert sim.sim_sn_pos(0, 1, 0) > sim.sim_sn_pos(0, 0, (1 << 24) - 1)                      # document order, then text order
    for base, nd, ok in ((0, 0, 1), (0, 1 << 40, 1), (1, 1 << 40, 0), ((1 << 40) - 1, 1, 1), ((1 << 40) - 1, 2, 0), (1 << 40, 0, 0),
                         (lr.M64, 1, 0), (0, -1, 0)):
        assert sim.sim_sn_docs_ok(base, nd) == ok, (base, nd)


def test_capacity_rule(sim):
    for c, m in ((0, 0), (0, 20), (0, 32), (0, 33), (20, 200), (220, 3000), (1000, 0), (4096, 1), (0, 1 << 20)):
        assert sim.sim_sn_capacity(c, m) == sr.capacity(c, m), (c, m)
    assert [sim.sim_sn_capacity(c, m) for c, m in ((0, 20), (20, 200), (220, 3000))] == [64, 512, 8192]


@pytest.mark.parametrize("order", [0, 1, 2])
def test_claim_wraps_and_merge_is_min_and_sum(sim, order):
    """Six keys with home slots 63, 63, 63, 62, 62 and 0 of a 64-slot table, two given twice: the walk wraps, any order of arrival."""
    low = (63, 63, 63, 62, 62, 0)
    keys = [((i + 1) << 8) | lo for i, lo in enumerate(low)] + [(1 << 8) | 63, (4 << 8) | 62]
    first = [70, 60, 50, 40, 30, 20, 7, 99]
    count = [1, 2, 3, 4, 5, 6, 10, 20]
    perm = np.random.default_rng(order).permutation(len(keys)) if order else np.arange(len(keys))
    k, f, c = (np.array(x, dtype=np.uint64)[perm] for x in (keys, first, count))
    planes = np.zeros(3 * 64, dtype=np.uint64)
    planes[128:] = sr.ABSENT                                     # key | count | first
    slots = np.zeros(len(k), dtype=np.int64)
    fresh = sim.sim_sn_add_entries(planes.ctypes.data, 64, k.ctypes.data, f.ctypes.data, c.ctypes.data, len(k), slots.ctypes.data)
    ref = sr.Set()
    ref.add_entries(k, f, c)
    assert fresh == 6 == len(ref.d)
    live = np.flatnonzero(planes[:64])
    by_key = np.argsort(planes[:64][live])
    got = tuple(planes[o:o + 64][live][by_key] for o in (0, 128, 64))
    assert all(np.array_equal(g, r) for g, r in zip(got, ref.entries()))
    assert set(live) <= {62, 63, 0, 1, 2, 3, 4} and {0, 62, 63} <= set(live) and len(live) == 6          # wrapped past 63
    assert all(planes[s] == key for s, key in zip(slots, k))
