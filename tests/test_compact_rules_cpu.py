"""CPU tier: the compact-ids rule (jtokkit_amd/csrc/jtk_compact_rules.h) -- a 16-bit plane plus a plane of hb high bits per
token --, run on the CPU through the shim tests/compact_sim, against the plain restatement tests/compact_ref.py: hb at every
edge of max_id and for the shipped encodings' tables and special ids, the planes of random streams at every hb and length,
compaction range by range with random cuts (as a job's chunks do it), widening of any range, and the golden prompts' token
lists.  Every comparison is exact."""
import base64
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import compact_ref
import golden_util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD16, GUARD32 = 0xFFFF, 0xFFFFFFFF          # all ones: a bit the shim fails to clear shows, wherever it is
LENGTHS = (0, 1, 31, 32, 33, 63, 64, 65, 1000, 100003)
HBS = (0, 1, 2, 4, 8, 16)


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("compact_sim") / "libcompact_sim.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-o", out,
                           os.path.join(ROOT, "tests", "compact_sim", "compact_sim.cpp")])
    L = C.CDLL(out)
    L.sim_compact_hb.restype = C.c_int
    L.sim_compact_hb.argtypes = [C.c_int64]
    L.sim_compact_valid_bits.restype = C.c_int
    L.sim_compact_valid_bits.argtypes = [C.c_int]
    L.sim_compact_hi_words.restype = C.c_int64
    L.sim_compact_hi_words.argtypes = [C.c_int64, C.c_int]
    L.sim_compact_lo_bytes.restype = C.c_int64
    L.sim_compact_lo_bytes.argtypes = [C.c_int64]
    L.sim_compact.restype = None
    L.sim_compact.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int]
    L.sim_widen.restype = None
    L.sim_widen.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int64, C.c_void_p]
    return L


def _max_id(hb):
    return min((1 << (16 + hb)) - 1, (1 << 31) - 1)


def _stream(rng, n, hb):
    """n random ids below 2^(16 + hb), with 0 and the largest id among them when there is room."""
    ids = rng.integers(0, _max_id(hb) + 1, size=n, dtype=np.int64)
    if n >= 1:
        ids[rng.integers(0, n)] = _max_id(hb)
    if n >= 2:
        ids[(int(np.argmax(ids)) + 1) % n] = 0
    if n >= 40:
        ids[31], ids[32] = _max_id(hb), _max_id(hb)          # both sides of a word boundary
    return ids.astype(np.int32)


def _sim_compact(sim, ids, hb, cuts=None):
    """Planes from the shim, each with a guard entry behind it that must stay untouched; pre-filled with ones so that bits
    the shim fails to clear show."""
    n = len(ids)
    cuts = np.asarray([0, n] if cuts is None else cuts, dtype=np.int64)
    nw = int(sim.sim_compact_hi_words(n, hb))
    assert nw == compact_ref.hi_words(n, hb) and sim.sim_compact_lo_bytes(n) == 2 * n
    src = np.concatenate([np.asarray(ids, dtype=np.int32), np.array([0x7FFFFFFF], dtype=np.int32)])   # never read: would set bits
    lo = np.full(n + 1, GUARD16, dtype=np.uint16)
    hi = np.full(nw + 1, GUARD32, dtype=np.uint32)
    sim.sim_compact(src.ctypes.data, cuts.ctypes.data, len(cuts), lo.ctypes.data, hi.ctypes.data, hb)
    assert lo[n] == GUARD16 and hi[nw] == GUARD32
    return lo[:n], (hi[:nw] if hb else None)


def _same(a, b):
    lo_a, hi_a = a
    lo_b, hi_b = b
    assert lo_a.dtype == lo_b.dtype == np.uint16 and np.array_equal(lo_a, lo_b)
    assert (hi_a is None) == (hi_b is None)
    if hi_a is not None:
        assert hi_a.dtype == hi_b.dtype == np.uint32 and np.array_equal(hi_a, hi_b)


def test_high_bits_at_every_edge(sim):
    want = {0: 0, 65535: 0, 65536: 1, 2 ** 17 - 2: 1, 2 ** 17 - 1: 1, 2 ** 17: 2, 2 ** 18 - 1: 2, 2 ** 18: 4, 2 ** 20 - 1: 4, 2 ** 20: 8,
            2 ** 24 - 1: 8, 2 ** 24: 16, 2 ** 31 - 1: 16}
    for max_id, hb in want.items():
        assert sim.sim_compact_hb(max_id) == hb == compact_ref.hb_for(max_id), max_id
    for bits in range(0, 40):
        assert bool(sim.sim_compact_valid_bits(bits)) == (bits in (16, 17, 18, 20, 24, 32))


def test_high_bits_of_the_shipped_encodings(sim):
    """From the real rank files and the registry's special ids: 16, 16, 16 and 17 bits."""
    from jtokkit_amd import registry
    want = {"r50k_base": 16, "p50k_base": 16, "p50k_edit": 16, "cl100k_base": 17}
    for name, (_, fname, specials) in registry.ENCODING_PARAMS.items():
        ranks, singles = [], 0
        with open(os.path.join(registry.DATA_DIR, fname), "rb") as f:
            for line in f:
                if line.strip():
                    tok, rank = line.split()
                    ranks.append(int(rank))
                    singles += len(base64.b64decode(tok)) == 1
        assert singles == 256                    # (all 256 single bytes are tokens: no pseudo ids above the table)
        max_id = max(max(ranks), max(specials.values()))
        assert 16 + sim.sim_compact_hb(max_id) == want[name], name


@pytest.mark.parametrize("hb", HBS)
def test_planes_of_random_streams(sim, hb):
    rng = np.random.default_rng(1000 + hb)
    for n in LENGTHS:
        ids = _stream(rng, n, hb)
        got = _sim_compact(sim, ids, hb)
        _same(got, compact_ref.compact(ids, hb))
        if hb and n:                                     # unused bits of the last word are zero
            used = n * hb - (len(got[1]) - 1) * 32
            assert used == 32 or int(got[1][-1]) >> used == 0


@pytest.mark.parametrize("hb", HBS)
def test_consecutive_ranges_equal_one_pass(sim, hb):
    rnd = random.Random(77 + hb)
    rng = np.random.default_rng(2000 + hb)
    for n in (1, 33, 64, 65, 1000, 100003):
        ids = _stream(rng, n, hb)
        whole = _sim_compact(sim, ids, hb)
        for trial in range(6):
            k = rnd.choice((1, 2, 5, 40))
            cuts = sorted({0, n} | {rnd.randrange(0, n + 1) for _ in range(k)})
            if trial == 0:
                cuts = sorted(set(cuts) | {min(n, 31), min(n, 32), min(n, 33)})
            assert n < 64 or any(c % 32 for c in cuts[1:-1]) or len(cuts) == 2
            _same(_sim_compact(sim, ids, hb, cuts), whole)
        # empty ranges among the cuts (chunks without tokens)
        _same(_sim_compact(sim, ids, hb, [0, 0, n // 2, n // 2, n, n]), whole)


@pytest.mark.parametrize("hb", HBS)
def test_widening_any_range(sim, hb):
    rnd = random.Random(5 + hb)
    rng = np.random.default_rng(3000 + hb)
    for n in LENGTHS:
        ids = _stream(rng, n, hb)
        lo, hi = compact_ref.compact(ids, hb)
        assert np.array_equal(compact_ref.widen(lo, hi, hb), ids)
        ranges = [(0, n), (0, 0), (n, 0)] + [(f, rnd.randrange(0, n - f + 1)) for f in (rnd.randrange(0, n + 1) for _ in range(20))]
        for first, m in ranges:
            out = np.full(m + 1, -5, dtype=np.int32)
            sim.sim_widen(lo.ctypes.data, hi.ctypes.data if hi is not None else None, hb, first, m, out.ctypes.data)
            assert out[m] == -5 and np.array_equal(out[:m], ids[first:first + m]), (n, first, m)


@pytest.mark.parametrize("name", golden_util.ENCODING_NAMES)
def test_golden_prompts_round_trip(sim, name):
    hb = {"cl100k_base": 1}.get(name, 0)
    docs = [toks for (_, toks, _) in golden_util.load_rows(name)]
    ids = np.array([t for d in docs for t in d], dtype=np.int32)
    assert len(ids) > 1000 and ids.max() < 1 << (16 + hb)
    off = np.zeros(len(docs) + 1, dtype=np.int64)
    np.cumsum([len(d) for d in docs], out=off[1:])
    lo, hi = _sim_compact(sim, ids, hb, off)                     # a range per document
    _same((lo, hi), compact_ref.compact(ids, hb))
    for d, toks in enumerate(docs):
        out = np.zeros(len(toks) + 1, dtype=np.int32)
        sim.sim_widen(lo.ctypes.data, hi.ctypes.data if hi is not None else None, hb, int(off[d]), len(toks), out.ctypes.data)
        assert out[:len(toks)].tolist() == toks
