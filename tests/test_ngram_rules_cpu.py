"""CPU tier of the n-gram set and overlap pass (jtk_ngram_set_*, jtk_batch_ngram_overlap): the rule header
jtokkit_amd/csrc/jtk_ngram_rules.h -- run serially through the shim tests/ngram_sim the way the kernels partition a batch into
tiles and lanes, tiles ascending and descending, insert orders shuffled -- against the plain restatement tests/ngram_ref.py on
every case of tests/ngram_cases.py: the sorted keys, the key count, the capacity, the flags and the three per-document arrays,
exactly.  The case set is checked to reach every edge it names (from the oracle's ids) and to tell the right rule from eight
wrong ones, no case passes or fails through a hash collision, and a stand-alone sanitizer build of the shim runs every case in
buffers of exactly the arrays' sizes.  No GPU."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import ngram_cases as nc
import ngram_ref as nr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIM_DIR = os.path.join(ROOT, "tests", "ngram_sim")
_BUILT, _REF = {}, {}

CASES = {c.name: c for c in nc.cases()}
CASE_NAMES = (["lengths_n%d" % n for n in (1, 2, 13, 32)] + ["straddle_n%d" % n for n in (2, 13, 32)] + ["patterns_n2", "patterns_n13", "doc_ends"]
              + ["empty_runs_%d" % r for r in (1, 2, 65)] + ["three_tiles_n13", "three_tiles_n1", "many_short", "refused_special", "refused_utf8",
                                                              "allow_special", "fim", "set_wrap", "set_chain", "set_dups", "set_grow_exact",
                                                              "set_grow_plus2", "set_grow_second", "set_grow_batch", "set_empty"])
WALKS = ((0, 0), (1, 7), (0, 99))             # (tile order, shuffle)


def corpus_of(case):
    """The corpus ids and statuses; a refused document keeps its tokens, which the rule must not look at."""
    if case.name not in _BUILT:
        _BUILT[case.name] = nc.ids_of(case.docs, case.route, keep_refused=True)
    return _BUILT[case.name]


def ref(case):
    """(the reference set, what fed it, the reference's overlap result), computed once."""
    if case.name not in _REF:
        s, fed = nc.build_set(case)
        ids, status = corpus_of(case)
        _REF[case.name] = (s, fed, nr.overlap(ids, status, s))
    return _REF[case.name]


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("ngram_sim") / "libngram_sim.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas", "-o", out,
                           os.path.join(SIM_DIR, "ngram_sim.cpp")])
    L = C.CDLL(out)
    p, i64, u64, i32 = C.c_void_p, C.c_int64, C.c_uint64, C.c_int32
    L.sim_ng_params_ok.argtypes = [i32, C.c_uint32]
    for name, res, args in (("sim_ng_key", u64, [u64, i32]), ("sim_ng_finish", u64, [u64, u64]), ("sim_ng_capacity", i64, [i64, i64]),
                            ("sim_ng_k", u64, [p, i32, u64]), ("sim_ng_k_rolled", u64, [p, i32, u64]), ("sim_ng_lookup", C.c_int, [p, i64, u64]),
                            ("sim_ng_count", i64, [p, p, i64, i32]), ("sim_ng_insert_keys", i64, [p, i64, p, i64, u64]),
                            ("sim_ng_insert_batch", i64, [p, p, p, i64, u64, i32, p, i64, C.c_int, u64]),
                            ("sim_ng_overlap", i64, [p, p, p, i64, u64, i32, p, i64, C.c_int, p, p, p, p])):
        getattr(L, name).restype, getattr(L, name).argtypes = res, args
    return L


def arrays(ids, status):
    """tokens, tok_off and status as the device holds them (one spare token: an address for an empty batch)."""
    tok_off = np.zeros(len(ids) + 1, dtype=np.int64)
    if ids:
        np.cumsum([len(x) for x in ids], out=tok_off[1:])
    tokens = np.array([t for x in ids for t in x] + [0], dtype=np.int32)
    return tokens, tok_off, np.array(list(status) + [0], dtype=np.int32)


class SimSet:
    """The host side of a set over the shim: the count, the capacity rule and the rehash through the same insert."""

    def __init__(self, sim, seed, n):
        self.sim, self.seed, self.n = sim, seed, n
        self.table = np.zeros(sim.sim_ng_min_capacity(), dtype=np.uint64)
        self.count = 0

    def reserve(self, m, shuffle):
        cap = self.sim.sim_ng_capacity(self.count, m)
        if cap > len(self.table):
            grown = np.zeros(cap, dtype=np.uint64)
            assert self.sim.sim_ng_insert_keys(self.table.ctypes.data, len(self.table), grown.ctypes.data, cap, shuffle) == self.count
            self.table = grown

    def add_keys(self, keys, shuffle):
        keys = np.array(keys, dtype=np.uint64)
        self.reserve(len(keys), shuffle)
        self.count += self.sim.sim_ng_insert_keys(keys.ctypes.data, len(keys), self.table.ctypes.data, len(self.table), shuffle)

    def add_batch(self, ids, status, order, shuffle):
        tokens, tok_off, st = arrays(ids, status)
        self.reserve(self.sim.sim_ng_count(tok_off.ctypes.data, st.ctypes.data, len(ids), self.n), shuffle)
        self.count += self.sim.sim_ng_insert_batch(tokens.ctypes.data, tok_off.ctypes.data, st.ctypes.data, len(ids), self.seed, self.n,
                                                   self.table.ctypes.data, len(self.table), order, shuffle)

    def keys(self):
        return np.sort(self.table[self.table != 0])

    def overlap(self, ids, status, order, want=(True, True, True, True)):
        tokens, tok_off, st = arrays(ids, status)
        nd, nt = len(ids), int(tok_off[-1])
        outs = [np.full(nt + 1, 0x5A, dtype=np.uint8), np.full(nd + 1, -7, dtype=np.int32), np.full(nd + 1, -7, dtype=np.int32),
                np.full(nd + 1, -7, dtype=np.int64)]
        rc = self.sim.sim_ng_overlap(tokens.ctypes.data, tok_off.ctypes.data, st.ctypes.data, nd, self.seed, self.n, self.table.ctypes.data,
                                     len(self.table), order, *[o.ctypes.data if w else None for o, w in zip(outs, want)])
        assert rc >= 0
        for o, w, guard in zip(outs, want, (0x5A, -7, -7, -7)):
            assert o[-1] == guard and (w or (o == guard).all())
        return [o[:-1] for o in outs]


def sim_set(sim, case, order, shuffle):
    s = SimSet(sim, case.seed, case.n)
    for f in nc.build_set(case)[1]:
        if f[0] == "keys":
            s.add_keys(f[1], shuffle)
        else:
            s.add_batch(f[1], f[2], order, shuffle)
    return s


def test_header_constants_are_pinned(sim):
    assert sim.sim_ng_tile() == nc.TILE == 512 and sim.sim_ng_lane() == nc.LANE == 8 and sim.sim_ng_tile() == 64 * sim.sim_ng_lane()
    assert sim.sim_ng_block_tiles() == 4 and sim.sim_ng_max_ngram() == 32 == max(nc.NGRAMS)
    assert sim.sim_ng_min_capacity() == nr.MIN_CAPACITY == 64
    assert sim.sim_ng_start() == nr.START == 1 and sim.sim_ng_covered() == nr.COVERED == 2
    hdr = open(os.path.join(ROOT, "include", "jtokkit_amd.h")).read()
    assert "#define JTK_NG_START 1\n" in hdr and "#define JTK_NG_COVERED 2\n" in hdr


def test_case_names_are_the_case_set():
    assert list(CASES) == CASE_NAMES


def test_parameter_ranges_key_and_capacity(sim):
    ok = lambda n, f=0: bool(sim.sim_ng_params_ok(n, f))
    assert ok(1) and ok(13) and ok(32) and not ok(0) and not ok(33) and not ok(-1) and not ok(13, 1) and not ok(13, 1 << 31)
    for seed in (0, 1, nc.MAX_SEED, 0x123456789ABCDEF0):
        for n in (1, 2, 13, 32):
            assert sim.sim_ng_key(seed, n) == nr.key_of(seed, n) == nr.mix(seed + nr.G * (n + 33))
    import minhash_ref
    assert nr.key_of(5, 13) != minhash_ref.key_of(5, 13) and nr.key_of(5, 1) == minhash_ref.key_of(5, 33)     # (n + 33 against n + 1)
    for c, m, cap in ((0, 0, 64), (0, 32, 64), (0, 33, 128), (31, 1, 64), (32, 1, 128), (100, 0, 256), (24, 9, 128), (1 << 20, 1, 1 << 22)):
        assert sim.sim_ng_capacity(c, m) == nr.capacity(c, m) == cap, (c, m)


def test_k_of_zero_becomes_g_and_rolled_is_direct(sim):
    """mix is a bijection with mix(0) = 0, so k would be 0 exactly when H == key: the rule makes it G.  At rule level only."""
    for key in (1, nr.G, nr.key_of(0, 13), nc.MAX_SEED):
        assert nr.mix(key ^ key) == 0 and sim.sim_ng_finish(key, key) == nr.G
        assert sim.sim_ng_finish(key ^ 1, key) == nr.mix(1) != 0
    assert nr.k_of([], 0) == nr.G                                           # (H = 0, key = 0: the restatement's own zero)
    rng = np.random.RandomState(3)
    t = np.concatenate([rng.randint(0, 100277, size=70), [-1, 0, 0x7FFFFFFF, -2]]).astype(np.int32)
    for n in (1, 2, 13, 32):
        key = nr.key_of(n, n)
        for i in range(1, len(t) - n + 1):
            want = nr.k_of(t[i:i + n].tolist(), key)
            at = t.ctypes.data + 4 * i
            assert sim.sim_ng_k(at, n, key) == want and sim.sim_ng_k_rolled(at, n, key) == want, (n, i)


def test_reference_on_hand_computed_values():
    assert nr.mix(0) == 0 and nr.mix(nr.G) == 0xE220A8397B1DCDAF            # splitmix64's first output from state 0
    assert [nr.n_ngrams(l, 3) for l in (0, 2, 3, 4)] == [0, 0, 1, 2]
    key = nr.key_of(0, 2)
    assert nr.k_of([3, 4], key) == nr.mix(((4 * nr.G + 5) & nr.M64) ^ key) and nr.k_of([-1], key) == nr.mix((0xFFFFFFFF + 1) ^ key)
    s = nr.Set(0, 2)
    s.add_docs([[1, 2, 3], [9], [7, 8]], [0, 0, -2])
    assert s.keys == {nr.k_of([1, 2], key), nr.k_of([2, 3], key)} and s.capacity == 64
    r = nr.overlap([[5, 1, 2, 3, 6, 2, 3], [2], [3, 1, 2], [1, 2, 3]], [0, 0, 0, -6], s)
    assert r.flags.tolist() == [0, 3, 3, 2, 0, 3, 2, 0, 0, 3, 2, 0, 0, 0]
    assert r.n_hit.tolist() == [3, 0, 1, 0] and r.n_covered.tolist() == [5, 0, 2, 0] and r.first_hit.tolist() == [1, -1, 1, -1]
    t = nr.Set(0, 1)
    t.add_keys([63, 127, 191, 5, 63])
    assert t.table()[63] == 63 and t.table()[0] == 127 and t.table()[1] == 191 and len(t.keys) == 4
    assert t.contains(191) and not t.contains(191, "probe_no_wrap", t.table()) and not t.contains(127, "probe_stops_at_mismatch", t.table())


@pytest.mark.parametrize("name", CASE_NAMES)
def test_rule_header_equals_the_restatement(sim, name):
    case = CASES[name]
    exp_set, _, exp = ref(case)
    ids, status = corpus_of(case)
    for order, shuffle in WALKS:
        s = sim_set(sim, case, order, shuffle)
        assert s.count == len(exp_set.keys) and len(s.table) == exp_set.capacity, (name, order, shuffle, s.count, len(s.table))
        assert np.array_equal(s.keys(), np.array(sorted(exp_set.keys), dtype=np.uint64)), (name, order, shuffle)
        flags, n_hit, n_cov, first = s.overlap(ids, status, order)
        assert np.array_equal(flags, exp.flags), (name, order, np.flatnonzero(flags != exp.flags)[:10])
        assert np.array_equal(n_hit, exp.n_hit) and np.array_equal(n_cov, exp.n_covered) and np.array_equal(first, exp.first_hit), (name, order)
    # outputs that are not asked for are not written
    for want in ((True, False, False, False), (False, True, False, False), (False, False, True, True)):
        got = s.overlap(ids, status, 0, want)
        for g, e, w in zip(got, (exp.flags, exp.n_hit, exp.n_covered, exp.first_hit), want):
            assert not w or np.array_equal(g, e), (name, want)
    # every key of the set is found in the shim's table, wherever the insert order put it
    for k in list(exp_set.keys)[:200]:
        assert sim.sim_ng_lookup(s.table.ctypes.data, len(s.table), k)
    assert not sim.sim_ng_lookup(s.table.ctypes.data, len(s.table), 12345) or 12345 in exp_set.keys


def test_case_set_reaches_the_edges():
    reached = set()
    for case in CASES.values():
        s, fed, exp = ref(case)
        ids, status = corpus_of(case)
        reached |= nc.edges_reached(case, ids, status, s, fed, exp)
    assert nc.all_edges() - reached == set()
    assert corpus_of(CASES["refused_special"])[1] == [0, -2, 0, 0, 0] and corpus_of(CASES["refused_utf8"])[1] == [0, -6, 0, 0, 0]
    assert len(corpus_of(CASES["refused_special"])[0][1]) > 5            # (the refused document has tokens here: they must not count)
    assert 100257 in corpus_of(CASES["allow_special"])[0][0] and any(set(nc.mc.FIM_IDS) <= set(x) for x in corpus_of(CASES["fim"])[0])
    assert [ref(CASES[n])[0].capacity for n in ("set_grow_exact", "set_grow_plus2", "set_grow_second", "set_grow_batch")] == [64, 128, 128, 128]
    assert len(ref(CASES["set_dups"])[0].keys) == 3 and ref(CASES["set_empty"])[0].capacity == 64 and not ref(CASES["set_empty"])[2].flags.any()


def test_case_set_tells_the_right_rule_from_wrong_ones():
    """Each wrong rule changes some case's keys, key count, capacity or overlap result."""
    for wrong in nr.WRONG_RULES:
        changed = []
        for name in CASE_NAMES:
            case = CASES[name]
            exp_set, _, exp = ref(case)
            ids, status = corpus_of(case)
            s, _ = nc.build_set(case, wrong)
            got = nr.overlap(ids, status, s, wrong=wrong, tile=nc.TILE)
            if not (s.keys == exp_set.keys and s.capacity == exp_set.capacity and np.array_equal(got.flags, exp.flags)
                    and np.array_equal(got.n_hit, exp.n_hit) and np.array_equal(got.n_covered, exp.n_covered)
                    and np.array_equal(got.first_hit, exp.first_hit)):
                changed.append(name)
        assert changed, wrong
    assert len(nr.WRONG_RULES) == 8


def test_no_case_depends_on_a_hash_collision():
    """The exact id tuples of all n-grams of a case -- the set's sources and the corpus -- and their k are as many."""
    for case in CASES.values():
        key = nr.key_of(case.seed, case.n)
        grams = set()
        for f in ref(case)[1]:
            if f[0] == "batch":
                grams |= {tuple(g) for here in nr.starts(f[1], f[2], case.n) for _, g in here}
        for kind, what, *_ in case.steps:
            if kind == "keys":
                grams |= {tuple(nc.oracle().encode_ordinary(g)) for g in what}
        ids, status = corpus_of(case)
        grams |= {tuple(g) for here in nr.starts(ids, status, case.n) for _, g in here}
        assert len({nr.k_of(g, key) for g in grams}) == len(grams), case.name
        assert nr.G not in {nr.k_of(g, key) for g in grams}


def test_sanitizer_build_runs_every_case_in_exact_buffers(tmp_path):
    exe = str(tmp_path / "ngram_sim_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, os.path.join(SIM_DIR, "ngram_sim_main.cpp")])
    cases, results = str(tmp_path / "cases.bin"), str(tmp_path / "results.bin")
    records = []                                  # (ids, status, seed, n, keys, capacity, order, insert_batch, expected set, expected overlap)
    for i, name in enumerate(CASE_NAMES):
        case = CASES[name]
        exp_set, fed, exp = ref(case)
        ids, status = corpus_of(case)
        records.append((ids, status, case, sorted(exp_set.keys), exp_set.capacity, i & 1, 0, exp_set, exp))
        for f in fed:                             # a source batch into an empty table of the rule's capacity, overlapped with itself
            if f[0] == "batch":
                own = nr.Set(case.seed, case.n)
                own.add_docs(f[1], f[2])
                records.append((f[1], f[2], case, [], own.capacity, i & 1, 1, own, nr.overlap(f[1], f[2], own)))
    with open(cases, "wb") as f:
        for ids, status, case, keys, cap, order, insert, _, _ in records:
            tokens, tok_off, st = arrays(ids, status)
            f.write(struct.pack("<2qQ5q", len(ids), len(tokens) - 1, case.seed, case.n, len(keys), cap, order, insert))
            f.write(tok_off.astype("<i8").tobytes())
            f.write(st[:-1].astype("<i4").tobytes())
            f.write(tokens[:-1].astype("<i4").tobytes())
            f.write(np.array(keys, dtype="<u8").tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe, cases, results], env=env, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-4000:]
    assert p.stdout.strip() == "%d cases" % len(records)
    raw = open(results, "rb").read()
    at = 0
    for ids, status, case, keys, cap, order, insert, exp_set, exp in records:
        want = [(np.array([len(exp_set.keys)]), "<i8"), (np.array(sorted(exp_set.keys), dtype=np.uint64), "<u8"), (exp.flags, "u1"),
                (exp.n_hit, "<i4"), (exp.n_covered, "<i4"), (exp.first_hit, "<i8")]
        for e, dt in want:
            got = np.frombuffer(raw, dtype=dt, count=e.size, offset=at)
            at += got.nbytes
            assert np.array_equal(got, e.ravel()), (case.name, insert, dt)
    assert at == len(raw)


def test_abi_refuses_what_needs_no_device():
    """What the entry points refuse before they touch a device, and the parameter struct's layout."""
    so = os.path.join(ROOT, "jtokkit_amd", "libjtokkit_amd.so")
    if not os.path.exists(so):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "jtokkit_amd", "csrc")])
    from jtokkit_amd import _native as N
    L = N.lib()
    assert C.sizeof(N.NgramParamsStruct) == 16 and N.JTK_NG_START == 1 and N.JTK_NG_COVERED == 2
    p = N.NgramParamsStruct(0, 13, 0)
    h = C.c_void_p()
    assert L.jtk_ngram_set_create(None, C.byref(p), C.byref(h)) == N.JTK_ERR_INVALID_ARGUMENT and not h.value
    for call in (lambda: L.jtk_ngram_set_add_batch(None, None, None), lambda: L.jtk_ngram_set_add_keys(None, None, 0),
                 lambda: L.jtk_ngram_set_size(None, None, None), lambda: L.jtk_ngram_set_keys(None, None, 0),
                 lambda: L.jtk_batch_ngram_overlap(None, None, None, None, None, None, None)):
        assert call() == N.JTK_ERR_INVALID_ARGUMENT and N.last_error()
    L.jtk_ngram_set_destroy(None)
    import jtokkit_amd
    assert callable(jtokkit_amd.encoding.Batch.ngram_overlap)
    for name in ("ngram_set", "ngram_overlap_batch", "ngram_overlap_batch_device"):
        assert callable(getattr(jtokkit_amd.HipEncoding, name))
    for name in ("add_texts", "add_last_encode", "add_keys", "keys", "close", "__len__"):
        assert callable(getattr(jtokkit_amd.NgramSet, name))
    assert isinstance(jtokkit_amd.NgramSet.capacity, property)
