"""CPU tier of the MinHash pass (jtk_batch_minhash, jtk_batch_minhash_agree): the rule header
jtokkit_amd/csrc/jtk_minhash_rules.h -- run serially through the shim tests/minhash_sim the way the kernels partition a batch
into tiles -- against the plain restatement tests/minhash_ref.py on every case of tests/minhash_cases.py: signatures, shingle
counts, band keys and agreement, exactly.  The case set is checked to reach every edge it names (from the oracle's token
counts) and to tell the right rule from seven wrong ones; the estimator is held to the binomial bound on 54 fixed pairs; the
near-duplicate procedure of the restatement finds the expected clusters of a 40-document batch; and a stand-alone sanitizer
build of the shim runs every case in buffers of exactly the arrays' sizes.  No GPU."""
import ctypes as C
import math
import os
import struct
import subprocess

import numpy as np
import pytest

import minhash_cases as mc
import minhash_ref as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIM_DIR = os.path.join(ROOT, "tests", "minhash_sim")
_IDS, _REF = {}, {}

CASES = {c.name: c for c in mc.cases()}
CASE_NAMES = (["lengths_n%d" % n for n in (1, 2, 5, 32)] + ["straddle_n%d" % n for n in (2, 5, 32)] + ["doc_edges", "short_straddles"]
              + ["empty_runs_%d" % r for r in (1, 2, 65)] + ["three_tiles", "one_doc_one_tile", "many_short", "refused_special", "refused_utf8",
                                                              "allow_special", "fim", "chunked"])
RUNS = [(name, p) for name in CASE_NAMES for p in CASES[name].params]


def ids_of(case):
    if case.name not in _IDS:
        _IDS[case.name] = mc.expected_ids(case)
    return _IDS[case.name]


def ref(case, params):
    """The reference's result for a case and one parameter set, computed once."""
    if (case.name, params) not in _REF:
        n, K, bands, seed = params
        _REF[(case.name, params)] = mr.minhash(ids_of(case)[0], seed, n, K, bands)
    return _REF[(case.name, params)]


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("minhash_sim") / "libminhash_sim.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas", "-o", out,
                           os.path.join(SIM_DIR, "minhash_sim.cpp")])
    L = C.CDLL(out)
    L.sim_mh_batch.restype = C.c_int64
    L.sim_mh_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_uint64, C.c_int32, C.c_int32, C.c_int32, C.c_int, C.c_void_p,
                               C.c_void_p, C.c_void_p]
    L.sim_mh_agree.restype = None
    L.sim_mh_agree.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    L.sim_mh_g.restype = C.c_uint64
    L.sim_mh_empty.restype = C.c_uint32
    L.sim_mh_value.restype = C.c_uint32
    L.sim_mh_value.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32]
    L.sim_mh_params_ok.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_uint32]
    return L


def arrays(ids, status):
    """tokens, tok_off and status as the device holds them (one spare token: an address for an empty batch)."""
    tok_off = np.zeros(len(ids) + 1, dtype=np.int64)
    if ids:
        np.cumsum([len(x) for x in ids], out=tok_off[1:])
    tokens = np.array([t for x in ids for t in x] + [0], dtype=np.int32)
    return tokens, tok_off, np.array(list(status) + [0], dtype=np.int32)


def sim_batch(sim, ids, status, params, order=0, want_keys=True):
    n, K, bands, seed = params
    tokens, tok_off, st = arrays(ids, status)
    nd = len(ids)
    sig = np.full((nd, K), 0x5A5A5A5A, dtype=np.uint32)
    nsh = np.full(nd, -7, dtype=np.int32)
    keys = np.full((nd, bands), 0x77, dtype=np.uint64) if bands else None
    rc = sim.sim_mh_batch(tokens.ctypes.data, tok_off.ctypes.data, st.ctypes.data, nd, seed, n, K, bands, order, sig.ctypes.data, nsh.ctypes.data,
                          keys.ctypes.data if bands and want_keys else None)
    assert rc >= 0
    return sig, nsh, keys, rc


def sim_agree(sim, sig, pairs):
    pa = np.array([p for p, _ in pairs] + [0], dtype=np.int64)
    pb = np.array([q for _, q in pairs] + [0], dtype=np.int64)
    out = np.full(len(pairs) + 1, -9, dtype=np.int32)
    s = np.ascontiguousarray(sig)
    sim.sim_mh_agree(s.ctypes.data, len(s), s.shape[1], pa.ctypes.data, pb.ctypes.data, len(pairs), out.ctypes.data)
    assert out[-1] == -9
    return out[:-1]


def test_header_constants_are_pinned(sim):
    assert sim.sim_mh_tile() == mc.TILE == 512
    assert sim.sim_mh_block_tiles() == 4 and sim.sim_mh_lane_hashes() == 4
    assert sim.sim_mh_max_hashes() == 256 == 64 * sim.sim_mh_lane_hashes() and max(mc.HASH_COUNTS) == sim.sim_mh_max_hashes()
    assert sim.sim_mh_max_ngram() == 32 == max(mc.NGRAMS)
    assert sim.sim_mh_g() == mr.G == 0x9E3779B97F4A7C15 and sim.sim_mh_empty() == mr.EMPTY == 0xFFFFFFFF


def test_case_names_are_the_case_set():
    assert list(CASES) == CASE_NAMES


def test_parameter_ranges(sim):
    ok = lambda n, K, b, f=0: bool(sim.sim_mh_params_ok(n, K, b, f))
    assert ok(1, 1, 0) and ok(32, 256, 256) and ok(5, 128, 16) and ok(5, 100, 20) and ok(5, 63, 9) and ok(5, 1, 1)
    assert not ok(0, 128, 0) and not ok(33, 128, 0) and not ok(-1, 128, 0)
    assert not ok(5, 0, 0) and not ok(5, 257, 0) and not ok(5, -4, 0)
    assert not ok(5, 128, -1) and not ok(5, 128, 3) and not ok(5, 100, 128) and not ok(5, 63, 2)
    assert not ok(5, 128, 16, 1) and not ok(5, 128, 0, 0x80000000)


def test_multiply_add_shift_in_two_words_is_the_64_bit_rule(sim):
    """The device's form (a 32 x 32 + 64 multiply-add and a 32-bit multiply) against Python integers, at the carries."""
    top = (1 << 64) - 1
    for a in (1, 3, top, 0xFFFFFFFF, 0x100000001, 0x9E3779B97F4A7C15, 0xFFFFFFFF00000001, 0x80000000FFFFFFFF):
        for b in (0, 1, top, 0xFFFFFFFF, 0x100000000, 0xFFFFFFFF00000000, 0x123456789ABCDEF0):
            for x in (0, 1, 2, 0xFFFFFFFF, 0x80000000, 0x7FFFFFFF, 0xDEADBEEF):
                assert sim.sim_mh_value(a, b, x) == ((a * x + b) & top) >> 32, (hex(a), hex(b), hex(x))


def test_reference_on_hand_computed_values():
    """The restatement itself, on values small enough to check by hand, and its array form against its integer form."""
    assert mr.mix(0) == 0 and mr.mix(0x9E3779B97F4A7C15) == 0xE220A8397B1DCDAF       # splitmix64's first output from state 0
    assert mr.n_shingles(0, 5) == 0 and mr.n_shingles(1, 5) == 1 and mr.n_shingles(4, 5) == 1 and mr.n_shingles(5, 5) == 1
    assert mr.n_shingles(6, 5) == 2 and mr.n_shingles(7, 1) == 7
    assert mr.shingle_sets([1, 2, 3], 2) == {(1, 2), (2, 3)} and mr.shingle_sets([1, 2], 5) == {(1, 2)} and mr.shingle_sets([], 2) == set()
    assert mr.jaccard([1, 2, 3], [2, 3, 4], 2) == 1 / 3 and mr.jaccard([1, 2, 3], [1, 2, 3], 2) == 1.0
    # one shingle of one token: H = id + 1
    key = mr.key_of(9, 1)
    x = mr.mix((41 + 1) ^ key) & 0xFFFFFFFF
    assert mr.plain_signature([41], 9, 1, 2) == [((((mr.draw(key, 2 * k + 1) | 1) * x + mr.draw(key, 2 * k + 2)) & mr.M64) >> 32) for k in (0, 1)]
    # H of (3, 4): (3 + 1) G + (4 + 1); a negative id counts as its uint32 pattern
    key = mr.key_of(0, 2)
    assert int(mr.shingle_x([3, 4], key, 2)[0]) == mr.mix(((4 * mr.G + 5) & mr.M64) ^ key) & 0xFFFFFFFF
    assert int(mr.shingle_x([-1], key, 1)[0]) == mr.mix((0xFFFFFFFF + 1) ^ key) & 0xFFFFFFFF
    docs = [[5, 6, 7, 8, 9, 10, 11], [5], [], [100000, -2, 7], list(range(50))]
    for n, K, seed in ((1, 3, 0), (2, 5, 1), (5, 4, mr.M64), (32, 2, 77)):
        r = mr.minhash(docs, seed, n, K, K)
        for d, ids in enumerate(docs):
            assert r.sig[d].tolist() == mr.plain_signature(ids, seed, n, K), (n, K, seed, d)
        key = mr.key_of(seed, n)
        assert int(r.band_keys[0, 1]) == mr.mix(mr.draw(key, (1 << 32) + 1) ^ int(r.sig[0, 1]))
    assert mr.agree(np.array([[1, 2, 3], [1, 5, 3]]), [0, 0, 1, 2, -1], [1, 0, 0, 0, 0]).tolist() == [2, 3, 2, -1, -1]


@pytest.mark.parametrize("name,params", RUNS, ids=["%s-n%d-K%d-b%d-s%s" % (n, p[0], p[1], p[2], "max" if p[3] else "0") for n, p in RUNS])
def test_rule_header_equals_the_restatement(sim, name, params):
    case = CASES[name]
    ids, status = ids_of(case)
    exp = ref(case, params)
    results = []
    for order in (0, 1):
        sig, nsh, keys, combines = sim_batch(sim, ids, status, params, order)
        assert np.array_equal(nsh, exp.n_shingles), (name, np.flatnonzero(nsh != exp.n_shingles)[:10])
        assert np.array_equal(sig, exp.sig), (name, order, np.flatnonzero((sig != exp.sig).any(axis=1))[:10])
        if params[2]:
            assert np.array_equal(keys, exp.band_keys), (name, order)
        results.append(combines)
    assert results[0] == results[1]
    # band keys may be left out: the buffer is then untouched
    if params[2]:
        sig, nsh, keys, _ = sim_batch(sim, ids, status, params, want_keys=False)
        assert np.array_equal(sig, exp.sig) and (keys == 0x77).all()
    pairs = mc.agree_pairs(len(ids))
    assert np.array_equal(sim_agree(sim, exp.sig, pairs), mr.agree(exp.sig, [p for p, _ in pairs], [q for _, q in pairs]))
    assert len(sim_agree(sim, exp.sig, [])) == 0


def test_a_status_below_zero_means_no_shingles_whatever_the_offsets_say(sim):
    """The encode leaves a refused document without tokens; the pass does not rely on it."""
    ids = [[1, 2, 3, 4, 5, 6, 7], [8, 9, 10, 11, 12, 13], [14, 15, 16, 17, 18, 19]]
    params = (2, 64, 8, 3)
    sig, nsh, keys, _ = sim_batch(sim, ids, [0, -2, 0], params)
    exp = mr.minhash([ids[0], [], ids[2]], 3, 2, 64, 8)
    assert np.array_equal(sig, exp.sig) and nsh.tolist() == [6, 0, 5] and np.array_equal(keys, exp.band_keys)


def test_case_set_reaches_the_edges():
    reached = set()
    for case in CASES.values():
        ids, status = ids_of(case)
        reached |= mc.edges_reached(case, [len(x) for x in ids], status)
    assert mc.all_edges() - reached == set()
    # the refused documents are refused for the reason their case names; the routes' ids are what the routes make
    assert ids_of(CASES["refused_special"])[1] == [0, -2, 0, 0] and ids_of(CASES["refused_utf8"])[1] == [0, -6, 0, 0]
    assert 100257 in ids_of(CASES["allow_special"])[0][0] and ids_of(CASES["allow_special"])[0][1] == [100257]
    assert any(set(mc.FIM_IDS) <= set(x) for x in ids_of(CASES["fim"])[0])
    assert sum(len(d) for d in CASES["chunked"].docs) > 2 * mc.CHUNK_BYTES
    # documents that span tiles are combined, the others stored: both happen in one batch
    assert len(ids_of(CASES["three_tiles"])[0][2]) == 2 * mc.TILE + 12


def test_case_set_tells_the_right_rule_from_wrong_ones():
    """Each wrong rule changes some case's result."""
    for wrong in mr.WRONG_RULES:
        changed = []
        for name, params in RUNS:
            case = CASES[name]
            if name == "chunked":
                continue
            n, K, bands, seed = params
            exp = ref(case, params)
            got = mr.minhash(ids_of(case)[0], seed, n, K, bands, wrong=wrong, tile=mc.TILE)
            if not (np.array_equal(got.sig, exp.sig) and np.array_equal(got.n_shingles, exp.n_shingles)
                    and (bands == 0 or np.array_equal(got.band_keys, exp.band_keys))):
                changed.append(name)
        assert changed, wrong
    assert len(mr.WRONG_RULES) == 7


def test_estimator_stays_inside_the_binomial_bound():
    """|agree / K - J| <= 5 sqrt(J (1 - J) / K) + 1 / K on the 54 fixed pairs, J the true Jaccard similarity of the two shingle
    sets: the binomial standard error, 5 sigma to keep 54 draws clear of chance; exact at J = 0 and J = 1."""
    o = mc.oracle()
    worst, count = 0.0, 0
    for f, a, b in mc.estimator_pairs():
        ia, ib = o.encode_ordinary(a), o.encode_ordinary(b)
        assert len(ia) == len(ib) == mc.EST_LEN
        for n in mc.EST_NGRAMS:
            J = mr.jaccard(ia, ib, n)
            if f == 0.0:
                assert J == 0.0
            if f == 1.0:
                assert J == 1.0
            for seed in mc.EST_SEEDS:
                r = mr.minhash([ia, ib], seed, n, mc.EST_K)
                est = int(mr.agree(r.sig, [0], [1])[0]) / mc.EST_K
                sigma = math.sqrt(J * (1 - J) / mc.EST_K)
                print("f=%.1f n=%d seed=%d J=%.4f estimate=%.4f sigmas=%.2f" % (f, n, seed, J, est, abs(est - J) / sigma if sigma else 0.0))
                assert abs(est - J) <= 5 * sigma + 1 / mc.EST_K, (f, n, seed, J, est)
                worst = max(worst, abs(est - J) / sigma if sigma else 0.0)
                count += 1
    assert count == 54
    print("worst: %.2f sigma" % worst)


def test_near_duplicates_of_the_reference_finds_the_expected_clusters():
    docs, labels = mc.near_dup_batch()
    o = mc.oracle()
    ids = [o.encode_ordinary(d) for d in docs]
    assert sorted(len(x) for x in ids)[:4] == [0, 0, 0, 2] and sorted(len(x) for x in ids)[4] == mc.NEAR_LEN
    got = mr.near_duplicates(ids, mc.NEAR["threshold"], mc.NEAR["seed"], mc.NEAR["ngram"], mc.NEAR["num_hashes"], mc.NEAR["bands"])
    assert np.array_equal(got, labels), (got.tolist(), labels.tolist())
    # the partition has clusters of 4 (an original, two copies, one variant), 2, 4, 3 and singletons
    sizes = sorted(np.bincount(labels)[np.bincount(labels) > 0].tolist(), reverse=True)
    assert sizes[:5] == [4, 4, 3, 2, 1] and len(sizes) == 40 - 3 - 3 - 2 - 1
    # a replaced copy is above the threshold by the true similarity too, an unrelated pair far below
    sets = [mr.shingle_sets(x, mc.NEAR["ngram"]) for x in ids]
    for d in range(40):
        for e in range(d + 1, 40):
            if sets[d] and sets[e]:
                J = len(sets[d] & sets[e]) / len(sets[d] | sets[e])
                assert J < 0.2 or labels[d] == labels[e]


def test_sanitizer_build_runs_every_case_in_exact_buffers(tmp_path):
    exe = str(tmp_path / "minhash_sim_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, os.path.join(SIM_DIR, "minhash_sim_main.cpp")])
    cases, results = str(tmp_path / "cases.bin"), str(tmp_path / "results.bin")
    with open(cases, "wb") as f:
        for name, (n, K, bands, seed) in RUNS:
            ids, status = ids_of(CASES[name])
            tokens, tok_off, st = arrays(ids, status)
            pairs = mc.agree_pairs(len(ids))
            f.write(struct.pack("<2qQ4q", len(ids), len(tokens) - 1, seed, n, K, bands, len(pairs)))
            f.write(tok_off.astype("<i8").tobytes())
            f.write(st[:-1].astype("<i4").tobytes())
            f.write(tokens[:-1].astype("<i4").tobytes())
            f.write(np.array([p for p, _ in pairs], dtype="<i8").tobytes())
            f.write(np.array([q for _, q in pairs], dtype="<i8").tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe, cases, results], env=env, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-4000:]
    assert p.stdout.strip() == "%d cases" % len(RUNS)
    raw = open(results, "rb").read()
    at = 0
    for name, params in RUNS:
        exp = ref(CASES[name], params)
        pairs = mc.agree_pairs(len(exp.sig))
        want = [(exp.sig, "<u4"), (exp.n_shingles, "<i4")] + ([(exp.band_keys, "<u8")] if params[2] else [])
        want.append((mr.agree(exp.sig, [p for p, _ in pairs], [q for _, q in pairs]), "<i4"))
        for e, dt in want:
            got = np.frombuffer(raw, dtype=dt, count=e.size, offset=at)
            at += got.nbytes
            assert np.array_equal(got, e.ravel()), (name, params)
    assert at == len(raw)


def test_abi_refuses_what_needs_no_device():
    """What the two entry points refuse before they touch a device, and the parameter struct's layout."""
    so = os.path.join(ROOT, "jtokkit_amd", "libjtokkit_amd.so")
    if not os.path.exists(so):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "jtokkit_amd", "csrc")])
    from jtokkit_amd import _native as N
    L = N.lib()
    p = N.MinhashParamsStruct(0, 5, 128, 16, 0)
    assert C.sizeof(N.MinhashParamsStruct) == 24
    assert L.jtk_batch_minhash(None, C.byref(p), None, None, None, None) == N.JTK_ERR_INVALID_ARGUMENT
    assert L.jtk_batch_minhash_agree(None, None, 0, 128, None, None, 0, None, None) == N.JTK_ERR_INVALID_ARGUMENT
    import jtokkit_amd
    for name in ("minhash", "minhash_agree"):
        assert callable(getattr(jtokkit_amd.encoding.Batch, name))
    for name in ("minhash_batch", "minhash_batch_device", "near_duplicates"):
        assert callable(getattr(jtokkit_amd.HipEncoding, name))
