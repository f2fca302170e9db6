"""CPU tier of the repeated-n-gram pass (jtk_batch_ngram_repeats): the rule header jtokkit_amd/csrc/jtk_repeat_rules.h -- run
serially through the shim tests/repeat_sim the way the call and its kernels partition a batch into groups, tiles and lanes, tiles
ascending and descending, insert order shuffled, under several table budgets -- against the plain restatement tests/repeat_ref.py
on every case of tests/repeat_cases.py and both modes: the flags and the four per-document arrays, exactly.  The case set is
checked to reach every edge it names (from the oracle's ids) and to tell the right rule from ten wrong ones, no case passes or
fails through a hash collision, and a stand-alone sanitizer build of the shim runs every case in buffers of exactly the arrays'
sizes.  No GPU."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import repeat_cases as rc
import repeat_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIM_DIR = os.path.join(ROOT, "tests", "repeat_sim")
_BUILT, _REF = {}, {}

CASES = {c.name: c for c in rc.cases()}
CASE_NAMES = (["lengths_n%d" % n for n in (1, 2, 13, 32)] + ["all_equal_n%d" % n for n in (1, 2, 13, 32)] + ["periods_n%d" % n for n in (2, 3, 13)]
              + ["same_across_docs_n2", "same_across_docs_n13", "straddle_n2", "straddle_n13", "placement_n2", "placement_n13", "top_edges_n2",
                 "top_edges_n13"] + ["empty_runs_%d" % r for r in (1, 2, 65)]
              + ["refused_special", "refused_utf8", "allow_special", "fim", "table_wrap", "table_cap_exact", "table_cap_plus2", "grouping_n2",
                 "grouping_n13"])
BIG = 1 << 40
WALKS = ((0, 0, BIG), (1, 7, rc.MIN_BUDGET), (0, 99, 4096), (1, 3, BIG))          # (tile order, shuffle, table budget in bytes)
OUTS = ("flags", "n_repeat", "n_covered", "top_count", "top_first")


def corpus_of(case):
    """The ids and statuses; a refused document keeps the tokens of its text, which the rule must not look at."""
    if case.name not in _BUILT:
        _BUILT[case.name] = rc.ids_of(case.docs, case.route, keep_refused=True)
    return _BUILT[case.name]


def ref(case, mark_first):
    """The restatement's result of a case in one mode, computed once."""
    if (case.name, mark_first) not in _REF:
        ids, status = corpus_of(case)
        _REF[case.name, mark_first] = rr.repeats(ids, status, case.n, case.seed, case.base, mark_first)
    return _REF[case.name, mark_first]


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("repeat_sim") / "librepeat_sim.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas", "-o", out,
                           os.path.join(SIM_DIR, "repeat_sim.cpp")])
    L = C.CDLL(out)
    p, i64, u64, i32, u32 = C.c_void_p, C.c_int64, C.c_uint64, C.c_int32, C.c_uint32
    for name, res, args in (("sim_rp_params_ok", C.c_int, [i32, u32]), ("sim_rp_key", u64, [u64, i32]), ("sim_rp_doc_key", u64, [u64, u64, i64]),
                            ("sim_rp_capacity", i64, [i64]), ("sim_rp_top_pack", u64, [u32, i64]), ("sim_rp_top_count", i32, [u64]),
                            ("sim_rp_top_first", i64, [u64]), ("sim_rp_max_doc_tokens", i64, []),
                            ("sim_rp_keys", C.c_int, [p, p, p, i64, u64, u64, i32, C.c_int, p]),
                            ("sim_rp_repeats", C.c_int, [p, p, p, i64, u64, u64, i32, u32, i64, C.c_int, u64, p, p, p, p, p, p])):
        getattr(L, name).restype, getattr(L, name).argtypes = res, args
    return L


def arrays(ids, status):
    """tokens, tok_off and status as the device holds them (one spare element: an address for an empty batch)."""
    tok_off = np.zeros(len(ids) + 1, dtype=np.int64)
    if ids:
        np.cumsum([len(x) for x in ids], out=tok_off[1:])
    tokens = np.array([t for x in ids for t in x] + [0], dtype=np.int32)
    return tokens, tok_off, np.array(list(status) + [0], dtype=np.int32)


def run_sim(sim, case, mark_first, order, shuffle, budget, want=(True,) * 5):
    """The shim's five outputs (guards checked; an output not asked for stays untouched) and its info."""
    ids, status = corpus_of(case)
    tokens, tok_off, st = arrays(ids, status)
    nd, nt = len(ids), int(tok_off[-1])
    outs = [np.full(nt + 1, 0x5A, dtype=np.uint8)] + [np.full(nd + 1, -7, dtype=np.int32) for _ in range(3)] + [np.full(nd + 1, -7, dtype=np.int64)]
    info = np.zeros(4, dtype=np.int64)
    got = sim.sim_rp_repeats(tokens.ctypes.data, tok_off.ctypes.data, st.ctypes.data, nd, case.seed, case.base, case.n,
                             rr.MARK_FIRST if mark_first else 0, budget, order, shuffle, *[o.ctypes.data if w else None for o, w in zip(outs, want)],
                             info.ctypes.data)
    assert got == 0, (case.name, got)
    for o, w, guard in zip(outs, want, (0x5A, -7, -7, -7, -7)):
        assert o[-1] == guard and (w or (o == guard).all())
    return [o[:-1] for o in outs], info


def ref_keys(case, wrong=None):
    """k of the n-gram that starts at every token, 0 where none does, by the restatement."""
    ids, status = corpus_of(case)
    out, at = np.zeros(sum(len(x) for x in ids), dtype=np.uint64), 0
    for x, here in zip(ids, rr.doc_ks(ids, status, case.n, case.seed, case.base, wrong)):
        for i, k in here:
            if at + i < len(out):
                out[at + i] = k
        at += len(x)
    return out


def test_header_constants_are_pinned(sim):
    assert sim.sim_rp_tile() == rc.TILE == 512 and sim.sim_rp_lane() == rc.LANE == 8 and sim.sim_rp_block_tiles() == 4
    assert rc.WG == sim.sim_rp_tile() * sim.sim_rp_block_tiles() and sim.sim_rp_max_ngram() == 32 == max(rc.NGRAMS)
    assert sim.sim_rp_start() == rr.START == 1 and sim.sim_rp_covered() == rr.COVERED == 2 and sim.sim_rp_mark_first() == rr.MARK_FIRST == 1
    assert sim.sim_rp_slot_bytes() == rr.SLOT_BYTES == 20 and sim.sim_rp_min_table_bytes() == rc.MIN_BUDGET == 1280
    assert sim.sim_rp_max_doc_tokens() == (1 << 31) - 1
    hdr = open(os.path.join(ROOT, "include", "jtokkit_amd.h")).read()
    assert "#define JTK_RP_START 1\n" in hdr and "#define JTK_RP_COVERED 2\n" in hdr and "#define JTK_REPEAT_MARK_FIRST 1u\n" in hdr
    assert "JTK_OPT_REPEAT_TABLE_BYTES = 5" in hdr


def test_case_names_are_the_case_set():
    assert list(CASES) == CASE_NAMES
    for case in CASES.values():
        assert sum(len(x) for x in corpus_of(case)[0]) <= 4600, case.name


def test_parameter_ranges_keys_capacity_and_top_word(sim):
    ok = lambda n, f=0: bool(sim.sim_rp_params_ok(n, f))
    assert ok(1) and ok(13) and ok(32) and ok(13, 1) and not ok(0) and not ok(33) and not ok(-1) and not ok(13, 2) and not ok(13, 3) and not ok(13, 1 << 31)
    import minhash_ref
    import ngram_ref
    for seed in (0, 1, rc.MAX_SEED, 0x123456789ABCDEF0):
        for n in (1, 2, 13, 32):
            key = sim.sim_rp_key(seed, n)
            assert key == rr.key_of(seed, n) == rr.mix(seed + rr.G * (n + 97))
            assert key not in {minhash_ref.key_of(seed, m) for m in range(1, 33)} | {ngram_ref.key_of(seed, m) for m in range(1, 33)}
            for base, d in ((0, 0), (5, 2), (rc.WRAP_BASE, 0), (rc.WRAP_BASE, 2), (rc.WRAP_BASE, 3), (rc.MAX_SEED, 7)):
                assert sim.sim_rp_doc_key(key, base, d) == rr.doc_key(key, base, d) == rr.mix(key + rr.G * (((base + d) % (1 << 64)) + 1))
    assert rr.doc_key(9, rc.WRAP_BASE, 3) == rr.doc_key(9, 0, 0)                                   # (2^64 - 3 + 3 wraps to 0)
    for m, cap in ((0, 64), (32, 64), (33, 128), (64, 128), (65, 256), (1 << 20, 1 << 21), ((1 << 20) + 1, 1 << 22)):
        assert sim.sim_rp_capacity(m) == rr.capacity(m) == cap, m
    # the packed top word: the larger count wins, then the smaller position; 0 = no n-gram
    pack = sim.sim_rp_top_pack
    assert pack(3, 9) > pack(2, 0) and pack(2, 4) > pack(2, 5) and pack(1, (1 << 31) - 1) > 0
    for count, rel in ((1, 0), (2, 5), (65, 511), ((1 << 31) - 1, (1 << 31) - 1)):
        assert sim.sim_rp_top_count(pack(count, rel)) == count and sim.sim_rp_top_first(pack(count, rel)) == rel
    assert sim.sim_rp_top_count(0) == 0 and sim.sim_rp_top_first(0) == -1


def test_reference_on_hand_computed_values():
    assert rr.mix(0) == 0 and rr.mix(rr.G) == 0xE220A8397B1DCDAF            # splitmix64's first output from state 0
    r = rr.repeats([[1, 2, 1, 2, 1, 2]], [0], 2)
    assert r.flags.tolist() == [0, 0, 3, 3, 3, 2]
    assert (r.n_repeat[0], r.n_covered[0], r.top_count[0], r.top_first[0]) == (3, 4, 3, 0)
    r = rr.repeats([[1, 2, 1, 2, 1, 2]], [0], 2, mark_first=True)
    assert r.flags.tolist() == [3, 3, 3, 3, 3, 2]
    assert (r.n_repeat[0], r.n_covered[0], r.top_count[0], r.top_first[0]) == (5, 6, 3, 0)
    r = rr.repeats([[7, 8, 9, 7, 8, 9]], [0], 2)
    assert (r.top_count[0], r.top_first[0]) == (2, 0)                       # (7, 8) and (8, 9) tie: the earlier one
    for mark in (False, True):
        r = rr.repeats([[1, 2, 3], [1, 2, 3]], [0, 0], 2, mark_first=mark)
        assert not r.flags.any() and r.n_repeat.tolist() == [0, 0] and r.top_count.tolist() == [1, 1] and r.top_first.tolist() == [0, 0]
    r = rr.repeats([[4, 4, 4], [4, 4, 4, 4], []], [0, -2, 0], 1)
    assert r.flags.tolist() == [0, 3, 3, 0, 0, 0, 0] and r.top_count.tolist() == [3, 0, 0] and r.top_first.tolist() == [0, -1, -1]
    assert rr.groups([5, 9, 0, 100, 0, 0, 100], [0] * 7, 2, 1280) == [(0, 3, 12), (3, 4, 99), (4, 6, 0), (6, 7, 99)]
    assert rr.groups([40, 40], [0, -2], 2, 1280) == [(0, 1, 39)] + [(1, 2, 0)] and rr.groups([10, 10], [0, -2], 2, 1280) == [(0, 2, 9)]


@pytest.mark.parametrize("name", CASE_NAMES)
def test_rule_header_equals_the_restatement(sim, name):
    case = CASES[name]
    groups_seen = set()
    ids, status = corpus_of(case)
    tokens, tok_off, st = arrays(ids, status)
    ks = np.zeros(len(tokens), dtype=np.uint64)
    assert sim.sim_rp_keys(tokens.ctypes.data, tok_off.ctypes.data, st.ctypes.data, len(ids), case.seed, case.base, case.n, 1, ks.ctypes.data) == 0
    assert np.array_equal(ks[:-1], ref_keys(case)), name                     # every k: the document's key, doc_index_base included
    for mark_first in (False, True):
        exp = ref(case, mark_first)
        for order, shuffle, budget in WALKS:
            got, info = run_sim(sim, case, mark_first, order, shuffle, budget)
            for g, out in zip(got, OUTS):
                e = getattr(exp, out)
                assert np.array_equal(g, e), (name, mark_first, order, shuffle, budget, out, np.flatnonzero(g != e)[:10])
            ids, status = corpus_of(case)
            assert info[0] == len(rr.groups([len(x) for x in ids], status, case.n, budget)) and info[2] <= info[3]
            assert info[3] == sum(rr.n_ngrams(len(x), case.n) for x, st in zip(ids, status) if st >= 0)
            groups_seen.add(int(info[0]))
        # outputs that are not asked for are not written
        for want in ((True, False, False, False, False), (False, True, False, False, False), (False, False, True, False, True),
                     (False, False, False, True, False), (False, False, False, False, False)):
            got, _ = run_sim(sim, case, mark_first, 0, 0, rc.MIN_BUDGET, want)
            for g, out, w in zip(got, OUTS, want):
                assert not w or np.array_equal(g, getattr(exp, out)), (name, mark_first, want, out)
    if name.startswith("grouping"):
        assert len(groups_seen) >= 2 and 1 in groups_seen and max(groups_seen) >= 7      # (one group, and many)


def test_lane_run_merge_spares_atomics(sim):
    """A page of one token repeated: pass 1 issues one pair of atomics per lane, not one per n-gram."""
    _, info = run_sim(sim, CASES["all_equal_n1"], False, 0, 0, BIG)
    assert info[3] > 100 and info[2] < info[3] // 3


def test_case_set_reaches_the_edges():
    reached = set()
    for case in CASES.values():
        ids, status = corpus_of(case)
        reached |= rc.edges_reached(case, ids, status, ref(case, False), ref(case, True))
    assert rc.all_edges() - reached == set()
    assert corpus_of(CASES["refused_special"])[1] == [0, -2, 0, 0] and corpus_of(CASES["refused_utf8"])[1] == [0, -6, 0, 0]
    assert 100257 in corpus_of(CASES["allow_special"])[0][0] and any(set(rc.mc.FIM_IDS) <= set(x) for x in corpus_of(CASES["fim"])[0])
    big = corpus_of(CASES["placement_n13"])[0]
    assert [len(x) for x in big] == [1900, 2400, 20]


def test_case_set_tells_the_right_rule_from_wrong_ones():
    """Each wrong rule changes some case's flags or per-document results, in one mode or the other -- or, for the rule that leaves
    doc_index_base out of the documents' keys, which by design changes no result but through a collision, the k themselves (which
    test_rule_header_equals_the_restatement pins on the header)."""
    for wrong in rr.WRONG_RULES:
        changed = []
        for name in CASE_NAMES:
            case = CASES[name]
            ids, status = corpus_of(case)
            for mark_first in (False, True):
                exp = ref(case, mark_first)
                got = rr.repeats(ids, status, case.n, case.seed, case.base, mark_first, wrong=wrong, tile=rc.TILE)
                if not all(np.array_equal(getattr(got, out), getattr(exp, out)) for out in OUTS):
                    changed.append((name, mark_first))
            if wrong in ("base_ignored", "no_doc_salt") and not np.array_equal(ref_keys(case, wrong), ref_keys(case)):
                changed.append((name, "k"))
        if wrong != "base_ignored":
            assert any(mode != "k" for _, mode in changed), wrong
        assert changed, wrong
    assert len(rr.WRONG_RULES) == 10


def test_no_case_depends_on_a_hash_collision():
    """Over all (document, n-gram) pairs of a case the distinct id tuples per document and the distinct k are as many -- inside and
    across documents: the one-table kernels see what the per-document rule sees -- and no k is G."""
    for case in CASES.values():
        ids, status = corpus_of(case)
        ks = rr.doc_ks(ids, status, case.n, case.seed, case.base)
        pairs = set()
        for d, (here, grams) in enumerate(zip(ks, rr.starts(ids, status, case.n))):
            assert len(here) == len(grams)
            pairs |= {(d, tuple(g), k) for (_, k), (_, g) in zip(here, grams)}
        assert len({(d, g) for d, g, _ in pairs}) == len({k for _, _, k in pairs}) == len(pairs), case.name
        assert rr.G not in {k for _, _, k in pairs}


def test_sanitizer_build_runs_every_case_in_exact_buffers(tmp_path):
    exe = str(tmp_path / "repeat_sim_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, os.path.join(SIM_DIR, "repeat_sim_main.cpp")])
    cases, results = str(tmp_path / "cases.bin"), str(tmp_path / "results.bin")
    records = []
    for i, name in enumerate(CASE_NAMES):
        for mark_first in (False, True):
            records.append((CASES[name], mark_first, (rc.MIN_BUDGET, 4096, BIG)[(i + mark_first) % 3], (i + mark_first) & 1))
    with open(cases, "wb") as f:
        for case, mark_first, budget, order in records:
            ids, status = corpus_of(case)
            tokens, tok_off, st = arrays(ids, status)
            f.write(struct.pack("<2q2Q4q", len(ids), len(tokens) - 1, case.seed, case.base, case.n, int(mark_first), budget, order))
            f.write(tok_off.astype("<i8").tobytes())
            f.write(st[:-1].astype("<i4").tobytes())
            f.write(tokens[:-1].astype("<i4").tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe, cases, results], env=env, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-4000:]
    assert p.stdout.strip() == "%d cases" % len(records)
    raw = open(results, "rb").read()
    at = 0
    for case, mark_first, budget, order in records:
        exp = ref(case, mark_first)
        for out, dt in zip(OUTS, ("u1", "<i4", "<i4", "<i4", "<i8")):
            e = getattr(exp, out)
            got = np.frombuffer(raw, dtype=dt, count=e.size, offset=at)
            at += got.nbytes
            assert np.array_equal(got, e.ravel()), (case.name, mark_first, out)
    assert at == len(raw)


def test_abi_refuses_what_needs_no_device():
    """What the entry point refuses before it touches a device, the parameter struct's layout and the Python surface."""
    so = os.path.join(ROOT, "jtokkit_amd", "libjtokkit_amd.so")
    if not os.path.exists(so):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "jtokkit_amd", "csrc")])
    from jtokkit_amd import _native as N
    L = N.lib()
    assert C.sizeof(N.RepeatParamsStruct) == 24 and N.RepeatParamsStruct.ngram.offset == 16 and N.RepeatParamsStruct.flags.offset == 20
    assert (N.JTK_RP_START, N.JTK_RP_COVERED, N.JTK_REPEAT_MARK_FIRST, N.JTK_OPT_REPEAT_TABLE_BYTES, N.JTK_RP_MIN_TABLE_BYTES) == (1, 2, 1, 5, 1280)
    p = N.RepeatParamsStruct(0, 0, 13, 0)
    assert L.jtk_batch_ngram_repeats(None, C.byref(p), None, None, None, None, None, None) == N.JTK_ERR_INVALID_ARGUMENT and N.last_error()
    assert L.jtk_batch_ngram_repeats(None, None, None, None, None, None, None, None) == N.JTK_ERR_INVALID_ARGUMENT
    assert L.jtk_batch_set_option(None, N.JTK_OPT_REPEAT_TABLE_BYTES, 1 << 20) == N.JTK_ERR_INVALID_ARGUMENT
    import jtokkit_amd
    assert callable(jtokkit_amd.encoding.Batch.ngram_repeats)
    for name in ("ngram_repeats_batch", "ngram_repeats_batch_device", "repetition_signals"):
        assert callable(getattr(jtokkit_amd.HipEncoding, name))
