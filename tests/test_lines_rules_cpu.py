"""CPU tier of the line / paragraph pass (jtk_batch_line_units, jtk_batch_line_repeats): the rule header
jtokkit_amd/csrc/jtk_lines_rules.h -- run serially through the shim tests/lines_sim the way the kernels partition the text into
granules and tiles (summaries, scan, write pass, then the groups), tiles ascending and descending, pass-1 order shuffled, under
several table budgets -- against the plain restatement tests/lines_ref.py on every case of tests/lines_cases.py, both units, both
TRIM values and both modes: every output, exactly, and every unit's k.  The case set is checked to reach every edge it names and to
tell the right rule from ten wrong ones, no case passes or fails through a hash collision, and a stand-alone sanitizer build of the
shim runs every case in buffers of exactly the arrays' sizes.  No GPU."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import lines_cases as lc
import lines_ref as lr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIM_DIR = os.path.join(ROOT, "tests", "lines_sim")
CASES = {c.name: c for c in lc.cases()}
CASE_NAMES = ["empties", "crlf", "trim_equal", "blank_between", "newline_runs", "prefix_nul_ends", "tile_edges", "long_unit", "scan_steps",
              "doc_edges", "utf8_edges", "counts", "refused_utf8", "refused_special", "table_cap_64", "table_cap_128", "grouping", "odd_offsets"]
BIG = 1 << 40
WALKS = ((0, 0, BIG), (1, 7, lc.MIN_BUDGET), (0, 99, 4096), (1, 3, BIG))          # (tile order, shuffle, table budget in bytes)
MODES = [(unit, trim, mark) for unit, trim in lc.COMBOS for mark in (False, True)]
DTYPES = dict(unit_begin=np.int64, unit_end=np.int64, unit_flags=np.uint8, unit_off=np.int64, n_dup=np.int32, dup_bytes=np.int64,
              dup_chars=np.int64, unit_bytes=np.int64, unit_chars=np.int64, doc_chars=np.int64, top_count=np.int32, top_first=np.int64)
_REF = {}


def ref(case, unit, trim, mark, wrong=None):
    """The restatement's result of a case in one mode, computed once."""
    key = (case.name, unit, trim, mark, wrong)
    if key not in _REF:
        _REF[key] = lr.repeats(case.docs, lc.status_of(case), unit, trim, mark, case.seed, case.base, wrong)
    return _REF[key]


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("lines_sim") / "liblines_sim.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas", "-o", out,
                           os.path.join(SIM_DIR, "lines_sim.cpp")])
    L = C.CDLL(out)
    p, i64, u64, i32, u32 = C.c_void_p, C.c_int64, C.c_uint64, C.c_int32, C.c_uint32
    for name, res, args in (("sim_ln_params_ok", C.c_int, [i32, u32]), ("sim_ln_key", u64, [u64, i32]), ("sim_ln_pow", u64, [u64]),
                            ("sim_ln_then", u32, [u32, u32]), ("sim_ln_apply", u32, [u32, u32]), ("sim_ln_max_doc_units", i64, []),
                            ("sim_ln_repeats", C.c_int, [p, i64, p, p, i64, u64, u64, i32, u32, i64, C.c_int, u64] + [p] * 14)):
        getattr(L, name).restype, getattr(L, name).argtypes = res, args
    return L


def arrays(case):
    """text, doc_off and status as the device holds them (one spare element: an address for an empty batch)."""
    docs = case.docs
    doc_off = np.zeros(len(docs) + 1, dtype=np.int64)
    if docs:
        np.cumsum([len(x) for x in docs], out=doc_off[1:])
    text = np.frombuffer(b"".join(docs) + b"\x00", dtype=np.uint8)
    return text, doc_off, np.array(lc.status_of(case) + [0], dtype=np.int32)


def run_sim(sim, case, unit, trim, mark, order, shuffle, budget, want=None):
    """The shim's twelve outputs by name (guards checked; an output not asked for stays untouched), the k per unit and the info."""
    text, doc_off, st = arrays(case)
    nd, nb = len(case.docs), int(doc_off[-1])
    nu = len(ref(case, unit, trim, mark).unit_begin)
    size = dict(unit_begin=nu, unit_end=nu, unit_flags=nu, unit_off=nd + 1)
    outs = {name: np.full(size.get(name, nd) + 1, 0x5A if dt is np.uint8 else -7, dtype=dt) for name, dt in DTYPES.items()}
    ks, info = np.zeros(nu + 1, dtype=np.uint64), np.zeros(4, dtype=np.int64)
    flags = (lr.MARK_FIRST if mark else 0) | (lr.TRIM if trim else 0)
    got = sim.sim_ln_repeats(text.ctypes.data, nb, doc_off.ctypes.data, st.ctypes.data, nd, case.seed, case.base, unit, flags, budget, order, shuffle,
                             *[outs[name].ctypes.data if want is None or name in want else None for name in lr.OUTS], ks.ctypes.data, info.ctypes.data)
    assert got == 0 and info[3] == nu, (case.name, got, info[3], nu)
    for name, o in outs.items():
        guard = 0x5A if o.dtype == np.uint8 else -7
        assert o[-1] == guard and (want is None or name in want or (o == guard).all()), (case.name, name)
    return {name: o[:-1] for name, o in outs.items()}, ks[:-1], info


def test_header_constants_are_pinned(sim):
    assert (sim.sim_ln_granule(), sim.sim_ln_wave_bytes(), sim.sim_ln_tile(), sim.sim_ln_scan_step()) == (lc.GRANULE, lc.WAVE, lc.TILE, lc.STEP) == (16, 1024, 4096, 1024)
    assert sim.sim_ln_key_c() == lr.KEY_C == 161 and sim.sim_ln_unit_bytes() == 48 and sim.sim_ln_max_doc_units() == (1 << 31) - 1
    hdr = open(os.path.join(ROOT, "include", "jtokkit_amd.h")).read()
    for line in ("#define JTK_LINES_LINE 0\n", "#define JTK_LINES_PARAGRAPH 1\n", "#define JTK_LINES_MARK_FIRST 1u\n", "#define JTK_LINES_TRIM 2u\n"):
        assert line in hdr
    assert "int jtk_batch_line_units(" in hdr and "int jtk_batch_line_repeats(" in hdr


def test_case_names_are_the_case_set():
    assert list(CASES) == CASE_NAMES


def test_parameters_keys_powers_and_the_carry(sim):
    ok = lambda u, f=0: bool(sim.sim_ln_params_ok(u, f))
    assert ok(0) and ok(1) and ok(0, 1) and ok(1, 2) and ok(1, 3) and not ok(2) and not ok(-1) and not ok(0, 4) and not ok(0, 8) and not ok(1, 1 << 31)
    import minhash_ref
    import ngram_ref
    import repeat_ref
    for seed in (0, 1, lc.MAX_SEED, 0x123456789ABCDEF0):
        others = set()
        for m in range(1, 33):
            others |= {minhash_ref.key_of(seed, m), ngram_ref.key_of(seed, m), repeat_ref.key_of(seed, m)}
        for unit in (0, 1):
            assert sim.sim_ln_key(seed, unit) == lr.key_of(seed, unit) == lr.mix(seed + lr.G * (unit + 161)) and lr.key_of(seed, unit) not in others
    for e in (0, 1, 2, 16, 1024, 4096, 4096 * 1024, (1 << 40) + 12345, (1 << 64) - 1):
        assert sim.sim_ln_pow(e) == pow(lr.G, e, 1 << 64)
    # the carry: an ink byte fixes 0, an edge fixes NOINK (3), a newline adds 1 up to 2; `then` composes as functions do
    INK, EDGE, NL, ID = 16, 16 | (3 << 2), 1, 0
    ts = [ID, NL, 2, INK, EDGE, 16 | (1 << 2), 16 | (2 << 2)]
    for a in ts:
        for b in ts:
            for s in range(4):
                assert sim.sim_ln_apply(sim.sim_ln_then(a, b), s) == sim.sim_ln_apply(b, sim.sim_ln_apply(a, s)), (a, b, s)
            for c in ts:
                assert sim.sim_ln_then(sim.sim_ln_then(a, b), c) == sim.sim_ln_then(a, sim.sim_ln_then(b, c))
    assert [sim.sim_ln_apply(NL, s) for s in range(4)] == [1, 2, 2, 3] and [sim.sim_ln_apply(INK, s) for s in range(4)] == [0] * 4


def test_reference_on_hand_computed_values():
    assert lr.mix(0) == 0 and lr.mix(lr.G) == 0xE220A8397B1DCDAF            # splitmix64's first output from state 0
    assert lr.horner(b"\x00") == 1 and lr.horner(b"\x00\x00") == (lr.G + 1) & lr.M64 and lr.horner(b"ab") == (98 * lr.G + 99) & lr.M64
    assert lr.units_of(b"\n\na\nb\n\nc \n \nd\n\n", lr.LINE, False) == [(2, 3), (4, 5), (7, 9), (10, 11), (12, 13)]
    assert lr.units_of(b"\n\na\nb\n\nc \n \nd\n\n", lr.LINE, True) == [(2, 3), (4, 5), (7, 8), (12, 13)]
    assert lr.units_of(b"\n\na\nb\n\nc \n \nd\n\n", lr.PARAGRAPH, False) == [(2, 5), (7, 13)]
    assert lr.units_of(b"\n\na\nb\n\nc \n \nd\n\n", lr.PARAGRAPH, True) == [(2, 5), (7, 8), (12, 13)]
    assert lr.units_of(b" a \r\n", lr.LINE, True) == [(1, 2)] and lr.units_of(b" a \r\n", lr.LINE, False) == [(0, 4)]
    import re
    for doc in (b"a\n\nb\nc\n\n\nd", b"\n\nx\ny\n", b"one"):                 # what the rule claims to match, without TRIM
        s = doc.strip(b"\n")
        assert [doc[b:e] for b, e in lr.units_of(doc, lr.LINE, False)] == re.split(b"\n+", s)
        assert [doc[b:e] for b, e in lr.units_of(doc, lr.PARAGRAPH, False)] == re.split(b"\n{2,}", s)
    r = lr.repeats([b"x\ny\nx\n\xc3\xa9\nx", b"x\nx", b"x\nx"], [0, -2, 0], lr.LINE)
    assert r.unit_flags.tolist() == [0, 0, 1, 0, 1, 0, 1] and r.unit_off.tolist() == [0, 5, 5, 7] and r.n_dup.tolist() == [2, 0, 1]
    assert r.unit_begin.tolist() == [0, 2, 4, 6, 9, 13, 15] and r.unit_end.tolist() == [1, 3, 5, 8, 10, 14, 16]
    assert r.dup_bytes.tolist() == [2, 0, 1] and r.unit_bytes.tolist() == [6, 0, 2] and r.unit_chars.tolist() == [5, 0, 2] and r.doc_chars.tolist() == [9, 3, 3]
    assert r.top_count.tolist() == [3, 0, 2] and r.top_first.tolist() == [0, -1, 0]
    r = lr.repeats([b"x\ny\nx"], [0], lr.LINE, mark_first=True)
    assert r.unit_flags.tolist() == [1, 0, 1]
    assert lr.groups([5, 9, 0, 100, 0, 0, 100], 1280) == [(0, 3, 14), (3, 4, 100), (4, 6, 0), (6, 7, 100)]


@pytest.mark.parametrize("name", CASE_NAMES)
def test_rule_header_equals_the_restatement(sim, name):
    case = CASES[name]
    groups_seen = set()
    walks = WALKS if name != "scan_steps" else WALKS[:2]
    for unit, trim, mark in (MODES if name != "scan_steps" else (MODES[0], MODES[3], MODES[6])):      # (8 MB of text: three of the modes)
        exp = ref(case, unit, trim, mark)
        exp_k = np.array([k for ks in exp.ks for k in ks], dtype=np.uint64)
        for order, shuffle, budget in walks:
            got, ks, info = run_sim(sim, case, unit, trim, mark, order, shuffle, budget)
            for out in lr.OUTS:
                g, e = got[out], getattr(exp, out)
                assert np.array_equal(g, e), (name, unit, trim, mark, order, shuffle, budget, out, np.flatnonzero(g != e)[:10] if g.shape == e.shape else (g.shape, e.shape))
            assert np.array_equal(ks, exp_k), (name, unit, trim, mark)
            assert info[0] == len(lr.groups(np.diff(exp.unit_off).tolist(), budget))
            groups_seen.add(int(info[0]))
        if name == "scan_steps":
            continue
        # outputs that are not asked for are not written
        for want in (("unit_flags",), ("unit_begin", "unit_end"), ("unit_off", "doc_chars"), ("n_dup", "dup_chars", "top_first"), ("top_count",),
                     ("dup_bytes", "unit_bytes", "unit_chars"), ()):
            got, _, _ = run_sim(sim, case, unit, trim, mark, 0, 0, lc.MIN_BUDGET, want)
            for out in want:
                assert np.array_equal(got[out], getattr(exp, out)), (name, unit, trim, mark, want, out)
    if name == "grouping":
        assert len(groups_seen) >= 2 and 1 in groups_seen and max(groups_seen) >= 7


def test_table_probe_wraps_in_the_shim(sim):
    for name, cap in (("table_cap_64", 64), ("table_cap_128", 128)):
        _, _, info = run_sim(sim, CASES[name], lr.LINE, False, False, 0, 0, BIG)
        assert info[1] == (32 if cap == 64 else 33) and lr.capacity(int(info[1])) == cap and info[2] >= 1


def test_case_set_reaches_the_edges():
    reached = set()
    for case in CASES.values():
        reached |= lc.edges_reached(case, {mode: ref(case, *mode) for mode in MODES})
    assert lc.all_edges() - reached == set()
    assert lc.status_of(CASES["refused_special"]) == [0, -2, 0, -2] and lc.status_of(CASES["refused_utf8"]) == [0, -6, 0, -6]


def test_case_set_tells_the_right_rule_from_wrong_ones():
    """Each wrong rule changes some output of some case, in some mode."""
    for wrong in lr.WRONG_RULES:
        changed = []
        for name in CASE_NAMES:
            if name == "scan_steps":
                continue
            case = CASES[name]
            for mode in MODES:
                exp, got = ref(case, *mode), ref(case, *mode, wrong=wrong)
                if not all(np.array_equal(getattr(got, out), getattr(exp, out)) for out in lr.OUTS):
                    changed.append((name, mode))
        assert changed, wrong
    assert len(lr.WRONG_RULES) == 10


def test_no_case_depends_on_a_hash_collision():
    """Over all (document, unit bytes) pairs of a case, in every mode, the distinct pairs and the distinct k are as many -- inside
    and across documents: the one-table kernels see what the per-document rule sees -- and no k is G."""
    for case in CASES.values():
        text = b"".join(case.docs)
        for unit, trim in lc.COMBOS:
            r = ref(case, unit, trim, False)
            pairs = set()
            for d, ks in enumerate(r.ks):
                lo = int(r.unit_off[d])
                pairs |= {(d, text[r.unit_begin[lo + i]:r.unit_end[lo + i]], k) for i, k in enumerate(ks)}
            assert len({(d, x) for d, x, _ in pairs}) == len({k for _, _, k in pairs}) == len(pairs), case.name
            assert lr.G not in {k for _, _, k in pairs}


def test_sanitizer_build_runs_every_case_in_exact_buffers(tmp_path):
    exe = str(tmp_path / "lines_sim_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, os.path.join(SIM_DIR, "lines_sim_main.cpp")])
    cases, results = str(tmp_path / "cases.bin"), str(tmp_path / "results.bin")
    records = []
    for i, name in enumerate(CASE_NAMES):
        for j, mode in enumerate(MODES):
            if name == "scan_steps" and j != 7:
                continue
            records.append((CASES[name], mode, (lc.MIN_BUDGET, 4096, BIG)[(i + j) % 3], (i + j) & 1))
    with open(cases, "wb") as f:
        for case, (unit, trim, mark), budget, order in records:
            text, doc_off, st = arrays(case)
            flags = (lr.MARK_FIRST if mark else 0) | (lr.TRIM if trim else 0)
            f.write(struct.pack("<2q2Q5q", len(case.docs), len(text) - 1, case.seed, case.base, unit, flags, budget, order,
                                len(ref(case, unit, trim, mark).unit_begin)))
            f.write(doc_off.astype("<i8").tobytes())
            f.write(st[:-1].astype("<i4").tobytes())
            f.write(text[:-1].tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe, cases, results], env=env, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-4000:]
    assert p.stdout.strip() == "%d cases" % len(records)
    raw = open(results, "rb").read()
    at = 0
    for case, mode, budget, order in records:
        exp = ref(case, *mode)
        for out in lr.OUTS:
            e = getattr(exp, out)
            got = np.frombuffer(raw, dtype=np.dtype(DTYPES[out]).newbyteorder("<"), count=e.size, offset=at)
            at += got.nbytes
            assert np.array_equal(got, e.ravel()), (case.name, mode, out)
    assert at == len(raw)


def test_abi_refuses_what_needs_no_device():
    """What the entry points refuse before they touch a device, the structs' layout and the Python surface."""
    so = os.path.join(ROOT, "jtokkit_amd", "libjtokkit_amd.so")
    if not os.path.exists(so):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "jtokkit_amd", "csrc")])
    from jtokkit_amd import _native as N
    L = N.lib()
    assert C.sizeof(N.LinesParamsStruct) == 24 and N.LinesParamsStruct.unit.offset == 16 and N.LinesParamsStruct.flags.offset == 20
    assert C.sizeof(N.LinesOutStruct) == 12 * 8 and N.LinesOutStruct.top_first.offset == 88 and N.LinesOutStruct.n_dup.offset == 32
    assert (N.JTK_LINES_LINE, N.JTK_LINES_PARAGRAPH, N.JTK_LINES_MARK_FIRST, N.JTK_LINES_TRIM) == (0, 1, 1, 2)
    p, o, n = N.LinesParamsStruct(0, 0, 0, 0), N.LinesOutStruct(), C.c_int64(5)
    assert L.jtk_batch_line_units(None, C.byref(p), None, C.byref(n)) == N.JTK_ERR_INVALID_ARGUMENT and N.last_error() and n.value == 0
    assert L.jtk_batch_line_units(None, C.byref(p), None, None) == N.JTK_ERR_INVALID_ARGUMENT
    assert L.jtk_batch_line_repeats(None, C.byref(p), C.byref(o), None) == N.JTK_ERR_INVALID_ARGUMENT
    assert L.jtk_batch_line_repeats(None, None, None, None) == N.JTK_ERR_INVALID_ARGUMENT
    import jtokkit_amd
    assert callable(jtokkit_amd.encoding.Batch.line_units) and callable(jtokkit_amd.encoding.Batch.line_repeats)
    for name in ("line_repeats_batch", "line_repeats_batch_device", "repetition_signals"):
        assert callable(getattr(jtokkit_amd.HipEncoding, name))
