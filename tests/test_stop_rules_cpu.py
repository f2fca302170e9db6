"""CPU tier of the stop strings (jtk_batch_decode_find_stops): the rule header jtokkit_amd/csrc/jtk_stop_rules.h -- run serially
through the shim tests/stop_sim the way the kernels partition the work -- against the plain restatement tests/stop_ref.py on
every case of tests/stop_cases.py.  stop_pos, stop_which, hold and stop_col are compared exactly; the case set must reach its
edges, so that the GPU tier cannot pass by missing one; and a stand-alone sanitizer build of the shim runs every case in
buffers of exactly the documented readable size.  No GPU."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import stop_cases as sc
import stop_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIM_DIR = os.path.join(ROOT, "tests", "stop_sim")
CASES = sc.cases()
_REF = {}


def ref(case):
    """The reference's result for a case, computed once."""
    if case.name not in _REF:
        _REF[case.name] = sr.find_stops(case.out, case.byte_off, case.strings, case.frm, case.cell_byte)
    return _REF[case.name]


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("stop_sim") / "libstop_sim.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas", "-o", out,
                           os.path.join(SIM_DIR, "stop_sim.cpp")])
    L = C.CDLL(out)
    L.sim_find_stops.restype = C.c_int
    L.sim_find_stops.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                 C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return L


def blob_of(strings):
    str_off = np.zeros(len(strings) + 1, dtype=np.uint32)
    if strings:
        np.cumsum([len(s) for s in strings], out=str_off[1:])
    return np.frombuffer(b"".join(strings), dtype=np.uint8), str_off


def sim_find(sim, out, byte_off, strings, frm=None, cell_byte=None, pad=0x61):
    n = len(byte_off) - 1
    size = (len(out) + 15) // 16 * 16 + 16
    raw = np.full(size + 16, pad, dtype=np.uint8)                      # (bytes past the end must not count)
    start = (-raw.ctypes.data) % 16
    view = raw[start:start + size]
    view[:len(out)] = np.frombuffer(out, dtype=np.uint8)
    blob, str_off = blob_of(strings)
    frm = None if frm is None else np.ascontiguousarray(frm, dtype=np.int64)
    width = 0 if cell_byte is None else cell_byte.shape[1]
    cb = None if cell_byte is None else np.ascontiguousarray(cell_byte)
    pos, col = np.full(max(n, 1), -7, dtype=np.int64), np.full(max(n, 1), -7, dtype=np.int64)
    which, hold = np.full(max(n, 1), -7, dtype=np.int32), np.full(max(n, 1), -7, dtype=np.int32)
    rc = sim.sim_find_stops(view.ctypes.data, len(out), byte_off.ctypes.data, n, blob.ctypes.data if len(blob) else None, str_off.ctypes.data,
                            len(strings), None if frm is None else frm.ctypes.data, None if cb is None or not cb.size else cb.ctypes.data,
                            width, pos.ctypes.data, which.ctypes.data, hold.ctypes.data, col.ctypes.data)
    if rc != 0:
        return None
    return pos[:n], which[:n], hold[:n], col[:n]


def same(got, exp):
    return all(np.array_equal(g, e) for g, e in zip(got, exp))


def test_the_shim_uses_the_tile_the_cases_are_built_for(sim):
    assert sim.sim_stop_tile() == sc.TILE and sim.sim_stop_lane() == sc.LANE
    assert sim.sim_stop_max_strings() == sc.MAX_STRINGS and sim.sim_stop_max_bytes() == sc.MAX_BYTES


@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_rule_header_finds_what_the_reference_finds(sim, name):
    case = {c.name: c for c in CASES}[name]
    exp = ref(case)
    got = sim_find(sim, case.out, case.byte_off, case.strings, case.frm, case.cell_byte if case.width else None)
    for key, g, e in zip(("stop_pos", "stop_which", "hold", "stop_col"), got, exp):
        assert np.array_equal(g, e), (name, key, np.flatnonzero(g != e)[:10], g[g != e][:10], e[g != e][:10])
    # the same text as one flat list per row: no cells, no columns
    got = sim_find(sim, case.out, case.byte_off, case.strings, case.frm)
    assert same(got[:3], exp[:3]) and (got[3] == -1).all()
    # and without `from`
    if case.frm is not None:
        exp0 = sr.find_stops(case.out, case.byte_off, case.strings)
        assert same(sim_find(sim, case.out, case.byte_off, case.strings)[:3], exp0[:3])


def test_bytes_behind_the_text_never_match(sim):
    """The readable bytes past the end of the output, whatever they hold, complete no match and no held-back tail."""
    out, off = b"..ab", np.array([0, 4], dtype=np.int64)
    for pad in (0x63, 0x00, 0x61):
        pos, which, hold, _ = sim_find(sim, out, off, [b"abc", b"bc"], pad=pad)
        assert (pos[0], which[0], hold[0]) == (4, -1, 2)


def test_rule_header_refuses_what_the_interface_refuses(sim):
    out, off = b"abc", np.array([0, 3], dtype=np.int64)
    assert sim_find(sim, out, off, [b"a"] * 17) is None
    assert sim_find(sim, out, off, [b"a", b""]) is None
    assert sim_find(sim, out, off, [b"a" * 65]) is None
    assert sim_find(sim, out, off, [b"a" * 64] * 16) is not None


def test_reference_on_hand_computed_rows():
    """The restatement itself, on rows small enough to check by eye."""
    out = b"xxSTOPyy" + b"abST" + b"OP"
    off = np.array([0, 8, 12, 14], dtype=np.int64)
    pos, which, hold, col = sr.find_stops(out, off, [b"STOP", b"yy"])
    assert pos.tolist() == [2, 12, 14] and which.tolist() == [0, -1, -1] and hold.tolist() == [0, 2, 0] and col.tolist() == [-1, -1, -1]
    pos, which, hold, _ = sr.find_stops(out, off, [b"STOP", b"yy"], [3, 0, 0])
    assert pos.tolist() == [6, 12, 14] and which.tolist() == [1, -1, -1]
    cells = np.array([[0, 2, 2, 6, 8]], dtype=np.int64)
    assert sr.find_stops(out[:8], off[:2], [b"TOP"], None, cells)[3].tolist() == [2]
    assert sr.cut_rows(out, off, *sr.find_stops(out, off, [b"STOP"])[:2], [b"STOP"]) == [b"xx", b"abST", b"OP"]
    assert sr.cut_rows(out, off, *sr.find_stops(out, off, [b"STOP"])[:2], [b"STOP"], True) == [b"xxSTOP", b"abST", b"OP"]


def test_case_set_reaches_the_edges():
    reached = set()
    for case in CASES:
        reached |= sc.edges_reached(case, ref(case))
    assert sc.ALL_EDGES - reached == set()
    total = [len(c.out) for c in CASES]
    assert max(total) >= 3 * sc.TILE and max(total) <= 4 * sc.TILE and sum(total) <= 16 * sc.TILE     # (tests that take seconds)


def test_sanitizer_build_runs_every_case_in_exact_buffers(tmp_path):
    exe = str(tmp_path / "stop_sim_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, os.path.join(SIM_DIR, "stop_sim_main.cpp")])
    cases, results = str(tmp_path / "cases.bin"), str(tmp_path / "results.bin")
    with open(cases, "wb") as f:
        for c in CASES:
            blob, str_off = blob_of(c.strings)
            f.write(struct.pack("<5q", len(c.rows), len(c.out), len(c.strings), int(c.frm is not None), c.width))
            f.write(c.byte_off.astype("<i8").tobytes())
            f.write(c.out)
            f.write(str_off.astype("<u4").tobytes())
            f.write(blob.tobytes())
            if c.frm is not None:
                f.write(c.from_array().astype("<i8").tobytes())
            f.write(c.cell_byte.astype("<i8").tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe, cases, results], env=env, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-4000:]
    assert p.stdout.strip() == "%d cases" % len(CASES)
    raw = open(results, "rb").read()
    at = 0
    for c in CASES:
        n = len(c.rows)
        exp = ref(c)
        for e, dt in zip(exp, ("<i8", "<i4", "<i4", "<i8")):
            got = np.frombuffer(raw, dtype=dt, count=n, offset=at)
            at += got.nbytes
            if c.width or e is not exp[3]:
                assert np.array_equal(got, e), c.name
            else:
                assert (got == -1).all(), c.name
    assert at == len(raw)
