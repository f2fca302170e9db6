"""CPU tier of the id-matrix decode: the rule header jtokkit_amd/csrc/jtk_decode_rows_rules.h, run serially through the shim
tests/decode_rows_sim, against the plain reference tests/decode_rows_ref.py on every case of tests/decode_rows_cases.py -- bytes,
byte_off, status, cell_byte and the first stop column, all exact, for 64-bit cells and (where the values fit) 32-bit cells, with
and without a row stride; a matrix without options equals the flat reference and the CPU oracle on the same lists; and the
conditions that the case set must meet to reach the edges of jtk_decode_rows.hip, so that the GPU tier cannot pass by missing
one.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import decode_cases as dc
import decode_rows_cases as rc
import oracle_lib
from test_decode_ref_cpu import _oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, S = rc.T, rc.S


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("decode_rows_sim") / "libdecode_rows_sim.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-o", out,
                           os.path.join(ROOT, "tests", "decode_rows_sim", "decode_rows_sim.cpp")])
    L = C.CDLL(out)
    L.sim_dr_max_stop.restype = C.c_int
    L.sim_decode_rows.restype = C.c_int64
    L.sim_decode_rows.argtypes = ([C.c_void_p, C.c_int] + [C.c_int64] * 3 + [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p] + [C.c_int] * 3
                                  + [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_int64] + [C.c_void_p] * 4)
    return L


_dev_tables = {}


def _table_arrays(name):
    """The table as the device holds it: offsets uint32 [n_ids_table + 1] into a blob (an id without an entry: empty)."""
    if name not in _dev_tables:
        tab = dc.table(name)
        lens = tab.lengths(np.arange(tab.n_ids_table))
        off = np.zeros(tab.n_ids_table + 1, dtype=np.uint32)
        np.cumsum(lens, out=off[1:])
        blob = np.frombuffer(b"".join(tab.table[i] for i in sorted(tab.table)), dtype=np.uint8)
        assert len(blob) == off[-1]
        _dev_tables[name] = (off, blob)
    return _dev_tables[name]


def _sim(sim, name, c, id_bytes, extra_stride):
    off, blob = _table_arrays(name)
    nr, width = c["rows"].shape
    stride = width + extra_stride
    m = np.full((max(nr, 1), max(stride, 1)), 0x7FFFFFF0, dtype=np.int64 if id_bytes == 8 else np.int32)   # the gaps: no valid id
    m[:nr, :width] = c["rows"]
    stop = np.array(c["stop"] + [0], dtype=np.int64)
    cap = 1 << 22
    out = np.zeros(cap, dtype=np.uint8)
    byte_off = np.full(nr + 1, -1, dtype=np.int64)
    status = np.full(max(nr, 1), 9, dtype=np.int32)
    cell = np.full(max(nr * width, 1), -1, dtype=np.int64)
    first = np.full(max(nr, 1), -9, dtype=np.int64)
    p = lambda a: None if a is None else a.ctypes.data
    n = sim.sim_decode_rows(m.ctypes.data, id_bytes, nr, width, stride, p(c["begin"]), p(c["end"]), c["pad_id"], stop.ctypes.data,
                            len(c["stop"]), int(c["skip_pad"]), int(c["keep_stop"]), off.ctypes.data, blob.ctypes.data, len(off) - 1,
                            out.ctypes.data, cap, byte_off.ctypes.data, status.ctypes.data, cell.ctypes.data, first.ctypes.data)
    assert n <= cap
    return dict(out=out[:n].tobytes(), byte_off=byte_off, status=status[:nr], cell_byte=cell[:nr * width].reshape(nr, width),
                first_stop=first[:nr])


@pytest.mark.parametrize("name", rc.TABLES)
def test_rule_header_equals_reference_on_every_case(sim, name):
    assert sim.sim_dr_max_stop() == 8
    exp = rc.expected(name)
    for c in rc.cases(name):
        for id_bytes, extra in ((8, 0), (8, 1), (4, 0), (4, 3)):
            if id_bytes == 4 and c["wide"]:
                continue
            got, e = _sim(sim, name, c, id_bytes, extra), exp[c["name"]]
            what = (c["name"], id_bytes, extra)
            assert got["out"] == e["out"], what
            for key in ("byte_off", "status", "cell_byte", "first_stop"):
                assert np.array_equal(got[key], e[key]), (what, key)


@pytest.mark.parametrize("name", rc.TABLES)
def test_reference_invariants(name):
    """What the contract promises about the outputs, on the reference itself."""
    for c in rc.cases(name):
        e = rc.expected(name)[c["name"]]
        nr, width = c["rows"].shape
        flat = e["cell_byte"].reshape(-1)
        assert (np.diff(flat) >= 0).all() and (np.diff(e["byte_off"]) >= 0).all(), c["name"]
        assert e["byte_off"][0] == 0 and e["byte_off"][-1] == len(e["out"]), c["name"]
        if width:
            assert np.array_equal(e["cell_byte"][:, 0], e["byte_off"][:-1]), c["name"]   # (cells left of b have no bytes)


@pytest.mark.parametrize("name", rc.TABLES)
def test_plain_matrix_equals_flat_reference_and_oracle(name):
    """Without options every row is one list: decode_ref on the rows as sequences gives the same, and the CPU oracle's
    decodeBytes agrees row by row (error -3 exactly where the status says so)."""
    tab, o, L = dc.table(name), _oracle(name), oracle_lib.lib()
    n_plain = n_bad = 0
    for c in rc.cases(name):
        if not rc.plain(c):
            continue
        n_plain += 1
        e = rc.expected(name)[c["name"]]
        nr, width = c["rows"].shape
        out, byte_off, status = tab.decode_ref(c["rows"].reshape(-1), np.arange(nr + 1, dtype=np.int64) * width)
        assert out == e["out"] and np.array_equal(byte_off, e["byte_off"]) and np.array_equal(status, e["status"]), c["name"]
        if c["wide"] or nr * width > 3 * T:
            continue                                                      # (the oracle takes 32-bit ids; a few cases are enough)
        ids = np.ascontiguousarray(c["rows"], dtype=np.int32)
        buf = np.empty(max(len(out), 1), dtype=np.uint8)
        for r in range(nr):
            n = L.jtko_decode(o._h, ids.ctypes.data + 4 * r * width, width, buf.ctypes.data, len(buf))
            if status[r]:
                assert n == oracle_lib.ERR_UNKNOWN_TOKEN, (c["name"], r)
                n_bad += 1
            else:
                assert buf[:n].tobytes() == out[byte_off[r]:byte_off[r + 1]], (c["name"], r)
    assert n_plain >= len(rc.WIDTHS) + 6 and n_bad > 10


@pytest.mark.parametrize("name", rc.TABLES)
def test_case_set_reaches_the_edges(name):
    """Conditions on the inputs and their expected results, so that a change to the builder cannot quietly lose an edge."""
    tile_sums, stop_res = set(), {8: set(), 512: set(), T: set()}
    kinds = set()
    widths, strided_lane_share = set(), False
    n_stop_ids = set()
    for c in rc.cases(name):
        e = rc.expected(name)[c["name"]]
        rows, (nr, width) = c["rows"], c["rows"].shape
        widths.add(width)
        n_stop_ids.add(len(c["stop"]))
        n_cells = nr * width
        if width in rc.WIDTHS and width > 0 and c["name"].startswith(("plain_w", "generated_")):
            assert n_cells > 3 * T and (n_cells % T != 0 or width % T == 0), c["name"]   # (rows of whole tiles: no ragged tail)
        flat = np.concatenate([e["cell_byte"].reshape(-1), [len(e["out"])]])
        edges = flat[np.minimum(np.arange(0, n_cells + T, T), n_cells)]
        tile_sums |= set(np.diff(edges).tolist())
        b = np.zeros(nr, dtype=np.int64) if c["begin"] is None else np.clip(c["begin"], 0, width)
        en = np.full(nr, width, dtype=np.int64) if c["end"] is None else np.clip(c["end"], 0, width)
        lens = dc.table(name).lengths(rows)
        for r in range(nr):
            s = int(e["first_stop"][r])
            if s >= 0:
                t = r * width + s
                for mod in stop_res:
                    stop_res[mod].add(t % mod)
                if s == b[r]:
                    kinds.add("stop at b")
                if s == width - 1:
                    kinds.add("stop at width - 1")
                if s + 1 < width and rows[r, s + 1] in c["stop"]:
                    kinds.add("dense fill behind the stop")
            if en[r] <= b[r]:
                kinds.add("empty window")
            if width and c["skip_pad"] and (rows[r] == c["pad_id"]).all():
                kinds.add("all-pad row")
            unknown = lens[r] == 0
            if c["skip_pad"]:
                unknown &= rows[r] != c["pad_id"]
            if (unknown & e["contributes"][r]).any():
                assert e["status"][r] == -3
                kinds.add("unknown inside")
                if r + 1 < nr and width % 8 and e["status"][r + 1] == 0 and unknown[width - 1]:
                    strided_lane_share = True                              # (the next row begins inside the same lane's 8 cells)
            elif unknown.any():
                assert e["status"][r] == 0
                kinds.add("unknown outside")
        if c["keep_stop"] and (e["first_stop"] >= 0).any():
            kinds.add("kept stop")
    assert {S - 1, S, S + 1} <= tile_sums and any(x > S + 1 for x in tile_sums) and any(1024 <= x < S - 1 for x in tile_sums)
    assert {7, 0} <= stop_res[8] and {511, 0} <= stop_res[512] and {T - 1, 0} <= stop_res[T]
    assert kinds == {"stop at b", "stop at width - 1", "dense fill behind the stop", "empty window", "all-pad row", "unknown inside",
                     "unknown outside", "kept stop"}
    assert set(rc.WIDTHS) <= widths and strided_lane_share and {0, 1, 8} <= n_stop_ids
    assert any(c["wide"] for c in rc.cases(name))
    assert len({c["name"] for c in rc.cases(name)}) == len(rc.cases(name))
