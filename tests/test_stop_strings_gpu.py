"""Stop strings on the device (jtk_stop.hip: k_stop_find, k_stop_finish) against the plain reference tests/stop_ref.py, on every
case of tests/stop_cases.py: matches on lane, wave and tile edges, strings across row ends, ties, `from`, held-back tails, cells
without bytes.  Every case runs after both decode kinds (flat, rows), from device and from host input, with int32 and int64 ids,
on the batch's stream and on a side stream; stop_pos, stop_which, hold and stop_col are compared exactly, through
jtk_batch_decode_stops_fetch and jtk_batch_decode_stops_device_result and through the four Python methods; the decode's own
outputs are the same bytes before and after the search.  Then the refusals, results dropped by a new decode, and a round trip of
this library's own chunk rows against str.find on the text, with no reference at all.  tests/test_stop_rules_cpu.py shows the
reference equal to the rule header and the case set complete.  Every test here needs a real MI355X (`-m gpu`)."""
import numpy as np
import pytest

import decode_cases as dc
import stop_cases as sc
import stop_ref as sr

pytestmark = pytest.mark.gpu

TABLE = "r50k_base"
UNK_ID = -5
CASES = sc.cases()
_REF = {}
LAYOUTS = {                      # decode kind, id bytes (rows) or host input (flat), side stream
    "rows_int32": ("rows", 4, False),
    "rows_int64_side_stream": ("rows", 8, True),
    "rows_int64_host_input": ("rows_host", 8, False),
    "rows_int32_host_input_side_stream": ("rows_host", 4, True),
    "flat": ("flat", 4, False),
    "flat_side_stream": ("flat", 4, True),
    "flat_host_input": ("flat_host", 4, False),
}


def ref(case, cells=True):
    key = (case.name, cells)
    if key not in _REF:
        _REF[key] = sr.find_stops(case.out, case.byte_off, case.strings, case.frm, case.cell_byte if cells and case.width else None)
    return _REF[key]


@pytest.fixture(scope="module")
def jt():
    import jtokkit_amd
    return jtokkit_amd


@pytest.fixture(scope="module")
def enc(jt):
    return jt.get_encoding(TABLE)


@pytest.fixture(scope="module")
def ids():
    """bytes -> id of the table under test, and the pad id: a real token that no case uses."""
    tab = dc.table(TABLE)
    by_bytes = {tok: i for i, tok in tab.table.items() if i < tab.n_table}
    for tok in sc.TOKENS:
        assert tok in by_bytes, tok
    assert all(bytes([x]) in by_bytes for x in range(256))
    return by_bytes, by_bytes[b"~"]


def matrix(case, ids):
    """int64 [n_rows, width] of the case's cells."""
    by_bytes, pad = ids
    m = np.full((len(case.rows), case.width), pad, dtype=np.int64)
    for r, row in enumerate(case.rows):
        for c, cell in enumerate(row):
            m[r, c] = pad if cell == sc.PAD else UNK_ID if cell == sc.UNK else by_bytes[cell]
    return m


def lists(case, ids):
    """The rows as id lists without the cells that hold no bytes: the same text from a flat decode."""
    by_bytes, _ = ids
    return [[by_bytes[cell] for cell in row if cell not in (sc.PAD, sc.UNK)] for row in case.rows]


class _Dev:
    def __init__(self, ptr, n, typestr):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": typestr, "data": (ptr, False), "version": 2}


def device_result(b, n):
    import torch
    p = b.decode_stops_device_result()
    view = lambda ptr, ts, dt: torch.as_tensor(_Dev(ptr, n, ts), device="cuda").cpu().numpy() if n else np.zeros(0, dtype=dt)
    return view(p[0], "<i8", np.int64), view(p[1], "<i4", np.int32), view(p[2], "<i4", np.int32), view(p[3], "<i8", np.int64)


def same(what, got, exp):
    for key, g, e in zip(("stop_pos", "stop_which", "hold", "stop_col"), got, exp):
        g = g.cpu().numpy() if hasattr(g, "cpu") else g
        assert g.shape == e.shape and g.dtype == e.dtype, (what, key, g.dtype, g.shape)
        assert np.array_equal(g, e), (what, key, np.flatnonzero(g != e)[:10], g[g != e][:10], e[g != e][:10])


def decode(b, case, ids, kind, id_bytes, stream):
    """One decode of the case's text on batch b -> (the tensors to keep alive, device pointer of cell_byte or None)."""
    import torch
    _, pad = ids
    n = len(case.rows)
    dt = np.int64 if id_bytes == 8 else np.int32
    if kind in ("flat", "flat_host"):
        seqs = lists(case, ids)
        flat = np.array([i for s in seqs for i in s], dtype=np.int32)
        seq_off = np.zeros(n + 1, dtype=np.int64)
        if n:
            np.cumsum([len(s) for s in seqs], out=seq_off[1:])
        if kind == "flat_host":
            assert b.decode_host(flat, seq_off) == len(case.out)
            return (), None
        d_ids, d_off = torch.from_numpy(flat).cuda(), torch.from_numpy(seq_off).cuda()
        torch.cuda.synchronize()                                           # (the library's streams do not wait for torch's)
        assert b.decode_device(d_ids.data_ptr() if len(flat) else None, d_off.data_ptr(), n, len(flat), stream) == len(case.out)
        return (d_ids, d_off), None
    m = matrix(case, ids).astype(dt)
    if kind == "rows_host":
        nb, cells = b.decode_rows_host(m, pad_id=pad, skip_pad=True, cell_byte=True)
        assert nb == len(case.out) and np.array_equal(cells, case.cell_byte)
        d_cells = torch.from_numpy(np.ascontiguousarray(cells)).cuda()
        torch.cuda.synchronize()
        return (d_cells,), d_cells.data_ptr() if cells.size else None
    d_m = torch.from_numpy(m).cuda()
    d_cells = torch.empty((n, case.width), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    nb = b.decode_rows_device(d_m.data_ptr() if m.size else None, id_bytes, n, case.width, pad_id=pad, skip_pad=True,
                              d_cell_byte_ptr=d_cells.data_ptr() if m.size else None, stream=stream)
    assert nb == len(case.out)
    return (d_m, d_cells), d_cells.data_ptr() if m.size else None


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_batch_entries_every_case(enc, ids, layout):
    """jtk_batch_decode_find_stops after every kind of decode, read through the fetch and through the device pointers; the
    decode's bytes, offsets and status are the same before and after."""
    import torch
    kind, id_bytes, on_side = LAYOUTS[layout]
    b = enc.new_batch()
    side = torch.cuda.Stream()
    stream = side.cuda_stream if on_side else None
    for case in CASES:
        n = len(case.rows)
        keep, cell_ptr = decode(b, case, ids, kind, id_bytes, stream)
        before = b.decode_fetch()
        assert before[0].tobytes() == case.out and np.array_equal(before[1], case.byte_off), case.name
        d_from = None if case.frm is None else torch.from_numpy(case.from_array()).cuda()
        torch.cuda.synchronize()
        b.decode_find_stops(case.strings, None if d_from is None else d_from.data_ptr(), cell_ptr, case.width if cell_ptr else 0, stream)
        exp = ref(case, cells=cell_ptr is not None)
        same((case.name, "fetch"), b.decode_stops_fetch(), exp)
        same((case.name, "device_result"), device_result(b, n), exp)
        after = b.decode_fetch()
        assert all(np.array_equal(x, y) for x, y in zip(before, after)), case.name
        del keep
    b.close()


def test_python_device_methods_every_case(enc, ids):
    """decode_rows_device and decode_rows_utf16_device with stop_strings: four more tensors, the others unchanged; without
    them, today's keys exactly."""
    import torch
    _, pad = ids
    base = {"bytes", "byte_off", "status"}
    for k, case in enumerate(CASES):
        if not len(case.rows):
            continue
        rows = torch.from_numpy(matrix(case, ids).astype(np.int64 if k % 2 else np.int32)).cuda()
        d_from = None if case.frm is None else torch.from_numpy(case.from_array()).cuda()
        plain = enc.decode_rows_device(rows, pad_id=pad)
        assert set(plain) == base and set(enc.decode_rows_device(rows, pad_id=pad, cell_offsets=True)) == base | {"cell_byte"}
        with torch.cuda.stream(torch.cuda.Stream()) if k % 3 == 0 else torch.cuda.stream(None):
            res = enc.decode_rows_device(rows, pad_id=pad, stop_strings=case.strings, search_from=d_from)
            res16 = enc.decode_rows_utf16_device(rows, pad_id=pad, cell_offsets=True, stop_strings=case.strings, search_from=d_from)
        torch.cuda.synchronize()
        stops = {"stop_pos", "stop_which", "hold", "stop_col"}
        assert set(res) == base | stops and set(res16) == base | stops | {"cell_byte", "units", "unit_off"}, case.name
        for r in (res, res16):
            same((case.name, "dict"), [r[key] for key in ("stop_pos", "stop_which", "hold", "stop_col")], ref(case))
            for key in base:
                assert torch.equal(r[key], plain[key]), (case.name, key)
        assert np.array_equal(res16["cell_byte"].cpu().numpy(), case.cell_byte), case.name
        assert set(enc.decode_rows_utf16_device(rows, pad_id=pad)) == base | {"units", "unit_off"}
    with pytest.raises(ValueError):
        enc.decode_rows_device(rows, search_from=torch.zeros(rows.shape[0], dtype=torch.int64, device="cuda"))


def test_python_host_methods_every_case(enc, ids):
    """decode_rows and decode_batch with stop_strings return every row cut at its stop, with the stop string when asked."""
    _, pad = ids
    for case in CASES:
        pos, which, _, _ = ref(case)
        plain = sr.cut_rows(case.out, case.byte_off, case.byte_off[1:], np.full(len(case.rows), -1), case.strings)
        for keep in (False, True):
            exp = sr.cut_rows(case.out, case.byte_off, pos, which, case.strings, keep)
            kw = dict(stop_strings=case.strings, search_from=case.frm, keep_stop_string=keep)
            if len(case.rows):
                assert enc.decode_rows(matrix(case, ids), pad_id=pad, strict=False, **kw) == exp, (case.name, keep)
            assert enc.decode_batch(lists(case, ids), **kw) == exp, (case.name, keep)
        if len(case.rows):
            assert enc.decode_rows(matrix(case, ids), pad_id=pad, strict=False) == plain, case.name
        assert enc.decode_batch(lists(case, ids)) == plain, case.name
    hello_world = [[ids[0][b"hello"], ids[0][b" world"]]]
    assert enc.decode_batch(hello_world, stop_strings="o w") == [b"hell"]         # a str is its UTF-8 bytes; one alone is a list of one
    assert enc.decode_batch(hello_world, stop_strings=["é", "wor"], keep_stop_string=True) == [b"hello wor"]


def _find(jt, b, blob, off, n, d_from=None, d_cell=None, width=0):
    from jtokkit_amd import _native as N
    blob = np.frombuffer(blob, dtype=np.uint8) if blob is not None else None
    off = np.array(off, dtype=np.uint32) if off is not None else None
    return N.lib().jtk_batch_decode_find_stops(b._h, None if blob is None or not len(blob) else blob.ctypes.data,
                                               None if off is None else off.ctypes.data, n, d_from, d_cell, width, None)


def test_refusals(jt, enc, ids):
    import torch
    from jtokkit_amd import _native as N
    by_bytes, pad = ids
    bad = N.JTK_ERR_INVALID_ARGUMENT
    b = enc.new_batch()
    assert _find(jt, b, b"ab", [0, 2], 1) == bad                              # no decode on the batch
    with pytest.raises(jt.EncodingError):
        b.decode_stops_device_result()
    rows = torch.tensor([[by_bytes[b"a"], by_bytes[b"b"], pad]] * 3, dtype=torch.int64, device="cuda")
    cells = torch.zeros((3, 3), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    b.decode_rows_device(rows.data_ptr(), 8, 3, 3, pad_id=pad, skip_pad=True, d_cell_byte_ptr=cells.data_ptr())
    with pytest.raises(jt.EncodingError):
        b.decode_stops_device_result()                                        # a decode, but no search yet
    assert _find(jt, b, b"a" * 17, list(range(18)), 17) == bad                # too many strings
    assert _find(jt, b, b"a", [0, 1], -1) == bad
    assert _find(jt, b, b"ab", [0, 2, 2], 2) == bad                           # an empty string
    assert _find(jt, b, b"a" * 65, [0, 65], 1) == bad                         # a string of 65 bytes
    assert _find(jt, b, b"abc", [1, 3], 1) == bad                             # str_off does not start at 0
    assert _find(jt, b, b"abc", [0, 2, 1], 2) == bad                          # str_off decreases
    assert _find(jt, b, None, [0, 2], 1) == bad and _find(jt, b, b"ab", None, 1) == bad
    assert _find(jt, b, b"ab", [0, 2], 1, None, cells.data_ptr(), 0) == bad   # cell_byte with width < 1
    assert _find(jt, b, b"ab", [0, 2], 1, None, cells.data_ptr(), 4) == bad   # not the width of the rows decode
    with pytest.raises(jt.EncodingError):
        b.decode_stops_device_result()                                        # a refused search leaves no result
    assert _find(jt, b, b"a" * 64, [0, 64], 1, None, cells.data_ptr(), 3) == 0
    assert _find(jt, b, None, [0], 0) == 0 and _find(jt, b, None, None, 0) == 0   # no strings: valid
    pos, which, hold, col = b.decode_stops_fetch()
    assert pos.tolist() == [2, 4, 6] and which.tolist() == [-1] * 3 and hold.tolist() == [0] * 3 and col.tolist() == [-1] * 3
    b.decode_host(np.array([by_bytes[b"a"]], dtype=np.int32), np.array([0, 1], dtype=np.int64))
    assert _find(jt, b, b"ab", [0, 2], 1, None, cells.data_ptr(), 1) == bad   # a flat decode has no cells
    assert _find(jt, b, b"ab", [0, 2], 1) == 0
    b.close()


def test_a_new_decode_drops_the_results(jt, enc, ids):
    by_bytes, _ = ids
    b = enc.new_batch()
    one = (np.array([by_bytes[b"a"], by_bytes[b"b"]], dtype=np.int32), np.array([0, 2], dtype=np.int64))
    for again in (lambda: b.decode_host(*one), lambda: b.decode_rows_host(one[0].reshape(1, 2))):
        b.decode_host(*one)
        b.decode_find_stops([b"b"])
        assert [x.tolist() for x in b.decode_stops_fetch()] == [[1], [0], [0], [-1]]
        assert all(b.decode_stops_device_result())
        again()
        with pytest.raises(jt.EncodingError):
            b.decode_stops_fetch()
        with pytest.raises(jt.EncodingError):
            b.decode_stops_device_result()
    b.close()


def test_chunk_rows_round_trip_against_str_find(jt):
    """No reference: chunk rows of a text, decoded and cut at a stop string taken from the text, against str.find on the text."""
    import torch
    from jtokkit_amd import corpus
    enc = jt.get_encoding("cl100k_base")
    text, doc_off = corpus.mixed(200, mean_bytes=600, lo=32, hi=4096)
    raw = text.tobytes()
    stops = [raw[doc_off[3] + 40:doc_off[3] + 44].decode("utf-8", "ignore") or " the", ". ", "\n\n"]
    bstops = [s.encode("utf-8") for s in stops]
    ck = enc.chunk_batch_device(torch.from_numpy(text).cuda(), torch.from_numpy(doc_off).cuda(), 64, ordinary=True, pad_id=-1)
    assert (ck["status"] == 0).all().item()
    bb, be = ck["byte_begin"].cpu().numpy(), ck["byte_end"].cpu().numpy()
    want, n_hit = [], 0
    for k in range(len(bb)):
        chunk = raw[bb[k]:be[k]]
        hits = [p for p in (chunk.find(s) for s in bstops) if p >= 0]
        n_hit += bool(hits)
        want.append(chunk[:min(hits)] if hits else chunk)
    assert 0 < n_hit < len(bb)
    res = enc.decode_rows_device(ck["rows"], pad_id=-1, stop_strings=stops)
    out, off, pos = res["bytes"].cpu().numpy().tobytes(), res["byte_off"].cpu().numpy(), res["stop_pos"].cpu().numpy()
    assert [out[off[k]:pos[k]] for k in range(len(want))] == want
    col, which = res["stop_col"].cpu().numpy(), res["stop_which"].cpu().numpy()
    assert ((col >= 0) == (which >= 0)).all() and (col < ck["n_tok"].cpu().numpy())[which >= 0].all()
    assert enc.decode_rows(ck["rows"].cpu().numpy(), pad_id=-1, stop_strings=stops) == want
