"""Decode of id matrices on the device (jtk_decode_rows.hip: k_dr_row_end, k_dr_count, k_dr_scatter) against the plain reference
tests/decode_rows_ref.py, on the inputs of tests/decode_rows_cases.py that are built for the kernels' own edges: every width from
0 to 5000 over at least three tiles, tiles on both sides of the LDS stage limit, windows and first stop columns on lane, wave and
tile edges, dense EOS fill, pads of every kind, ids without an entry in 32 and 64 bits.  n_bytes, every output byte, byte_off,
status and cell_byte are compared exactly, for both id widths, with and without a row stride, at addresses aligned to the id
size only, through both C entries and both Python methods; then round trips of this library's own padded rows against the text
they came from, with no reference at all.  tests/test_decode_rows_rules_cpu.py shows the reference equal to the rule header and
the case set complete.  Every test here needs a real MI355X (`-m gpu`)."""
import ctypes as C

import numpy as np
import pytest

import decode_cases as dc
import decode_rows_cases as rc

pytestmark = pytest.mark.gpu

GAP = 0x7FFFFFF0                 # what lies between the rows of a strided matrix: no valid id, never decoded
LAYOUTS = {                      # id bytes, extra row stride, misaligned start, side stream
    "int64": (8, 0, False, False),
    "int64_strided_8_mod_16_side_stream": (8, 1, True, True),
    "int32": (4, 0, False, False),
    "int32_strided_4_mod_16_side_stream": (4, 3, True, True),
}


@pytest.fixture(scope="module")
def jt():
    import jtokkit_amd
    return jtokkit_amd


@pytest.fixture(scope="module")
def encs(jt):
    kind, ranks, specials = dc.custom_spec()
    custom = jt.new_custom_encoding("decode_rows_custom", kind, ranks, specials)
    yield {name: custom if name == "custom" else jt.get_encoding(name) for name in rc.TABLES}
    custom.close()


def _same(what, got, e, cells=True):
    """got = (n_bytes, out uint8[], byte_off, status, cell_byte or None) of the device; e = decode_rows_ref's result."""
    nb, out, byte_off, status, cell_byte = got
    assert nb == len(e["out"]), what
    assert np.array_equal(status, e["status"]), (what, "status", np.flatnonzero(status != e["status"])[:5])
    assert np.array_equal(byte_off, e["byte_off"]), (what, "byte_off", np.flatnonzero(byte_off != e["byte_off"])[:5])
    exp = np.frombuffer(e["out"], dtype=np.uint8)
    assert len(out) == len(exp), what
    assert np.array_equal(out, exp), (what, "first wrong byte", int(np.flatnonzero(out != exp)[0]))
    if cells:
        assert cell_byte.shape == e["cell_byte"].shape and np.array_equal(cell_byte, e["cell_byte"]), (what, "cell_byte")


def _matrix(c, id_bytes, extra, misaligned):
    """The case's matrix on the device: (tensor that owns the memory, 2-d view [n_rows, width] with row stride width + extra)."""
    import torch
    nr, width = c["rows"].shape
    stride = width + extra
    host = np.full(nr * stride + 1, GAP, dtype=np.int64 if id_bytes == 8 else np.int32)
    if nr * width:
        host[1:].reshape(nr, stride)[:, :width] = c["rows"]
    buf = torch.from_numpy(host).cuda()
    if not misaligned:
        buf = buf[1:].clone()
        view = torch.as_strided(buf, (nr, width), (stride, 1))
    else:
        view = torch.as_strided(buf, (nr, width), (stride, 1), 1)
        assert view.numel() == 0 or view.data_ptr() % 16 == id_bytes
    return buf, view


def _dev(a):
    import torch
    return None if a is None else torch.from_numpy(np.array(a)).cuda()


class _Dev:
    def __init__(self, ptr, n, typestr):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": typestr, "data": (ptr, False), "version": 2}


def _device_result(b, nb, n_rows):
    import torch
    p = b.decode_device_result()
    view = lambda ptr, n, ts, dt: torch.as_tensor(_Dev(ptr, n, ts), device="cuda").cpu().numpy() if n else np.zeros(0, dtype=dt)
    return view(p[0], nb, "|u1", np.uint8), view(p[1], n_rows + 1, "<i8", np.int64), view(p[2], n_rows, "<i4", np.int32)


def _run_device(b, c, id_bytes, extra, misaligned, stream, cells=True):
    """Batch.decode_rows_device of a case -> (nb, cell_byte [n_rows, width] or None); the rest is read by the caller."""
    import torch
    nr, width = c["rows"].shape
    buf, view = _matrix(c, id_bytes, extra, misaligned)
    d_b, d_e = _dev(c["begin"]), _dev(c["end"])
    d_cell = torch.full((nr * width + 2,), -77, dtype=torch.int64, device="cuda") if cells else None
    torch.cuda.synchronize()                                               # (the library's streams do not wait for torch's)
    nb = b.decode_rows_device(view.data_ptr() if nr * width else None, id_bytes, nr, width, width + extra,
                              None if d_b is None else d_b.data_ptr(), None if d_e is None else d_e.data_ptr(), c["pad_id"], c["stop"],
                              c["skip_pad"], c["keep_stop"], d_cell[1:].data_ptr() if cells else None, stream)
    cell = None
    if cells:
        h = d_cell.cpu().numpy()
        assert h[0] == -77 and h[-1] == -77, c["name"]                     # nothing written around cell_byte
        cell = h[1:-1].reshape(nr, width)
    return nb, cell


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("name", rc.TABLES)
def test_device_entry_every_case(encs, name, layout):
    """jtk_batch_decode_rows_device on every case, one batch: fetched through jtk_batch_decode_fetch and read in place through
    jtk_batch_decode_device_result."""
    import torch
    id_bytes, extra, misaligned, on_side = LAYOUTS[layout]
    b = encs[name].new_batch()
    exp = rc.expected(name)
    side = torch.cuda.Stream()
    n = 0
    for c in rc.cases(name):
        if id_bytes == 4 and c["wide"]:
            continue
        nb, cell = _run_device(b, c, id_bytes, extra, misaligned, side.cuda_stream if on_side else None)
        _same((c["name"], "fetch"), (nb,) + b.decode_fetch() + (cell,), exp[c["name"]])
        _same((c["name"], "device_result"), (nb,) + _device_result(b, nb, c["rows"].shape[0]) + (None,), exp[c["name"]], cells=False)
        n += 1
    assert n >= 100
    b.close()


@pytest.mark.parametrize("name", rc.TABLES)
def test_host_entry_every_case(encs, name):
    """jtk_batch_decode_rows on host matrices: 64-bit cells, and 32-bit cells in a row-strided view where the values fit."""
    b = encs[name].new_batch()
    exp = rc.expected(name)
    for k, c in enumerate(rc.cases(name)):
        nr, width = c["rows"].shape
        opts = dict(begin=c["begin"], end=c["end"], pad_id=c["pad_id"], stop_ids=c["stop"], skip_pad=c["skip_pad"], keep_stop=c["keep_stop"])
        if c["wide"] or k % 2:
            rows = c["rows"]
        else:
            rows = np.full((nr, width + 3), GAP, dtype=np.int32)
            rows[:, :width] = c["rows"]
            rows = rows[:, :width]
        nb, cell = b.decode_rows_host(rows, cell_byte=True, **opts)
        _same(c["name"], (nb,) + b.decode_fetch() + (cell,), exp[c["name"]])
        if k % 7 == 0:                                                     # without cell_byte the rest is the same
            nb = b.decode_rows_host(rows, **opts)
            _same(c["name"], (nb,) + b.decode_fetch() + (None,), exp[c["name"]], cells=False)
    b.close()


def _py_options(c):
    """A case's options as HipEncoding.decode_rows* takes them (pad_id given == skipped), or None when they cannot be said so."""
    return dict(pad_id=c["pad_id"] if c["skip_pad"] else None, stop=c["stop"], keep_stop=c["keep_stop"])


@pytest.mark.parametrize("name", rc.TABLES)
def test_python_device_method(encs, name):
    """HipEncoding.decode_rows_device: tensors on the current stream -- the legacy default stream and a side stream --, a
    row-strided view read in place, both dtypes, with and without cell offsets."""
    import torch
    enc, exp = encs[name], rc.expected(name)
    side = torch.cuda.Stream()
    picked = [c for c in rc.cases(name) if c["name"].startswith(("generated_windows_w", "stop_", "pad_", "unknown_", "plain_w0", "no_rows"))]
    assert len(picked) > 40
    for k, c in enumerate(picked):
        id_bytes = 8 if c["wide"] or k % 2 else 4
        with torch.cuda.stream(side if k % 3 == 0 else torch.cuda.default_stream()):
            buf, view = _matrix(c, id_bytes, (0, 5)[k % 2], bool(k % 2))
            res = enc.decode_rows_device(view, _dev(c["begin"]), _dev(c["end"]), cell_offsets=k % 4 != 1, **_py_options(c))
            got = {key: t.cpu().numpy() for key, t in res.items()}          # (ordered after the call on the current stream)
        assert res["bytes"].dtype == torch.uint8 and res["byte_off"].dtype == torch.int64 and res["status"].dtype == torch.int32
        assert ("cell_byte" in res) == (k % 4 != 1)
        _same(c["name"], (len(got["bytes"]), got["bytes"], got["byte_off"], got["status"], got.get("cell_byte")), exp[c["name"]],
              cells="cell_byte" in res)
    m = torch.zeros((4, 6), dtype=torch.int64, device="cuda")
    for bad in (m.cpu(), m.float(), m[0], m.t(), m[:, ::2]):
        with pytest.raises(ValueError):
            enc.decode_rows_device(bad)
    for kw in (dict(begin=torch.zeros(3, dtype=torch.int64, device="cuda")), dict(end=torch.zeros(4, dtype=torch.int32, device="cuda")),
               dict(begin=np.zeros(4, dtype=np.int64)), dict(stop=list(range(9))), dict(stop=["<|no such token|>"])):
        with pytest.raises(ValueError):
            enc.decode_rows_device(m, **kw)


@pytest.mark.parametrize("name", rc.TABLES)
def test_python_host_method(jt, encs, name):
    """HipEncoding.decode_rows: a list of bytes per row; strict raises and names the first row with an unknown id."""
    enc, exp = encs[name], rc.expected(name)
    n_raised = n_clean = 0
    for c in rc.cases(name):
        if not c["name"].startswith(("generated_w", "stop_", "pad_", "unknown_", "plain_w9", "plain_w0", "no_rows")):
            continue
        e = exp[c["name"]]
        want = [e["out"][e["byte_off"][r]:e["byte_off"][r + 1]] for r in range(len(e["status"]))]
        rows = c["rows"] if c["wide"] else c["rows"].astype(np.int32)
        args = (rows, c["begin"], c["end"])
        assert enc.decode_rows(*args, strict=False, **_py_options(c)) == want, c["name"]
        if (e["status"] != 0).any():
            with pytest.raises(jt.EncodingError) as ei:
                enc.decode_rows(*args, **_py_options(c))
            assert ei.value.code == -3 and "(row %d)" % int(np.flatnonzero(e["status"] != 0)[0]) in str(ei.value), c["name"]
            n_raised += 1
        else:
            assert enc.decode_rows(*args, **_py_options(c)) == want, c["name"]
            n_clean += 1
    assert n_raised >= 5 and n_clean >= 5


def test_kept_stop_literal_and_stop_by_literal(encs):
    """A special token named by its literal ends the row; kept, its literal is the row's last bytes."""
    enc = encs["cl100k_base"]
    eot = enc.special_ids(["<|endoftext|>"])[0]
    hello = enc.encode("hello world")
    rows = np.array([hello + [eot, eot, eot], [eot] + hello + [eot, hello[0]], hello + hello[:1] + [hello[1], eot]], dtype=np.int64)
    assert enc.decode_rows(rows, stop=["<|endoftext|>"]) == [b"hello world", b"", b"hello worldhello world"]
    assert enc.decode_rows(rows, stop="<|endoftext|>", keep_stop=True) == [b"hello world<|endoftext|>", b"<|endoftext|>",
                                                                           b"hello worldhello world<|endoftext|>"]
    assert enc.decode_rows(rows, begin=[0, 1, 2], stop=[eot]) == [b"hello world", b"hello world", b"hello world"]


def test_cell_byte_is_optional_and_flat_decode_is_unchanged(encs):
    """Without a cell_byte pointer nothing of an earlier call's buffer is written; a flat decode on the same batch before and
    after gives what it always gave, and the rows result replaces it for fetch and device_result."""
    import torch
    name = "cl100k_base"
    b = encs[name].new_batch()
    by_name = {c["name"]: c for c in rc.cases(name)}
    flat = {c[0]: c for c in dc.cases(name)}
    c = by_name["generated_windows_w513"]
    nr, width = c["rows"].shape
    buf, view = _matrix(c, 8, 0, False)
    d_b, d_e = _dev(c["begin"]), _dev(c["end"])
    d_cell = torch.full((nr * width,), -5, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    args = (view.data_ptr(), 8, nr, width, width, d_b.data_ptr(), d_e.data_ptr(), c["pad_id"], c["stop"], c["skip_pad"], c["keep_stop"])

    def flat_is_right(cname):
        nb = b.decode_host(flat[cname][1], flat[cname][2])
        out, byte_off, status = b.decode_fetch()
        e_out, e_off, e_status = dc.expected(name)[cname]
        assert nb == len(e_out) and out.tobytes() == e_out and np.array_equal(byte_off, e_off) and np.array_equal(status, e_status)

    flat_is_right("fuzz_2")
    nb = b.decode_rows_device(*args, d_cell.data_ptr())
    _same("with cells", (nb,) + b.decode_fetch() + (d_cell.cpu().numpy().reshape(nr, width),), rc.expected(name)[c["name"]])
    d_cell.fill_(-5)
    torch.cuda.synchronize()
    nb = b.decode_rows_device(*args, None)
    _same("without cells", (nb,) + b.decode_fetch() + (None,), rc.expected(name)[c["name"]], cells=False)
    assert (d_cell == -5).all().item()
    flat_is_right("stage_%d_between_staged" % (dc.S + 1))
    flat_is_right("no_ids_300_seqs")
    nb = b.decode_rows_device(*args, None)
    _same("after flat", (nb,) + b.decode_fetch() + (None,), rc.expected(name)[c["name"]], cells=False)
    b.close()


def test_argument_errors(encs):
    """Every refusal of the two entries: JTK_ERR_INVALID_ARGUMENT, *n_bytes untouched, and the next valid decode is right."""
    import torch
    from jtokkit_amd import _native as N
    L = N.lib()
    name = "cl100k_base"
    c = {x["name"]: x for x in rc.cases(name)}["generated_w65"]
    e = rc.expected(name)[c["name"]]
    nr, width = c["rows"].shape
    b = encs[name].new_batch()
    host = np.ascontiguousarray(c["rows"])
    dev = torch.from_numpy(host).cuda()
    torch.cuda.synchronize()
    stop = np.array(c["stop"] * 9, dtype=np.int64)
    nb = C.c_int64(-7)
    good = dict(id_bytes=8, n_rows=nr, width=width, row_stride=width, stop=stop.ctypes.data, n_stop=1, flags=N.JTK_DECODE_SKIP_PAD, rows=True)
    bad = [dict(id_bytes=2), dict(id_bytes=0), dict(id_bytes=16), dict(row_stride=width - 1), dict(n_rows=-1), dict(width=-1),
           dict(width=-1, row_stride=-1), dict(n_stop=-1), dict(n_stop=9), dict(stop=None), dict(flags=4), dict(flags=N.JTK_DECODE_SKIP_PAD | 8),
           dict(flags=1 << 31), dict(rows=False)]

    def call(device, a):
        p = (dev.data_ptr() if device else host.ctypes.data) if a["rows"] else None
        head = (b._h, p, a["id_bytes"], a["n_rows"], a["width"], a["row_stride"], None, None, -1, a["stop"], a["n_stop"], a["flags"], None)
        if device:
            return L.jtk_batch_decode_rows_device(*head, None, C.byref(nb))
        return L.jtk_batch_decode_rows(*head, C.byref(nb))

    for device in (True, False):
        for change in bad:
            assert call(device, dict(good, **change)) == N.JTK_ERR_INVALID_ARGUMENT, (device, change)
            assert nb.value == -7, (device, change)
        assert call(device, good) == N.JTK_OK and nb.value == len(e["out"])
        b._dec_shape = (nb.value, nr)
        _same(("valid", device), (nb.value,) + b.decode_fetch() + (None,), e, cells=False)
        nb.value = -7
    # rows may be NULL when there are no cells; no rows and no columns are valid
    for shape in ((0, 5), (5, 0), (0, 0)):
        for device in (True, False):
            assert call(device, dict(good, rows=False, n_rows=shape[0], width=shape[1], row_stride=shape[1])) == N.JTK_OK
            assert nb.value == 0
            b._dec_shape = (0, shape[0])
            out, byte_off, status = b.decode_fetch()
            assert len(out) == 0 and byte_off.tolist() == [0] * (shape[0] + 1) and status.tolist() == [0] * shape[0]
    b.close()


# ---- round trips of this library's own rows, with no reference ---------------------------------------
@pytest.fixture(scope="module")
def corpus_dev():
    import torch
    from jtokkit_amd import corpus
    text, doc_off = corpus.mixed(300, mean_bytes=600, lo=32, hi=4096)
    for d in range(len(doc_off) - 1):
        text[doc_off[d]:doc_off[d + 1]].tobytes().decode("utf-8")          # every document is valid UTF-8
    return text, doc_off, torch.from_numpy(text).cuda(), torch.from_numpy(doc_off).cuda()


@pytest.mark.parametrize("chunk_tokens", [7, 64, 600])
def test_chunk_rows_round_trip(encs, corpus_dev, chunk_tokens):
    """chunk_batch_device rows decode to text[byte_begin:byte_end], chunk by chunk: with end = n_tok, and with the pad skipped."""
    enc = encs["cl100k_base"]
    text, doc_off, d_text, d_off = corpus_dev
    ck = enc.chunk_batch_device(d_text, d_off, chunk_tokens, ordinary=True, pad_id=-1)
    assert (ck["status"] == 0).all().item() and ck["rows"].shape[0] >= 300
    raw = text.tobytes()
    bb, be = ck["byte_begin"].cpu().numpy(), ck["byte_end"].cpu().numpy()
    want = [raw[bb[k]:be[k]] for k in range(len(bb))]
    for kw in (dict(end=ck["n_tok"].to(dtype=ck["byte_begin"].dtype)), dict(pad_id=-1)):
        res = enc.decode_rows_device(ck["rows"], cell_offsets=True, **kw)
        out, off = res["bytes"].cpu().numpy().tobytes(), res["byte_off"].cpu().numpy()
        assert (res["status"] == 0).all().item()
        assert [out[off[k]:off[k + 1]] for k in range(len(want))] == want
        assert np.array_equal(res["cell_byte"][:, 0].cpu().numpy(), off[:-1])
    if chunk_tokens == 7:                                                  # with neither, the pad cells are unknown ids
        res = enc.decode_rows_device(ck["rows"])
        padded = (ck["n_tok"] < chunk_tokens).cpu().numpy()
        assert padded.any() and np.array_equal(res["status"].cpu().numpy() != 0, padded)


@pytest.mark.parametrize("max_tokens", [1, 33, 200])
def test_max_tokens_rows_round_trip(encs, corpus_dev, max_tokens):
    """encode_batch_max_tokens_device rows decode to a prefix of their document: with end = kept, and with the pad skipped."""
    enc = encs["cl100k_base"]
    text, doc_off, d_text, d_off = corpus_dev
    rows, kept, truncated, status = enc.encode_batch_max_tokens_device(d_text, d_off, max_tokens, ordinary=True, pad_id=-1)
    assert (status == 0).all().item()
    raw = text.tobytes()
    results = []
    for kw in (dict(end=kept), dict(pad_id=-1)):
        res = enc.decode_rows_device(rows, **kw)
        out, off = res["bytes"].cpu().numpy().tobytes(), res["byte_off"].cpu().numpy()
        assert (res["status"] == 0).all().item()
        results.append((out, off.tolist()))
        tr = truncated.cpu().numpy()
        for d in range(len(doc_off) - 1):
            doc = raw[doc_off[d]:doc_off[d + 1]]
            got = out[off[d]:off[d + 1]]
            assert doc.startswith(got) and (tr[d] or got == doc), d
    assert results[0] == results[1]
