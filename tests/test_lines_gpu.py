"""jtk_batch_line_units / jtk_batch_line_repeats and the Python surface on them (Batch.line_units, Batch.line_repeats,
HipEncoding.line_repeats_batch, line_repeats_batch_device, repetition_signals(lines=True)): every case of tests/lines_cases.py
through the C ABI, all twelve outputs equal to the plain restatement tests/lines_ref.py exactly -- the pass is integer arithmetic
only.  Every test here needs a real MI355X (`-m gpu`)."""
import ctypes as C

import numpy as np
import pytest

import lines_cases as lc
import lines_ref as lr

pytestmark = pytest.mark.gpu

GUARD8, GUARD32, GUARD64 = 0x5A, 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A
PAD = 4                                      # guard elements before and behind every output
CASES = {c.name: c for c in lc.cases()}
MODES = [(unit, trim, mark) for unit, trim in lc.COMBOS for mark in (False, True)]
PER_UNIT = ("unit_begin", "unit_end", "unit_flags")
INT32 = ("n_dup", "top_count")
SUBSETS = (("unit_flags",), ("unit_begin", "unit_end"), ("unit_off", "doc_chars"), ("n_dup", "dup_chars", "top_first"), ("top_count",),
           ("dup_bytes", "unit_bytes", "unit_chars"), ("unit_off",), ())
_REF = {}


@pytest.fixture(scope="module")
def jt():
    import jtokkit_amd
    return jtokkit_amd


@pytest.fixture(scope="module")
def enc(jt):
    return jt.get_encoding("cl100k_base")


def ref(case, unit, trim, mark, base=None):
    """The restatement's result of a case in one mode, computed once, shared and left unchanged."""
    key = (case.name, unit, trim, mark, base)
    if key not in _REF:
        r = lr.repeats(case.docs, lc.status_of(case), unit, trim, mark, case.seed, case.base if base is None else base)
        for out in lr.OUTS:
            getattr(r, out).setflags(write=False)
        _REF[key] = r
    return _REF[key]


def pack(docs):
    doc_off = np.zeros(len(docs) + 1, dtype=np.int64)
    if docs:
        np.cumsum([len(x) for x in docs], out=doc_off[1:])
    return (np.frombuffer(b"".join(docs), dtype=np.uint8) if doc_off[-1] else np.zeros(0, dtype=np.uint8)), doc_off


def device_copy(text, doc_off):
    import torch
    d_text = torch.zeros(len(text) + 32, dtype=torch.uint8, device="cuda")           # (16-byte aligned, readable past the end)
    if len(text):
        d_text[:len(text)].copy_(torch.from_numpy(text.copy()))
    d_off = torch.from_numpy(doc_off).cuda()
    torch.cuda.synchronize()
    return d_text, d_off


def encode(enc, case, via, stream=None, b=None):
    """A batch (a fresh one unless given) holding the encode of the case's documents by its route: through host input, device
    input, or a count-only encode of device input.  The statuses the device leaves have the signs the case expects."""
    b = b or enc.new_batch()
    kw = dict(ordinary=case.route != "encode", validate=case.route == "validate", count_only=via == "count_only")
    text, doc_off = pack(case.docs)
    if via == "host":
        b.encode_host(text, doc_off, **kw)
    else:
        b._keep = device_copy(text, doc_off)
        b.encode_device(b._keep[0].data_ptr(), b._keep[1].data_ptr(), len(case.docs), len(text), stream=stream, **kw)
    status = b.fetch_counts()[1]
    assert (np.sign(status) == np.sign(lc.status_of(case))).all(), (case.name, via, status)
    return b


def run(b, nd, unit, trim, mark, seed, base, stream=None, want=None, shift=1):
    """line_units, then line_repeats into torch buffers with guards around every output; shift: the offset of the flag bytes past
    an 8-byte boundary.  Returns (n_units, the outputs by name); one that was not asked for is None (its buffer is checked
    untouched)."""
    import torch
    nu = b.line_units(unit, trim, seed, base, stream)
    bufs, lo, n = {}, {}, {}
    for name in lr.OUTS:
        n[name] = nu if name in PER_UNIT else nd + 1 if name == "unit_off" else nd
        if name == "unit_flags":
            bufs[name], lo[name] = torch.full((nu + 32 + shift,), GUARD8, dtype=torch.uint8, device="cuda"), 16 + shift
        elif name in INT32:
            bufs[name], lo[name] = torch.full((nd + 2 * PAD,), GUARD32, dtype=torch.int32, device="cuda"), PAD
        else:
            bufs[name], lo[name] = torch.full((n[name] + 2 * PAD,), GUARD64, dtype=torch.int64, device="cuda"), PAD
    torch.cuda.synchronize()                 # (the fills run on torch's stream, the pass on the batch's or the caller's)
    asked = lr.OUTS if want is None else want
    b.line_repeats(unit, trim, mark, seed, base, stream, **{name: bufs[name].data_ptr() + lo[name] * bufs[name].element_size() for name in asked})
    torch.cuda.synchronize()
    out = {}
    for name in lr.OUTS:
        a = bufs[name].cpu().numpy()
        guard = GUARD8 if name == "unit_flags" else GUARD32 if name in INT32 else GUARD64
        assert (a[:lo[name]] == guard).all() and (a[lo[name] + n[name]:] == guard).all(), name
        if name not in asked:
            assert (a == guard).all(), name
        out[name] = a[lo[name]:lo[name] + n[name]] if name in asked else None
    return nu, out


def same(got, exp, what):
    nu, outs = got
    assert nu == len(exp.unit_begin), (what, nu, len(exp.unit_begin))
    for name, g in outs.items():
        if g is not None:
            e = getattr(exp, name)
            assert np.array_equal(g, e), (what, name, np.flatnonzero(g != e)[:10])


@pytest.mark.parametrize("name", list(CASES))
def test_every_case_equals_the_reference(jt, enc, name):
    """All twelve outputs for both units, both TRIM values and both modes after a device-input encode, half of the modes after a
    host-input and a count-only encode; at the default and at the smallest table budget; guards around every buffer, the flag bytes
    at offsets 1 and 7; subsets of the outputs."""
    N = jt._native
    case = CASES[name]
    nd = len(case.docs)
    big = name == "scan_steps"
    for via in ("device", "host", "count_only"):
        b = encode(enc, case, via)
        if big:
            modes = {"device": [MODES[0], MODES[7]], "host": [MODES[5]], "count_only": [MODES[2]]}[via]
        else:
            modes = {"device": MODES, "host": MODES[0::2], "count_only": MODES[1::2]}[via]
        for i, (unit, trim, mark) in enumerate(modes):
            exp = ref(case, unit, trim, mark)
            got = run(b, nd, unit, trim, mark, case.seed, case.base, shift=(1, 7)[i & 1])
            same(got, exp, (name, via, unit, trim, mark))
            b.set_option(N.JTK_OPT_REPEAT_TABLE_BYTES, N.JTK_RP_MIN_TABLE_BYTES)
            small = run(b, nd, unit, trim, mark, case.seed, case.base)
            b.set_option(N.JTK_OPT_REPEAT_TABLE_BYTES, 256 << 20)
            assert all(np.array_equal(x, small[1][k]) for k, x in got[1].items()), (name, via, unit, trim, mark, "the smallest budget")
        if via == "device" and not big:
            unit, trim, mark = MODES[3]
            for want in SUBSETS:
                same(run(b, nd, unit, trim, mark, case.seed, case.base, want=want), ref(case, unit, trim, mark), (name, want))
        b.close()


def test_a_callers_stream(jt, enc):
    import torch
    st = torch.cuda.Stream()
    for name in ("long_unit", "grouping", "counts"):
        case = CASES[name]
        nd = len(case.docs)
        b = encode(enc, case, "device", stream=st.cuda_stream)
        same(run(b, nd, lr.LINE, False, True, case.seed, case.base, stream=st.cuda_stream), ref(case, lr.LINE, False, True), name)
        # the list and the table are reused from the batch's own stream, then from the caller's again: the calls take effect in order
        same(run(b, nd, lr.PARAGRAPH, True, False, case.seed, case.base), ref(case, lr.PARAGRAPH, True, False), (name, "own stream"))
        same(run(b, nd, lr.LINE, True, False, case.seed, case.base, stream=st.cuda_stream), ref(case, lr.LINE, True, False), (name, "caller's again"))
        b.close()


def test_shard_property(jt, enc):
    """Documents [cut:] encoded alone with doc_index_base = cut give the whole batch's per-document results, and its per-unit
    results shifted."""
    docs = CASES["counts"].docs + CASES["doc_edges"].docs + CASES["grouping"].docs + CASES["newline_runs"].docs
    whole_case = lc.Case("shards", docs, "ordinary", 77, 0)
    b = encode(enc, whole_case, "device")
    nu, whole = run(b, len(docs), lr.LINE, True, True, 77, 0)
    same((nu, whole), ref(whole_case, lr.LINE, True, True), "whole")
    assert whole["n_dup"].sum() > 0
    b.close()
    doc_off = pack(docs)[1]
    for cut in (1, len(docs) // 2, len(docs) - 2):
        b = encode(enc, lc.Case("part", docs[cut:], "ordinary", 77, cut), "device")
        _, part = run(b, len(docs) - cut, lr.LINE, True, True, 77, cut)
        u0 = int(whole["unit_off"][cut])
        assert np.array_equal(part["unit_begin"] + doc_off[cut], whole["unit_begin"][u0:]) and np.array_equal(part["unit_end"] + doc_off[cut], whole["unit_end"][u0:])
        assert np.array_equal(part["unit_flags"], whole["unit_flags"][u0:]) and np.array_equal(part["unit_off"] + u0, whole["unit_off"][cut:])
        for k in ("n_dup", "dup_bytes", "dup_chars", "unit_bytes", "unit_chars", "doc_chars", "top_count", "top_first"):
            assert np.array_equal(part[k], whole[k][cut:]), (cut, k)
        b.close()


def test_invalid_arguments_and_stale_lists(jt, enc):
    import torch
    N = jt._native
    L = N.lib()
    E = N.JTK_ERR_INVALID_ARGUMENT
    case = CASES["counts"]
    exp = ref(case, lr.LINE, False, False)
    text, doc_off = pack(case.docs)
    nd, nu = len(case.docs), len(exp.unit_begin)
    b = enc.new_batch()
    u8 = torch.full((nu + 64,), GUARD8, dtype=torch.uint8, device="cuda")
    i32 = torch.full((nd + 8,), GUARD32, dtype=torch.int32, device="cuda")
    i64 = torch.full((nu + nd + 8,), GUARD64, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    good = N.LinesParamsStruct(case.seed, case.base, 0, 0)

    def fields(**over):
        f = {name: (u8 if name == "unit_flags" else i32 if name in INT32 else i64).data_ptr() for name in lr.OUTS}
        f.update(over)
        return N.LinesOutStruct(**f)

    def units(bh, p=good):
        n = C.c_int64(-1)
        rc_ = L.jtk_batch_line_units(bh, C.byref(p) if p is not None else None, None, C.byref(n))
        assert rc_ == N.JTK_OK or (N.last_error() and n.value == 0)
        return rc_

    def repeats(bh, p=good, o=None):
        o = o or fields()
        rc_ = L.jtk_batch_line_repeats(bh, C.byref(p) if p is not None else None, C.byref(o), None)
        assert rc_ == N.JTK_OK or N.last_error()
        return rc_

    assert units(b._h) == E and repeats(b._h) == E                                                # before any encode
    b.encode_host(text, doc_off, ordinary=True)
    b.chunk(100, 10)
    b.pack(64)

    def others():
        sig = torch.zeros((nd, 64), dtype=torch.int32, device="cuda")
        fl = torch.zeros((b.result()[0] + 8,), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        b.minhash(sig.data_ptr(), 5, 64, 0, 3)
        b.ngram_repeats(2, fl.data_ptr(), seed=4)
        torch.cuda.synchronize()
        return b.chunk_fetch(), b.pack_fetch(), b.fetch(), sig.cpu().numpy(), fl.cpu().numpy()

    before = others()
    assert repeats(b._h) == E and "jtk_batch_line_units" in N.last_error()                        # no list yet
    for unit, fl in ((2, 0), (-1, 0), (0, 4), (1, 8), (0, 1 << 31)):
        assert units(b._h, N.LinesParamsStruct(0, 0, unit, fl)) == E and repeats(b._h, N.LinesParamsStruct(0, 0, unit, fl)) == E, (unit, fl)
    assert units(None) == E and units(b._h, None) == E and repeats(None) == E and repeats(b._h, None) == E
    assert L.jtk_batch_line_units(b._h, C.byref(good), None, None) == E                            # n_units NULL
    assert L.jtk_batch_line_repeats(b._h, C.byref(good), None, None) == E                          # out NULL
    assert units(b._h) == N.JTK_OK
    for name in lr.OUTS:                                                                          # misaligned int32 / int64 arrays
        if name == "unit_flags":
            continue
        for k in ((1, 2, 3) if name in INT32 else (1, 2, 4, 7)):
            assert repeats(b._h, o=fields(**{name: (i32 if name in INT32 else i64).data_ptr() + k})) == E, (name, k)
    # a list of other parameters does not serve: another unit, TRIM, seed or base (MARK_FIRST is the repeats' own)
    for p in (N.LinesParamsStruct(case.seed, case.base, 1, 0), N.LinesParamsStruct(case.seed, case.base, 0, 2),
              N.LinesParamsStruct(case.seed + 1, case.base, 0, 0), N.LinesParamsStruct(case.seed, case.base + 1, 0, 0)):
        assert repeats(b._h, p) == E
    torch.cuda.synchronize()
    for t, guard in ((u8, GUARD8), (i32, GUARD32), (i64, GUARD64)):
        assert (t.cpu().numpy() == guard).all()                                                   # a refused call wrote nothing
    # the pass still runs (MARK_FIRST on the same list too), and the other results of the encode are as they were
    same(run(b, nd, lr.LINE, False, False, case.seed, case.base), exp, "after the refusals")
    o = fields()
    assert L.jtk_batch_line_repeats(b._h, C.byref(N.LinesParamsStruct(case.seed, case.base, 0, 1)), C.byref(o), None) == N.JTK_OK
    torch.cuda.synchronize()
    after = others()
    for x, y in zip(before[:2], after[:2]):
        assert x.keys() == y.keys() and all(np.array_equal(x[k], y[k]) for k in x)
    assert all(np.array_equal(getattr(before[2], k), getattr(after[2], k)) for k in ("tokens", "tok_off", "status"))
    assert np.array_equal(before[3], after[3]) and np.array_equal(before[4], after[4])
    # a new encode drops the list
    b.encode_host(text, doc_off, ordinary=True)
    u8.fill_(GUARD8), i32.fill_(GUARD32), i64.fill_(GUARD64)
    torch.cuda.synchronize()
    assert repeats(b._h) == E
    torch.cuda.synchronize()
    for t, guard in ((u8, GUARD8), (i32, GUARD32), (i64, GUARD64)):
        assert (t.cpu().numpy() == guard).all()
    # not after a fill-in-the-middle encode: its tokens have no positions in the text
    b.set_fim(jt.FimParams(0.5, 0.5, seed=1, doc_index_base=0))
    b.encode_host(text, doc_off, ordinary=True, fim=True)
    assert units(b._h) == E and repeats(b._h) == E
    # not after an encode of caller-supplied pieces: its positions are not positions in the text
    b.encode_host(text, doc_off, ordinary=True)
    assert units(b._h) == N.JTK_OK
    b.encode_pieces(text, doc_off, doc_off[:-1], doc_off[1:])
    assert units(b._h) == E and "pieces" in N.last_error() and repeats(b._h) == E
    # not after jtk_batch_encode_device_max_tokens: it leaves no encode result
    b.encode_host(text, doc_off, ordinary=True)
    assert units(b._h) == N.JTK_OK
    d_text, d_off = device_copy(text, doc_off)
    rows = torch.zeros((nd, 8), dtype=torch.int32, device="cuda")
    kept, trunc, st = (torch.zeros(nd, dtype=dt, device="cuda") for dt in (torch.int64, torch.uint8, torch.int32))
    torch.cuda.synchronize()
    b.encode_device_max_tokens(d_text.data_ptr(), d_off.data_ptr(), nd, len(text), 8, rows.data_ptr(), kept.data_ptr(), trunc.data_ptr(),
                               st.data_ptr(), ordinary=True)
    torch.cuda.synchronize()
    assert units(b._h) == E and repeats(b._h) == E
    torch.cuda.synchronize()
    for t, guard in ((u8, GUARD8), (i32, GUARD32), (i64, GUARD64)):
        assert (t.cpu().numpy() == guard).all()
    b.close()


LINES = ["Home | About | Contact", "Click here to subscribe to our newsletter.", "Water boils at one hundred degrees Celsius at sea level.",
         "In 1969 the Apollo 11 mission landed two astronauts on the Moon.", "Canberra is the capital of Australia.", "© 2021 Example – all rights reserved",
         "naïve café – “quoted” text", "    indented code line", "x"]


def surface_batch():
    """40 small documents: some repeat boilerplate lines or paragraphs, some have CRLF or indented copies, some have none repeated."""
    docs = []
    for i in range(36):
        body = [LINES[(i + k) % len(LINES)] for k in range(2 + i % 5)]
        if i % 3 == 0:
            body += [LINES[0], LINES[i % len(LINES)], LINES[0]]
        if i % 4 == 1:
            body = body + [""] + body[:2] + ["", " "] + body[:2]
        if i % 5 == 2:
            body += ["  " + body[0] + " \r"]
        docs.append(("\r\n" if i % 7 == 3 else "\n").join(body) + ("\n" if i % 2 else ""))
    return docs + ["", "\n\n", "one line", "a\na\na\na"]


def test_python_surface_on_the_40_document_batch(jt, enc):
    import torch
    docs = surface_batch()
    bs = [d.encode() for d in docs]
    status = [0] * len(docs)
    exp = lr.repeats(bs, status, lr.PARAGRAPH, True, True, 5, 0)
    got = enc.line_repeats_batch(docs, unit="paragraph", trim=True, mark_first=True, seed=5)
    assert sorted(got) == sorted(lr.OUTS)
    for name in lr.OUTS:
        assert got[name].dtype == getattr(exp, name).dtype and np.array_equal(got[name], getattr(exp, name)), name
    text, doc_off = pack(bs)
    d_text, d_off = device_copy(text, doc_off)
    out = enc.line_repeats_batch_device(d_text[:len(text)], d_off, unit="line", seed=5, doc_index_base=9)
    torch.cuda.synchronize()
    exp = lr.repeats(bs, status, lr.LINE, False, False, 5, 9)
    assert out["unit_flags"].dtype == torch.uint8 and out["n_dup"].dtype == torch.int32 and out["unit_begin"].dtype == torch.int64
    assert (out["status"].cpu().numpy() == 0).all()
    for name in lr.OUTS:
        assert np.array_equal(out[name].cpu().numpy(), getattr(exp, name)), name
    # the fractions, exactly, from the restatement
    plain = enc.repetition_signals(docs, top=(2,), dup=(5,))
    off = enc.repetition_signals(docs, top=(2,), dup=(5,), lines=False)
    assert sorted(plain) == sorted(off) == ["dup", "n_bytes", "n_tokens", "status", "top"]
    for k in ("n_bytes", "n_tokens", "status"):
        assert np.array_equal(plain[k], off[k])
    for k in ("top", "dup"):
        assert plain[k].keys() == off[k].keys() and all(np.array_equal(a, c) for n in plain[k] for a, c in zip(plain[k][n], off[k][n]))
    for trim in (False, True):
        sig = enc.repetition_signals(docs, top=(2,), dup=(5,), lines=True, trim=trim)
        assert sorted(sig) == sorted(list(plain) + ["dup_line", "dup_paragraph", "n_lines", "n_paragraphs"])
        for name, unit in (("line", lr.LINE), ("paragraph", lr.PARAGRAPH)):
            r = lr.repeats(bs, status, unit, trim, False, 0, 0)
            n_units = np.diff(r.unit_off)
            assert np.array_equal(sig["n_%ss" % name], n_units)
            for d in range(len(docs)):
                want = (r.n_dup[d] / n_units[d] if n_units[d] else 0.0, r.dup_bytes[d] / len(bs[d]) if bs[d] else 0.0,
                        r.dup_chars[d] / r.doc_chars[d] if r.doc_chars[d] else 0.0)
                assert tuple(float(sig["dup_" + name][j][d]) for j in range(3)) == tuple(float(x) for x in want), (trim, name, d)
        assert sig["dup_line"][0].max() > 0.3 and sig["dup_line"][0].min() == 0.0


def test_an_empty_batch(jt, enc):
    z = enc.line_repeats_batch([])
    assert [len(z[name]) for name in lr.OUTS] == [0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0]
    e = enc.repetition_signals([], lines=True)
    assert len(e["n_lines"]) == 0 and all(len(x) == 0 for x in e["dup_line"] + e["dup_paragraph"])
    only_empty = enc.line_repeats_batch(["", ""], unit="paragraph", mark_first=True)
    assert len(only_empty["unit_begin"]) == 0 and only_empty["unit_off"].tolist() == [0, 0, 0]
    assert only_empty["top_count"].tolist() == [0, 0] and only_empty["top_first"].tolist() == [-1, -1] and only_empty["doc_chars"].tolist() == [0, 0]
    s = enc.repetition_signals(["", ""], lines=True)
    assert s["n_lines"].tolist() == [0, 0] and all((x == 0.0).all() for x in s["dup_line"] + s["dup_paragraph"])
