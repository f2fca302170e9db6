"""jtk_batch_phrase_hits and the Python surface on it (PhraseSet, Batch.phrase_hits, phrase_hits_batch, phrase_hits_batch_device,
C4_PHRASES): the cases of tests/phrase_ref.py, every output equal to its plain restatement exactly, through host and device input,
with and without folding and word boundaries; the units are the device's own line list, read back through
jtk_batch_line_repeats.  Every test needs a real MI355X (`-m gpu`)."""
import numpy as np
import pytest

import phrase_ref as pr
from jtokkit_amd import _native as N

pytestmark = pytest.mark.gpu
GUARD, PAD = 0x5A, 4


@pytest.fixture(scope="module")
def enc():
    import jtokkit_amd
    return jtokkit_amd.get_encoding("cl100k_base")


def check(enc, c, via, fold, word_bounds, unit="line", trim=False, **kw):
    """The case encoded by its route through host or device input, the list of line_units read back, every output against the restatement."""
    import torch
    b = enc.new_batch()
    kw = dict(dict(ordinary=c.route != "encode"), **kw)
    text, doc_off = pr.pack(c.docs)
    if via == "host":
        b.encode_host(text, doc_off, **kw)
    else:
        b._keep = (torch.from_numpy(np.concatenate([text, np.zeros(32, np.uint8)])).cuda(), torch.from_numpy(doc_off).cuda())
        torch.cuda.synchronize()
        b.encode_device(b._keep[0].data_ptr(), b._keep[1].data_ptr(), len(c.docs), len(text), **kw)
    assert (np.sign(b.fetch_counts()[1]) == np.sign(c.status)).all(), (c.name, via)
    nu = b.line_units(unit, trim)
    t = [torch.zeros(n, dtype=torch.int64, device="cuda") for n in (len(c.docs) + 1, nu, nu)]
    torch.cuda.synchronize()
    b.line_repeats(unit, trim, **{k: x.data_ptr() for k, x in zip(("unit_off", "unit_begin", "unit_end"), t) if x.numel()})
    torch.cuda.synchronize()
    exp = pr.hits(c.docs, c.status, c.phrases, fold, word_bounds, tuple(x.cpu().numpy() for x in t))
    ps = enc.phrase_set(c.phrases, fold_ascii=fold, word_bounds=word_bounds)
    assert len(ps) == len({pr.fold(ph) if fold else ph for ph, _ in c.phrases})
    got = run(b, ps, len(c.docs), nu)
    for k, _ in pr.OUTS:
        assert np.array_equal(got[k], exp[k]), (c.name, via, fold, word_bounds, unit, trim, k, got[k], exp[k])
    return b, ps, got


def run(b, ps, nd, nu, want=None):
    """phrase_hits into torch buffers with guard cells around every output; one that was not asked for is checked untouched."""
    import torch
    want = [k for k, _ in pr.OUTS] if want is None else want
    size = {k: (nu if k == "unit_mask" else nd) for k, _ in pr.OUTS}
    bufs = {k: torch.full(((size[k] + 2 * PAD) * np.dtype(dt).itemsize,), GUARD, dtype=torch.uint8, device="cuda") for k, dt in pr.OUTS}
    torch.cuda.synchronize()                 # (the fills run on torch's stream, the pass on the batch's)
    b.phrase_hits(ps, **{k: bufs[k].data_ptr() + PAD * np.dtype(dict(pr.OUTS)[k]).itemsize for k in want})
    torch.cuda.synchronize()
    out = {}
    for k, dt in pr.OUTS:
        a = bufs[k].cpu().numpy().view(dt)
        guard = np.frombuffer(bytes([GUARD]) * 8, dtype=dt)[0]
        assert (a[:PAD] == guard).all() and (a[PAD + size[k]:] == guard).all() and (k in want or (a == guard).all()), k
        out[k] = a[PAD:PAD + size[k]]
    return out


@pytest.mark.parametrize("via", ["host", "device"])
@pytest.mark.parametrize("word_bounds", [False, True])
@pytest.mark.parametrize("fold", [False, True])
@pytest.mark.parametrize("name", list(pr.CASES))
def test_case_equals_restatement(enc, name, fold, word_bounds, via):
    got = check(enc, pr.CASES[name], via, fold, word_bounds)[2]
    assert name != "dense_one_document" or word_bounds or got["n_hits"][0] == 19999
    if name == "table_in_global":            # the same text against the six phrases alone, their table in LDS: identical
        assert enc.phrase_set(pr.CASES[name].phrases).n_states > N.JTK_PH_LDS_SLOTS // 2 >= enc.phrase_set(pr.CASES["table_in_lds"].phrases).n_states
        near = check(enc, pr.CASES["table_in_lds"], via, fold, word_bounds)[2]
        assert all(np.array_equal(got[k], near[k]) for k, _ in pr.OUTS)


@pytest.mark.parametrize("trim", [False, True])
@pytest.mark.parametrize("unit", ["line", "paragraph"])
def test_units_of_either_kind_and_count_only(enc, unit, trim):
    got = check(enc, pr.CASES["units"], "device", True, False, unit, trim, count_only=True)[2]
    assert got["n_hit_units"][0] >= 3 and got["unit_mask"].any()


def test_each_output_alone_and_refusals_write_nothing(enc):
    import jtokkit_amd as jt
    import torch
    c = pr.CASES["units"]
    nd = len(c.docs)
    b, ps, full = check(enc, c, "host", False, False)
    for k, _ in pr.OUTS:
        assert np.array_equal(run(b, ps, nd, len(full["unit_mask"]), want=[k])[k], full[k]), k
    run(b, ps, nd, len(full["unit_mask"]), want=[])
    buf = torch.full((4096,), GUARD, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    p = buf.data_ptr() + 16

    def refused(ps=ps, **kw):
        with pytest.raises(jt.EncodingError) as e:
            b.phrase_hits(ps, **(kw or dict(group_mask=p, n_hits=p + 1024, first_hit=p + 2048)))
        assert e.value.code == N.JTK_ERR_INVALID_ARGUMENT, kw
    refused(ps=None)
    refused(ps=jt.new_encoding("r50k_base").phrase_set(c.phrases))
    for k, _ in pr.OUTS:
        refused(**{k: p + (4 if k == "first_hit" else 2)})       # misaligned
    text, doc_off = pr.pack(c.docs)
    b.encode_host(text, doc_off, ordinary=True)                  # (a new encode: no list is held)
    refused(unit_mask=p)
    refused(n_hit_units=p)
    b.set_fim(jt.FimParams(0.5, 0.5, seed=1, doc_index_base=0))
    b.encode_host(text, doc_off, ordinary=True, fim=True)
    refused()
    full_docs = doc_off[1:] > doc_off[:-1]
    b.encode_pieces(text, doc_off, doc_off[:-1][full_docs], doc_off[1:][full_docs])
    refused()
    d_text, d_off = torch.from_numpy(np.concatenate([text, np.zeros(32, np.uint8)])).cuda(), torch.from_numpy(doc_off).cuda()
    rows = torch.zeros(nd * 8, dtype=torch.int32, device="cuda")
    kept, trunc, st = (torch.zeros(nd, dtype=dt, device="cuda") for dt in (torch.int64, torch.uint8, torch.int32))
    torch.cuda.synchronize()
    b.encode_device_max_tokens(d_text.data_ptr(), d_off.data_ptr(), nd, len(text), 8, rows.data_ptr(), kept.data_ptr(), trunc.data_ptr(),
                               st.data_ptr(), ordinary=True)
    refused()
    with pytest.raises(jt.EncodingError):
        enc.phrase_set([b"x" * 65])
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == GUARD).all()


def test_c4_phrases_on_lines(enc):
    import jtokkit_amd as jt
    import torch
    lines = ["Read our Terms of Use before you go on.", "Privacy Policy | Cookie Policy", "This site uses cookies.", "We use cookies to serve you.",
             "Your use of cookies is up to you.", "Please enable JavaScript to view this page.", "A plain sentence about a cat.", "function f() { return 1; }",
             "Lorem ipsum dolor sit amet.", "lorem", "ipsum and javascript:void(0)", "The terms of\tuse are not here."]
    mask = lambda s: sum(1 << g for g in range(4) if any(ph in s.lower() for ph, gg in jt.C4_PHRASES if gg == g))
    ps = enc.phrase_set(jt.C4_PHRASES, fold_ascii=True)
    got = enc.phrase_hits_batch(["\n".join(lines), "nothing here"], ps, units="line", trim=True)
    assert list(got["group_mask"]) == [mask("\n".join(lines)), 0] and list(got["unit_mask"]) == [mask(ln) for ln in lines] + [0]
    assert list(got["first_hit"]) == [9, -1] and list(got["n_hit_units"]) == [sum(1 for ln in lines if mask(ln)), 0]
    text, doc_off = pr.pack(["\n".join(lines).encode(), b"nothing here"])
    dev = enc.phrase_hits_batch_device(torch.from_numpy(text.copy()).cuda(), torch.from_numpy(doc_off).cuda(), ps, units="line", trim=True)
    for k in got:
        assert np.array_equal(dev[k].cpu().numpy().astype(got[k].dtype), got[k]), k
    assert not dev["status"].cpu().numpy().any() and "unit_mask" not in enc.phrase_hits_batch(["a {"], ps)
