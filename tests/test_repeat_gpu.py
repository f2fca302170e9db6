"""jtk_batch_ngram_repeats and the Python surface on it (Batch.ngram_repeats, HipEncoding.ngram_repeats_batch,
ngram_repeats_batch_device, repetition_signals): every case of tests/repeat_cases.py through the C ABI, the flags and the four
per-document arrays equal to the plain restatement tests/repeat_ref.py exactly -- the pass is integer arithmetic only.  The ids the
restatement hashes are the CPU oracle's, and every case first checks that the device's encodes left exactly those.  Every test
here needs a real MI355X (`-m gpu`)."""
import ctypes as C
import itertools
from fractions import Fraction

import numpy as np
import pytest

import repeat_cases as rc
import repeat_ref as rr

pytestmark = pytest.mark.gpu

GUARD8, GUARD32, GUARD64 = 0x5A, 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A
PAD = 4                                      # guard elements before every per-document output
PAD8 = 16                                    # guard bytes before the flags (the 8-byte alignment stays)
CASES = {c.name: c for c in rc.cases()}
OUTS = ("flags", "n_repeat", "n_covered", "top_count", "top_first")
ALL = (True,) * 5
_REF = {}


@pytest.fixture(scope="module")
def jt():
    import jtokkit_amd
    return jtokkit_amd


@pytest.fixture(scope="module")
def enc(jt):
    return jt.get_encoding("cl100k_base")


def ref(case, mark_first):
    """(ids, statuses, the restatement's result) of a case in one mode, computed once and shared."""
    if (case.name, mark_first) not in _REF:
        ids, status = rc.ids_of(case.docs, case.route)
        r = rr.repeats(ids, status, case.n, case.seed, case.base, mark_first)
        for out in OUTS:
            getattr(r, out).setflags(write=False)
        _REF[case.name, mark_first] = (ids, status, r)
    return _REF[case.name, mark_first]


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


def encode(jt, enc, docs, route, via, stream=None, b=None):
    """A batch (a fresh one unless given) holding the encode of docs by route, through host or device input."""
    b = b or enc.new_batch()
    kw = dict(ordinary=route != "encode" and route != "allow_special")
    if route == "validate":
        kw["validate"] = True
    if route == "allow_special":
        b.set_allowed_special("all")
        kw["allow_special"] = True
    if route == "fim":
        b.set_fim(jt.FimParams(0.5, 0.5, seed=rc.mc.FIM["seed"], doc_index_base=rc.mc.FIM["base"]))
        kw["fim"] = True
    text, doc_off = pack(docs)
    if via == "host":
        b.encode_host(text, doc_off, **kw)
    else:
        b._keep = device_copy(text, doc_off)
        b.encode_device(b._keep[0].data_ptr(), b._keep[1].data_ptr(), len(docs), len(text), stream=stream, **kw)
    return b


def check_ids(b, docs, route):
    """The device holds the ids the restatement hashes; a refused document has a negative status (and whatever tokens the
    encode left it: the pass must not look at them).  Returns the device's tok_off."""
    ids, status = rc.ids_of(docs, route)
    res = b.fetch()
    assert (np.sign(res.status) == np.sign(status)).all()
    assert [res.doc(d).tolist() for d in range(len(ids)) if status[d] >= 0] == [x for x, st in zip(ids, status) if st >= 0]
    return res.tok_off


def run(b, case, mark_first, stream=None, want=ALL, shift=0, base=None):
    """jtk_batch_ngram_repeats into torch buffers with guards around every output; shift: bytes past the flags' 8-byte boundary.
    Returns the five outputs, None for one that was not asked for (its buffer is checked untouched)."""
    import torch
    nt, nd, _ = b.result()
    bufs = [torch.full((nt + 2 * PAD8 + shift,), GUARD8, dtype=torch.uint8, device="cuda")]
    bufs += [torch.full((nd + 2 * PAD,), GUARD32, dtype=torch.int32, device="cuda") for _ in range(3)]
    bufs += [torch.full((nd + 2 * PAD,), GUARD64, dtype=torch.int64, device="cuda")]
    lo = [PAD8 + shift, PAD, PAD, PAD, PAD]
    n = [nt, nd, nd, nd, nd]
    torch.cuda.synchronize()                 # (the fills run on torch's stream, the pass on the batch's or the caller's)
    b.ngram_repeats(case.n, *[t.data_ptr() + l * t.element_size() if w else None for t, l, w in zip(bufs, lo, want)], seed=case.seed,
                    mark_first=mark_first, doc_index_base=case.base if base is None else base, stream=stream)
    torch.cuda.synchronize()
    out = []
    for t, l, k, w, guard in zip(bufs, lo, n, want, (GUARD8, GUARD32, GUARD32, GUARD32, GUARD64)):
        a = t.cpu().numpy()
        assert (a[:l] == guard).all() and (a[l + k:] == guard).all()
        if not w:
            assert (a == guard).all()
        out.append(a[l:l + k] if w else None)
    return out


def expected_on_device(exp, status, tok_off):
    """The reference's flags in the device's token layout: a refused document has no tokens in the reference and whatever the
    encode left it on the device, all of them unflagged."""
    flags = np.zeros(int(tok_off[-1]), dtype=np.uint8)
    for d, st in enumerate(status):
        if st >= 0:
            assert tok_off[d + 1] - tok_off[d] == exp.tok_off[d + 1] - exp.tok_off[d]
            flags[tok_off[d]:tok_off[d + 1]] = exp.flags[exp.tok_off[d]:exp.tok_off[d + 1]]
    return flags


def same(got, exp, status, tok_off, what):
    want = [expected_on_device(exp, status, tok_off), exp.n_repeat, exp.n_covered, exp.top_count, exp.top_first]
    for g, e, name in zip(got, want, OUTS):
        if g is not None:
            assert np.array_equal(g, e), (what, name, np.flatnonzero(g != e)[:10])


SUBSETS = list(itertools.product((False, True), repeat=5))          # every subset of the five outputs


@pytest.mark.parametrize("name", list(CASES))
def test_every_case_equals_the_reference(jt, enc, name):
    """All five outputs in both modes, after device-input and host-input encodes, at the default and at the smallest table budget,
    with guards around every buffer."""
    N = jt._native
    case = CASES[name]
    for via in ("device", "host"):
        b = encode(jt, enc, case.docs, case.route, via)
        tok_off = check_ids(b, case.docs, case.route)
        for mark_first in (False, True):
            ids, status, exp = ref(case, mark_first)
            got = run(b, case, mark_first)
            same(got, exp, status, tok_off, (name, via, mark_first))
            b.set_option(N.JTK_OPT_REPEAT_TABLE_BYTES, N.JTK_RP_MIN_TABLE_BYTES)
            small = run(b, case, mark_first)
            b.set_option(N.JTK_OPT_REPEAT_TABLE_BYTES, 256 << 20)
            assert all(np.array_equal(x, y) for x, y in zip(got, small)), (name, via, mark_first, "the smallest budget")
        # unaligned flag buffers; each subset of outputs; outputs that are not asked for are not written
        mark_first = via == "host"
        ids, status, exp = ref(case, mark_first)
        for shift in (1, 4, 7):
            same(run(b, case, mark_first, want=(True, False, False, False, False), shift=shift), exp, status, tok_off, (name, via, shift))
        for want in SUBSETS:
            same(run(b, case, mark_first, want=want), exp, status, tok_off, (name, via, want))
        assert np.array_equal(check_ids(b, case.docs, case.route), tok_off)     # the pass left the encode's result alone
        b.close()


def test_a_callers_stream(jt, enc):
    import torch
    st = torch.cuda.Stream()
    for name in ("placement_n13", "grouping_n2", "periods_n2"):
        case = CASES[name]
        ids, status, exp = ref(case, True)
        b = encode(jt, enc, case.docs, case.route, "device", stream=st.cuda_stream)
        got = run(b, case, True, stream=st.cuda_stream)
        tok_off = check_ids(b, case.docs, case.route)
        same(got, exp, status, tok_off, name)
        # the batch's table is reused from the batch's own stream, then from the caller's again: the calls take effect in order
        same(run(b, case, True), exp, status, tok_off, (name, "own stream"))
        same(run(b, case, False, stream=st.cuda_stream), ref(case, False)[2], status, tok_off, (name, "caller's stream again"))
        b.close()


def test_shard_property(jt, enc):
    """Documents [cut:] encoded alone with doc_index_base = cut give exactly the rows and flags of the whole batch."""
    docs = CASES["periods_n2"].docs + CASES["same_across_docs_n2"].docs + CASES["grouping_n2"].docs + CASES["straddle_n2"].docs
    case = rc.Case("shards", 2, 77, 0, docs, "ordinary")
    b = encode(jt, enc, docs, "ordinary", "device")
    tok_off = check_ids(b, docs, "ordinary")
    whole = run(b, case, True)
    ids, status = rc.ids_of(docs, "ordinary")
    same(whole, rr.repeats(ids, status, 2, 77, 0, True), status, tok_off, "whole")
    assert whole[1].sum() > 0
    b.close()
    for cut in (1, len(docs) // 2, len(docs) - 2):
        b = encode(jt, enc, docs[cut:], "ordinary", "device")
        part = run(b, case, True, base=cut)
        assert np.array_equal(part[0], whole[0][tok_off[cut]:]), cut
        assert all(np.array_equal(p, w[cut:]) for p, w in zip(part[1:], whole[1:])), cut
        b.close()


def test_invalid_arguments(jt, enc):
    import torch
    N = jt._native
    L = N.lib()
    E = N.JTK_ERR_INVALID_ARGUMENT
    case = CASES["periods_n13"]
    ids, status, exp = ref(case, False)
    text, doc_off = pack(case.docs)
    nd = len(case.docs)
    b = enc.new_batch()
    flags_t = torch.full((4096,), GUARD8, dtype=torch.uint8, device="cuda")
    i32 = torch.full((nd + 8,), GUARD32, dtype=torch.int32, device="cuda")
    i64 = torch.full((nd + 8,), GUARD64, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    good = N.RepeatParamsStruct(0, 0, 13, 0)

    def call(bh, p=good, f=flags_t.data_ptr(), a=i32.data_ptr(), c=i32.data_ptr(), t=i32.data_ptr(), g=i64.data_ptr()):
        rc_ = L.jtk_batch_ngram_repeats(bh, C.byref(p) if p is not None else None, f, a, c, t, g, None)
        assert rc_ == N.JTK_OK or N.last_error()
        return rc_

    assert call(b._h) == E                                                                        # before any encode
    b.encode_host(text, doc_off, ordinary=True, count_only=True)
    assert call(b._h) == E and "count-only" in N.last_error()                                     # after a count-only encode
    b.encode_host(text, doc_off, ordinary=True)
    b.chunk(100, 10)
    b.pack(64)

    def minhash():
        sig = torch.zeros((nd, 64), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        b.minhash(sig.data_ptr(), 5, 64, 0, 3)
        torch.cuda.synchronize()
        return sig.cpu().numpy()

    before = (b.chunk_fetch(), b.pack_fetch(), b.fetch(), minhash())
    for n, fl in ((0, 0), (33, 0), (-1, 0), (13, 2), (13, 3), (13, 1 << 31)):
        assert call(b._h, N.RepeatParamsStruct(0, 0, n, fl)) == E, (n, fl)
    assert call(None) == E and call(b._h, None) == E                                              # a NULL batch, NULL params
    for k in (1, 2, 3):                                                                           # misaligned int32 / int64 arrays
        assert call(b._h, a=i32.data_ptr() + k) == E and call(b._h, c=i32.data_ptr() + k) == E and call(b._h, t=i32.data_ptr() + k) == E
    for k in (1, 2, 4, 7):
        assert call(b._h, g=i64.data_ptr() + k) == E
    assert L.jtk_batch_set_option(b._h, N.JTK_OPT_REPEAT_TABLE_BYTES, N.JTK_RP_MIN_TABLE_BYTES - 1) == E
    torch.cuda.synchronize()
    for t, guard in ((flags_t, GUARD8), (i32, GUARD32), (i64, GUARD64)):
        assert (t.cpu().numpy() == guard).all()                                                   # a refused call wrote nothing
    # the pass still runs, and the other results of the encode are as they were
    same(run(b, case, False), exp, status, before[2].tok_off, "after the refusals")
    after = (b.chunk_fetch(), b.pack_fetch(), b.fetch(), minhash())
    for x, y in zip(before[:2], after[:2]):
        assert x.keys() == y.keys() and all(np.array_equal(x[k], y[k]) for k in x)
    assert all(np.array_equal(getattr(before[2], k), getattr(after[2], k)) for k in ("tokens", "tok_off", "status"))
    assert np.array_equal(before[3], after[3])
    b.close()


SENTENCES = ["The quick brown fox jumps over the lazy dog while the farmer counts seventeen sheep beside the old stone wall.",
             "Click here to subscribe to our newsletter and receive the latest offers straight to your inbox every week.",
             "Water boils at one hundred degrees Celsius at sea level, but the boiling point drops as altitude increases.",
             "In 1969 the Apollo 11 mission landed two astronauts on the Moon, and they returned safely four days later.",
             "Question: what is the capital of Australia? Answer: Canberra, a compromise between Sydney and Melbourne."]


def surface_batch():
    """40 documents of ordinary sentences: 10 have one sentence repeated 3 to 6 times inside them, 30 have none repeated."""
    filler = lambda i, l: rc.doc(l, 900 + i).decode()
    plan = []
    for i in range(10):
        s = SENTENCES[i % 5]
        plan.append((filler(i, 12 + i) + " " + " ".join([s] * (3 + i % 4)) + filler(20 + i, 9), True))
    for i in range(28):
        plan.append((" ".join(SENTENCES[(i + k) % 5] for k in range(1 + i % 4)) + filler(40 + i, 15 + 3 * i), False))
    plan += [("", False), ("short one", False)]
    order = [(7 * i + 3) % 40 for i in range(40)]                                                # (7 and 40 are coprime: a permutation)
    docs, repeated = [None] * 40, [False] * 40
    for src, at in enumerate(order):
        docs[at], repeated[at] = plan[src]
    return docs, repeated


def test_python_surface_on_the_40_document_batch(jt, enc):
    import torch
    N = jt._native
    docs, repeated = surface_batch()
    o = rc.oracle()
    ids = [o.encode_ordinary(d.encode()) for d in docs]
    status = [0] * 40
    n = 6
    exp = rr.repeats(ids, status, n, 5, 0, True)
    flags, n_rep, n_cov, top_count, top_first, tok_off = enc.ngram_repeats_batch(docs, n, seed=5, mark_first=True)
    assert flags.dtype == np.uint8 and n_rep.dtype == np.int32 and n_cov.dtype == np.int32 and top_count.dtype == np.int32
    assert top_first.dtype == np.int64 and tok_off.dtype == np.int64 and np.array_equal(tok_off, exp.tok_off)
    same((flags, n_rep, n_cov, top_count, top_first), exp, status, tok_off, "ngram_repeats_batch")
    text, doc_off = pack([d.encode() for d in docs])
    d_text, d_off = device_copy(text, doc_off)
    out = enc.ngram_repeats_batch_device(d_text[:len(text)], d_off, n, seed=5, mark_first=False, doc_index_base=9)
    torch.cuda.synchronize()
    assert [t.dtype for t in out] == [torch.uint8, torch.int32, torch.int32, torch.int32, torch.int64, torch.int64, torch.int32]
    assert out[5].cpu().numpy().tolist() == exp.tok_off.tolist() and (out[6].cpu().numpy() == 0).all()
    same([t.cpu().numpy() for t in out[:5]], rr.repeats(ids, status, n, 5, 9, False), status, tok_off, "ngram_repeats_batch_device")
    # the Gopher fractions against the oracle's ids and the decoded byte lengths
    sig = enc.repetition_signals(docs, mark_first=True)
    blen = [[len(o.decode_bytes([t])) for t in x] for x in ids]
    assert [sum(x) for x in blen] == [len(d.encode()) for d in docs]
    assert sig["n_tokens"].tolist() == [len(x) for x in ids] and sig["n_bytes"].tolist() == [len(d.encode()) for d in docs]
    assert sorted(sig["top"]) == [2, 3, 4] and sorted(sig["dup"]) == [5, 6, 7, 8, 9, 10]
    for k in (2, 3, 4):
        r = rr.repeats(ids, status, k, 0, 0, False)
        for d in range(40):
            l, nb, tc, tf = len(ids[d]), sum(blen[d]), int(r.top_count[d]), int(r.top_first[d])
            tok = Fraction(tc * k, l) if tc else Fraction(0)
            byt = Fraction(tc * sum(blen[d][tf:tf + k]), nb) if tc else Fraction(0)
            assert sig["top"][k][0][d] == float(tok) and sig["top"][k][1][d] == float(byt), (k, d)
    for k in (5, 6, 7, 8, 9, 10):
        r = rr.repeats(ids, status, k, 0, 0, True)
        for d in range(40):
            l, nb = len(ids[d]), sum(blen[d])
            cov = [bool(f & rr.COVERED) for f in r.flags[r.tok_off[d]:r.tok_off[d + 1]]]
            tok = Fraction(int(r.n_covered[d]), l) if l else Fraction(0)
            byt = Fraction(sum(x for x, c in zip(blen[d], cov) if c), nb) if nb else Fraction(0)
            assert sig["dup"][k][0][d] == float(tok) and sig["dup"][k][1][d] == float(byt), (k, d)
    # the 10 stand out from the 30
    for k in (5, 10):
        for which in (0, 1):
            f = sig["dup"][k][which]
            assert min(f[d] for d in range(40) if repeated[d]) > 0.5 > 0.0 == max(f[d] for d in range(40) if not repeated[d]), (k, which)
    times = [round(sig["top"][4][0][d] * len(ids[d]) / 4) for d in range(40)]                  # (top_count back out of the fraction)
    assert min(t for t, r in zip(times, repeated) if r) >= 3 and max(t for t, r in zip(times, repeated) if not r) <= 1
    later = enc.repetition_signals(docs, top=(), dup=(5,), mark_first=False)
    assert all(later["dup"][5][0][d] < sig["dup"][5][0][d] for d in range(40) if repeated[d]) and later["top"] == {}


def test_an_empty_batch(jt, enc):
    z = enc.ngram_repeats_batch([], 3)
    assert [len(a) for a in z] == [0, 0, 0, 0, 0, 1]
    e = enc.repetition_signals([])
    assert all(len(v[0]) == 0 and len(v[1]) == 0 for v in list(e["top"].values()) + list(e["dup"].values())) and len(e["n_tokens"]) == 0
    only_empty = enc.ngram_repeats_batch(["", ""], 3, mark_first=True)
    assert len(only_empty[0]) == 0 and only_empty[3].tolist() == [0, 0] and only_empty[4].tolist() == [-1, -1]
    s = enc.repetition_signals(["", ""])
    assert s["top"][2][0].tolist() == [0.0, 0.0] and s["dup"][10][1].tolist() == [0.0, 0.0]
