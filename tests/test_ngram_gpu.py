"""jtk_ngram_set_* / jtk_batch_ngram_overlap and the Python surface on them (NgramSet, Batch.ngram_overlap,
HipEncoding.ngram_set, ngram_overlap_batch, ngram_overlap_batch_device): every case of tests/ngram_cases.py through the C ABI,
the set's keys, count and capacity and the overlap's flags and per-document results equal to the plain restatement
tests/ngram_ref.py exactly -- the pass is integer arithmetic only.  The ids the restatement hashes are the CPU oracle's, and
every case first checks that the device's encodes left exactly those.  Every test here needs a real MI355X (`-m gpu`)."""
import ctypes as C

import numpy as np
import pytest

import ngram_cases as nc
import ngram_ref as nr

pytestmark = pytest.mark.gpu

GUARD8, GUARD32, GUARD64 = 0x5A, 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A
PAD = 4                                      # guard elements before every per-document output
PAD8 = 16                                    # guard bytes before the flags (the 8-byte alignment stays)
CASES = {c.name: c for c in nc.cases()}
_REF = {}


@pytest.fixture(scope="module")
def jt():
    import jtokkit_amd
    return jtokkit_amd


@pytest.fixture(scope="module")
def enc(jt):
    return jt.get_encoding("cl100k_base")


def ref(case):
    """(the reference set, the corpus ids, statuses, the reference's overlap), computed once and shared."""
    if case.name not in _REF:
        s, _ = nc.build_set(case)
        ids, status = nc.ids_of(case.docs, case.route)
        r = nr.overlap(ids, status, s)
        for a in (r.flags, r.n_hit, r.n_covered, r.first_hit):
            a.setflags(write=False)
        _REF[case.name] = (s, ids, status, r)
    return _REF[case.name]


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
        b.set_fim(jt.FimParams(0.5, 0.5, seed=nc.mc.FIM["seed"], doc_index_base=nc.mc.FIM["base"]))
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
    ids, status = nc.ids_of(docs, route)
    res = b.fetch()
    assert (np.sign(res.status) == np.sign(status)).all()
    assert [res.doc(d).tolist() for d in range(len(ids)) if status[d] >= 0] == [x for x, st in zip(ids, status) if st >= 0]
    return res.tok_off


def build(jt, enc, case, via, stream=None):
    """The case's set through the C ABI: every "texts" step an encode (checked against the oracle) and add_batch, every "keys"
    step an add_keys.  The source batches are closed before the set is used."""
    s = enc.ngram_set(case.n, case.seed)
    key = nr.key_of(case.seed, case.n)
    for kind, what, *route in case.steps:
        if kind == "texts":
            b = encode(jt, enc, what, route[0], via, stream)
            check_ids(b, what, route[0])
            s.add_last_encode(b, stream)
            b.close()
        else:
            s.add_keys(np.array([nr.k_of(nc.oracle().encode_ordinary(g), key) for g in what], dtype=np.uint64))
    return s


def same_set(s, exp, what):
    assert len(s) == len(exp.keys) and s.capacity == exp.capacity, (what, len(s), s.capacity, len(exp.keys), exp.capacity)
    got = s.keys()
    assert got.dtype == np.uint64 and np.array_equal(np.sort(got), np.array(sorted(exp.keys), dtype=np.uint64)), what


def run_overlap(b, s, stream=None, want=(True, True, True, True), shift=0):
    """jtk_batch_ngram_overlap into torch buffers with guards around every output; shift: bytes past the flags' 8-byte boundary.
    Returns (flags, n_hit, n_covered, first_hit), None for an output that was not asked for (its buffer is checked untouched)."""
    import torch
    nt, nd, _ = b.result()
    bufs = [torch.full((nt + 2 * PAD8 + shift,), GUARD8, dtype=torch.uint8, device="cuda"),
            torch.full((nd + 2 * PAD,), GUARD32, dtype=torch.int32, device="cuda"),
            torch.full((nd + 2 * PAD,), GUARD32, dtype=torch.int32, device="cuda"),
            torch.full((nd + 2 * PAD,), GUARD64, dtype=torch.int64, device="cuda")]
    lo = [PAD8 + shift, PAD, PAD, PAD]
    n = [nt, nd, nd, nd]
    torch.cuda.synchronize()                 # (the fills run on torch's stream, the pass on the batch's or the caller's)
    b.ngram_overlap(s, *[t.data_ptr() + l * t.element_size() if w else None for t, l, w in zip(bufs, lo, want)], stream=stream)
    torch.cuda.synchronize()
    out = []
    for t, l, k, w, guard in zip(bufs, lo, n, want, (GUARD8, GUARD32, GUARD32, GUARD64)):
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
    flags, n_hit, n_cov, first = got
    want = expected_on_device(exp, status, tok_off)
    if flags is not None:
        assert np.array_equal(flags, want), (what, np.flatnonzero(flags != want)[:10])
    for g, e, name in ((n_hit, exp.n_hit, "n_hit"), (n_cov, exp.n_covered, "n_covered"), (first, exp.first_hit, "first_hit")):
        if g is not None:
            assert np.array_equal(g, e), (what, name, np.flatnonzero(g != e)[:10])


@pytest.mark.parametrize("name", list(CASES))
def test_every_case_equals_the_reference(jt, enc, name):
    """The set and all four outputs, after device-input and host-input encodes, with guards around every buffer."""
    case = CASES[name]
    exp_set, ids, status, exp = ref(case)
    for via in ("device", "host"):
        s = build(jt, enc, case, via)
        same_set(s, exp_set, (name, via))
        b = encode(jt, enc, case.docs, case.route, via)
        tok_off = check_ids(b, case.docs, case.route)
        same(run_overlap(b, s), exp, status, tok_off, (name, via))
        # unaligned flag buffers; outputs that are not asked for are not written
        for shift in (1, 4, 7):
            same(run_overlap(b, s, want=(True, False, False, False), shift=shift), exp, status, tok_off, (name, via, shift))
        same(run_overlap(b, s, want=(False, True, False, False)), exp, status, tok_off, (name, via, "n_hit only"))
        same(run_overlap(b, s, want=(False, False, True, True)), exp, status, tok_off, (name, via, "no flags"))
        assert run_overlap(b, s, want=(False, False, False, False)) == [None] * 4
        assert np.array_equal(check_ids(b, case.docs, case.route), tok_off)     # the pass left the encode's result alone
        same_set(s, exp_set, (name, via, "after the overlaps"))
        b.close()
        s.close()


def test_a_callers_stream(jt, enc):
    import torch
    st = torch.cuda.Stream()
    for name in ("straddle_n13", "three_tiles_n13", "set_grow_batch"):
        case = CASES[name]
        exp_set, ids, status, exp = ref(case)
        s = build(jt, enc, case, "device", stream=st.cuda_stream)
        same_set(s, exp_set, name)
        b = encode(jt, enc, case.docs, case.route, "device", stream=st.cuda_stream)
        got = run_overlap(b, s, stream=st.cuda_stream)
        same(got, exp, status, check_ids(b, case.docs, case.route), name)
        # the same set read from the batch's own stream, then fed again from the caller's: the calls take effect in order
        same(run_overlap(b, s), exp, status, b.fetch().tok_off, (name, "own stream"))
        s.add_last_encode(b, st.cuda_stream)
        assert len(s) == len(exp_set.keys | set(nr.doc_keys(ids, status, case.seed, case.n)))
        b.close()
        s.close()


def test_invalid_arguments(jt, enc):
    import torch
    N = jt._native
    L = N.lib()
    E = N.JTK_ERR_INVALID_ARGUMENT
    case = CASES["lengths_n13"]
    exp_set, ids, status, exp = ref(case)
    h = C.c_void_p()
    for n, flags in ((0, 0), (33, 0), (-1, 0), (13, 1), (13, 1 << 31)):
        p = N.NgramParamsStruct(0, n, flags)
        assert L.jtk_ngram_set_create(enc._h, C.byref(p), C.byref(h)) == E and N.last_error() and not h.value, (n, flags)
    assert L.jtk_ngram_set_create(enc._h, None, C.byref(h)) == E
    s = build(jt, enc, case, "host")
    text, doc_off = pack(case.docs)
    nd = len(case.docs)
    b = enc.new_batch()
    flags_t = torch.full((4096,), GUARD8, dtype=torch.uint8, device="cuda")
    i32 = torch.full((nd + 8,), GUARD32, dtype=torch.int32, device="cuda")
    i64 = torch.full((nd + 8,), GUARD64, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()

    def overlap(bh, sh, f=flags_t.data_ptr(), a=i32.data_ptr(), c=i32.data_ptr(), g=i64.data_ptr()):
        rc = L.jtk_batch_ngram_overlap(bh, sh, f, a, c, g, None)
        assert rc == N.JTK_OK or N.last_error()
        return rc

    assert overlap(b._h, s._h) == E and L.jtk_ngram_set_add_batch(s._h, b._h, None) == E          # before any encode
    b.encode_host(text, doc_off, ordinary=True, count_only=True)
    assert overlap(b._h, s._h) == E and L.jtk_ngram_set_add_batch(s._h, b._h, None) == E          # after a count-only encode
    b.encode_host(text, doc_off, ordinary=True)
    assert overlap(b._h, None) == E and overlap(None, s._h) == E                                  # a NULL set, a NULL batch
    assert L.jtk_ngram_set_add_batch(None, b._h, None) == E and L.jtk_ngram_set_add_batch(s._h, None, None) == E
    for k in (1, 2, 3):                                                                           # misaligned int32 / int64 arrays
        assert overlap(b._h, s._h, a=i32.data_ptr() + k) == E and overlap(b._h, s._h, c=i32.data_ptr() + k) == E
    for k in (1, 2, 4, 7):
        assert overlap(b._h, s._h, g=i64.data_ptr() + k) == E
    other = jt.new_encoding("cl100k_base")                                                        # another encoding object
    ob = other.new_batch()
    ob.encode_host(text, doc_off, ordinary=True)
    assert overlap(ob._h, s._h) == E and "another encoding object" in N.last_error()
    assert L.jtk_ngram_set_add_batch(s._h, ob._h, None) == E and "another encoding object" in N.last_error()
    ob.close()
    other.close()
    keys = np.array([5, 6, 7], dtype=np.uint64)
    assert L.jtk_ngram_set_add_keys(s._h, keys.ctypes.data, -1) == E and L.jtk_ngram_set_add_keys(s._h, None, 3) == E
    assert L.jtk_ngram_set_add_keys(s._h, np.array([5, 0, 7], dtype=np.uint64).ctypes.data, 3) == E and "0" in N.last_error()
    assert L.jtk_ngram_set_add_keys(s._h, None, 0) == N.JTK_OK
    room = np.zeros(len(exp_set.keys), dtype=np.uint64)
    assert L.jtk_ngram_set_keys(s._h, room.ctypes.data, len(room) - 1) == E and L.jtk_ngram_set_keys(s._h, room.ctypes.data, -1) == E
    torch.cuda.synchronize()
    for t, guard in ((flags_t, GUARD8), (i32, GUARD32), (i64, GUARD64)):
        assert (t.cpu().numpy() == guard).all()                                                   # a refused call wrote nothing
    # the set and the batch are as they were, and the pass still runs on them
    same_set(s, exp_set, "after the refusals")
    same(run_overlap(b, s), exp, status, check_ids(b, case.docs, case.route), "after the refusals")
    b.close()
    s.close()


def test_shard_property(jt, enc):
    """keys() of a set built from a batch = the union of keys() of sets built from its halves; those keys loaded into a fresh
    set give identical overlap results."""
    src = CASES["three_tiles_n13"].docs + CASES["patterns_n13"].docs + CASES["lengths_n13"].docs
    corpus = CASES["patterns_n13"].docs + CASES["doc_ends"].docs + CASES["three_tiles_n13"].docs
    n, seed = 13, 77

    def set_of(docs):
        s = enc.ngram_set(n, seed)
        b = encode(jt, enc, docs, "ordinary", "device")
        s.add_last_encode(b)
        b.close()
        return s

    whole = set_of(src)
    ids, status = nc.ids_of(src, "ordinary")
    exp_set = nr.Set(seed, n)
    exp_set.add_docs(ids, status)
    same_set(whole, exp_set, "whole")
    b = encode(jt, enc, corpus, "ordinary", "device")
    want = run_overlap(b, whole)
    cids, cstatus = nc.ids_of(corpus, "ordinary")
    same(want, nr.overlap(cids, cstatus, exp_set), cstatus, b.fetch().tok_off, "whole")
    assert want[1].sum() > 0
    for cut in (1, len(src) // 2, len(src) - 2):
        halves = [set_of(src[:cut]), set_of(src[cut:])]
        k0, k1 = halves[0].keys(), halves[1].keys()
        assert set(k0.tolist()) | set(k1.tolist()) == set(whole.keys().tolist()), cut
        loaded = enc.ngram_set(n, seed)
        loaded.add_keys(k0)
        loaded.add_keys(k1)
        assert len(loaded) == len(whole)
        got = run_overlap(b, loaded)
        assert all(np.array_equal(g, w) for g, w in zip(got, want)), cut
        for s in halves + [loaded]:
            s.close()
    b.close()
    whole.close()


def test_the_set_outlives_its_source_batch(jt, enc):
    case = CASES["patterns_n13"]
    exp_set, ids, status, exp = ref(case)
    s = enc.ngram_set(case.n, case.seed)
    b = enc.new_batch()
    for _, docs, route in case.steps:
        encode(jt, enc, docs, route, "device", b=b)
        s.add_last_encode(b)
    # a later encode on the same batch, then its destruction
    encode(jt, enc, case.docs, case.route, "device", b=b)
    same_set(s, exp_set, "after a later encode")
    same(run_overlap(b, s), exp, status, b.fetch().tok_off, "same batch")
    b.close()
    same_set(s, exp_set, "after jtk_batch_destroy")
    b2 = encode(jt, enc, case.docs, case.route, "host")
    same(run_overlap(b2, s), exp, status, b2.fetch().tok_off, "another batch")
    b2.close()
    s.close()


def test_other_results_of_the_encode_stay_intact(jt, enc):
    """fetch, pack_fetch, chunk_fetch and minhash give the same before and after an overlap and an add_batch."""
    import torch
    case = CASES["three_tiles_n13"]
    exp_set, ids, status, exp = ref(case)
    s = build(jt, enc, case, "host")
    text, doc_off = pack(case.docs)
    b = enc.new_batch()
    b.encode_host(text, doc_off, ordinary=True)
    b.chunk(100, 10)
    b.pack(64)

    def minhash():
        sig = torch.zeros((len(case.docs), 64), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        b.minhash(sig.data_ptr(), 5, 64, 0, 3)
        torch.cuda.synchronize()
        return sig.cpu().numpy()

    before = (b.chunk_fetch(), b.pack_fetch(), b.fetch(), minhash())
    same(run_overlap(b, s), exp, status, before[2].tok_off, "overlap")
    s.add_last_encode(b)
    after = (b.chunk_fetch(), b.pack_fetch(), b.fetch(), minhash())
    for x, y in zip(before[:2], after[:2]):
        assert x.keys() == y.keys() and all(np.array_equal(x[k], y[k]) for k in x)
    assert all(np.array_equal(getattr(before[2], k), getattr(after[2], k)) for k in ("tokens", "tok_off", "status"))
    assert np.array_equal(before[3], after[3])
    b.close()
    s.close()


PASSAGES = ["The quick brown fox jumps over the lazy dog while the farmer counts seventeen sheep beside the old stone wall near the river.",
            "In 1969 the Apollo 11 mission landed two astronauts on the Moon, and they returned safely to Earth four days later with rock samples.",
            "def fibonacci(n):\n    a, b = 0, 1\n    for _ in range(n):\n        a, b = b, a + b\n    return a  # iterative version",
            "Water boils at one hundred degrees Celsius at sea level, but the boiling point drops as altitude increases and pressure falls.",
            "Question: what is the capital of Australia? Answer: Canberra, which was chosen as a compromise between Sydney and Melbourne."]


def surface_batch():
    """40 documents: each passage mid-document, at a document's start and at its end, among 25 unrelated ones."""
    plan = []
    for i, p in enumerate(PASSAGES):
        plan += [nc.doc(40 + i, 800 + i).decode() + " " + p + nc.doc(25, 810 + i).decode(), p + nc.doc(30 + i, 820 + i).decode(),
                 nc.doc(35, 830 + i).decode() + " " + p]
    plan += [nc.doc(20 + 7 * i, 840 + i).decode() for i in range(23)] + ["", "short one"]
    order = [(7 * i + 3) % 40 for i in range(40)]                                                # (7 and 40 are coprime: a permutation)
    docs = [None] * 40
    embeds = [False] * 40
    for src, at in enumerate(order):
        docs[at], embeds[at] = plan[src], src < 15
    return docs, embeds


def test_python_surface_on_the_40_document_batch(jt, enc):
    import torch
    N = jt._native
    n = 13
    docs, embeds = surface_batch()
    o = nc.oracle()
    ids = [o.encode_ordinary(d.encode()) for d in docs]
    status = [0] * 40
    exp_set = nr.Set(0, n)
    exp_set.add_docs([o.encode_ordinary(p.encode()) for p in PASSAGES], [0] * 5)
    exp = nr.overlap(ids, status, exp_set)
    s = enc.ngram_set(n)
    res = s.add_texts(PASSAGES)
    assert [res.doc(d).tolist() for d in range(5)] == [o.encode_ordinary(p.encode()) for p in PASSAGES]
    assert len(s) == len(exp_set.keys) > 5 * 10 and s.capacity == exp_set.capacity and s.ngram == n and s.seed == 0
    flags, n_hit, n_cov, first, tok_off = enc.ngram_overlap_batch(docs, s)
    assert flags.dtype == np.uint8 and n_hit.dtype == np.int32 and n_cov.dtype == np.int32 and first.dtype == np.int64 and tok_off.dtype == np.int64
    assert np.array_equal(tok_off, exp.tok_off)
    same((flags, n_hit, n_cov, first), exp, status, tok_off, "ngram_overlap_batch")
    for d in range(40):
        f = flags[tok_off[d]:tok_off[d + 1]]
        covered = np.flatnonzero(f & N.JTK_NG_COVERED)
        if embeds[d]:
            # one run of covered tokens, from the first start to n - 1 past the last: the passage but for retokenized ends
            assert n_hit[d] > 0 and first[d] == covered[0] and len(covered) == n_cov[d] == covered[-1] - covered[0] + 1 >= n
            assert covered[-1] == np.flatnonzero(f & N.JTK_NG_START)[-1] + n - 1
            got = enc.decode(ids[d][covered[0]:covered[-1] + 1])
            assert got in docs[d] and any(got.strip() in p and len(got) > len(p) - 12 for p in PASSAGES), (d, got)
        else:
            assert n_hit[d] == 0 and n_cov[d] == 0 and first[d] == -1 and not f.any()
    # bytes in, the device form, and a second set loaded from the first one's keys
    text, doc_off = pack([d.encode() for d in docs])
    d_text, d_off = device_copy(text, doc_off)
    loaded = enc.ngram_set(n)
    loaded.add_keys(s.keys())
    out = enc.ngram_overlap_batch_device(d_text[:len(text)], d_off, loaded)
    torch.cuda.synchronize()
    d_flags, d_hit, d_cov, d_first, d_tok_off, d_status = out
    assert d_flags.dtype == torch.uint8 and d_hit.dtype == torch.int32 and d_cov.dtype == torch.int32 and d_first.dtype == torch.int64
    assert d_tok_off.cpu().numpy().tolist() == exp.tok_off.tolist() and (d_status.cpu().numpy() == 0).all()
    same([t.cpu().numpy() for t in (d_flags, d_hit, d_cov, d_first)], exp, status, tok_off, "ngram_overlap_batch_device")
    # an empty set, and an empty batch
    empty = enc.ngram_set(n, seed=5)
    assert len(empty) == 0 and empty.capacity == 64 and len(empty.keys()) == 0
    e = enc.ngram_overlap_batch(docs, empty)
    assert not e[0].any() and not e[1].any() and not e[2].any() and (e[3] == -1).all()
    z = enc.ngram_overlap_batch([], s)
    assert [len(a) for a in z] == [0, 0, 0, 0, 1]
    for x in (s, loaded, empty):
        x.close()
