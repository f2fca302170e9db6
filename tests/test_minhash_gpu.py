"""jtk_batch_minhash / jtk_batch_minhash_agree and the Python surface on them (Batch.minhash, Batch.minhash_agree,
HipEncoding.minhash_batch, minhash_batch_device, near_duplicates): every case of tests/minhash_cases.py through the C ABI,
signatures, shingle counts, band keys and agreement equal to the plain restatement tests/minhash_ref.py exactly -- the pass is
integer arithmetic only.  The ids the restatement hashes are the CPU oracle's, and every case first checks that the device's
encode left exactly those.  Every test here needs a real MI355X (`-m gpu`)."""
import ctypes as C

import numpy as np
import pytest

import minhash_cases as mc
import minhash_ref as mr

pytestmark = pytest.mark.gpu

GUARD32 = 0x5A5A5A5A
GUARD64 = 0x5A5A5A5A5A5A5A5A
PAD = 4                                      # guard elements before every output (16 or 32 bytes: the alignment stays)
CASES = {c.name: c for c in mc.cases()}
RUNS = [(c.name, p) for c in mc.cases() for p in c.params]
_IDS, _REF = {}, {}


@pytest.fixture(scope="module")
def jt():
    import jtokkit_amd
    return jtokkit_amd


@pytest.fixture(scope="module")
def enc(jt):
    return jt.get_encoding("cl100k_base")


def ids_of(case):
    if case.name not in _IDS:
        _IDS[case.name] = mc.expected_ids(case)
    return _IDS[case.name]


def ref(case, params):
    """The reference's result for a case and one parameter set, computed once and shared."""
    if (case.name, params) not in _REF:
        n, K, bands, seed = params
        r = mr.minhash(ids_of(case)[0], seed, n, K, bands)
        for a in (r.sig, r.n_shingles) + ((r.band_keys,) if bands else ()):
            a.setflags(write=False)
        _REF[(case.name, params)] = r
    return _REF[(case.name, params)]


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


def encode_case(jt, enc, case, via, stream=None):
    """A fresh batch holding the case's encode by its route, through host or device input; the device arrays are kept alive on it."""
    N = jt._native
    b = enc.new_batch()
    route = case.route
    kw = dict(ordinary=route != "encode" and route != "allow_special")
    if route == "validate":
        kw["validate"] = True
    if route == "allow_special":
        b.set_allowed_special("all")
        kw["allow_special"] = True
    if route == "fim":
        b.set_fim(jt.FimParams(0.5, 0.5, seed=mc.FIM["seed"], doc_index_base=mc.FIM["base"]))
        kw["fim"] = True
    if route == "chunked":
        b.set_option(N.JTK_OPT_CHUNK_BYTES if via == "device" else N.JTK_OPT_HOST_CHUNK_BYTES, mc.CHUNK_BYTES)
    text, doc_off = pack(case.docs)
    if via == "host":
        b.encode_host(text, doc_off, **kw)
    else:
        b._keep = device_copy(text, doc_off)
        b.encode_device(b._keep[0].data_ptr(), b._keep[1].data_ptr(), len(case.docs), len(text), stream=stream, **kw)
    return b


def check_ids(b, case):
    """The device holds the ids the restatement hashes; a refused document has a negative status (and whatever tokens the
    encode left it: the pass must not look at them)."""
    ids, status = ids_of(case)
    res = b.fetch()
    assert (np.sign(res.status) == np.sign(status)).all()
    assert [res.doc(d).tolist() for d in range(len(ids)) if status[d] >= 0] == [x for x, st in zip(ids, status) if st >= 0]


def run_pass(b, params, stream=None, want_nsh=True, want_keys=True, shift=0):
    """jtk_batch_minhash into torch buffers with guard words around every output; shift: elements past the 16-byte boundary."""
    import torch
    n, K, bands, seed = params
    nd = b.result()[1]
    sig_t = torch.full((nd * K + 2 * PAD + shift,), GUARD32, dtype=torch.int32, device="cuda")
    nsh_t = torch.full((nd + 2 * PAD + shift,), GUARD32, dtype=torch.int32, device="cuda")
    key_t = torch.full((nd * bands + 2 * PAD + shift,), GUARD64, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()                 # (the fills run on torch's stream, the pass on the batch's or the caller's)
    b.minhash(sig_t.data_ptr() + 4 * (PAD + shift), n, K, bands, seed, nsh_t.data_ptr() + 4 * (PAD + shift) if want_nsh else None,
              key_t.data_ptr() + 8 * (PAD + shift) if bands and want_keys else None, stream)
    torch.cuda.synchronize()
    sig, nsh, keys = sig_t.cpu().numpy().view(np.uint32), nsh_t.cpu().numpy(), key_t.cpu().numpy().view(np.uint64)
    lo = PAD + shift
    assert (sig[:lo] == GUARD32).all() and (sig[lo + nd * K:] == GUARD32).all()
    assert (nsh[:lo] == GUARD32).all() and (nsh[lo + nd:] == GUARD32).all()
    assert (keys[:lo] == GUARD64).all() and (keys[lo + nd * bands:] == GUARD64).all()
    if not want_nsh:
        assert (nsh == GUARD32).all()
    if not (bands and want_keys):
        assert (keys == GUARD64).all()
    return sig[lo:lo + nd * K].reshape(nd, K), nsh[lo:lo + nd], keys[lo:lo + nd * bands].reshape(nd, bands) if bands else None


def run_agree(b, sig, pairs, shift=0, stream=None):
    import torch
    sig = np.ascontiguousarray(sig, dtype=np.uint32)
    n_sig, K = sig.shape
    sig_t = torch.zeros(sig.size + 4 + shift, dtype=torch.int32, device="cuda")
    sig_t[shift:shift + sig.size].copy_(torch.from_numpy(sig.view(np.int32).ravel().copy()))
    pa = torch.tensor([p for p, _ in pairs] + [0], dtype=torch.int64, device="cuda")
    pb = torch.tensor([q for _, q in pairs] + [0], dtype=torch.int64, device="cuda")
    out = torch.full((len(pairs) + 2 * PAD,), GUARD32, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    b.minhash_agree(sig_t.data_ptr() + 4 * shift, n_sig, K, pa.data_ptr(), pb.data_ptr(), len(pairs), out.data_ptr() + 4 * PAD, stream)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[:PAD] == GUARD32).all() and (got[PAD + len(pairs):] == GUARD32).all()
    return got[PAD:PAD + len(pairs)]


def same(got, exp, bands, what):
    sig, nsh, keys = got
    assert np.array_equal(nsh, exp.n_shingles), (what, np.flatnonzero(nsh != exp.n_shingles)[:10])
    assert np.array_equal(sig, exp.sig), (what, np.flatnonzero((sig != exp.sig).any(axis=1))[:10])
    if bands:
        assert np.array_equal(keys, exp.band_keys), (what, np.flatnonzero((keys != exp.band_keys).any(axis=1))[:10])


@pytest.mark.parametrize("name", list(CASES))
def test_every_case_equals_the_reference(jt, enc, name):
    """All four outputs, after a device-input and a host-input encode, with guard words around every buffer."""
    case = CASES[name]
    for via in ("device", "host"):
        b = encode_case(jt, enc, case, via)
        check_ids(b, case)
        for params in case.params:
            exp = ref(case, params)
            same(run_pass(b, params), exp, params[2], (name, via, params))
        params = case.params[0]
        exp = ref(case, params)
        # outputs that are not asked for are not written; buffers that are only 4- and 8-byte aligned
        assert np.array_equal(run_pass(b, params, want_nsh=False, want_keys=False, shift=1)[0], exp.sig), (name, via, "sig only")
        pairs = mc.agree_pairs(len(case.docs))
        want = mr.agree(exp.sig, [p for p, _ in pairs], [q for _, q in pairs])
        for shift in (0, 1):
            assert np.array_equal(run_agree(b, exp.sig, pairs, shift), want), (name, via, shift)
        check_ids(b, case)                                               # the pass left the encode's result alone
        b.close()


@pytest.mark.parametrize("K", mc.HASH_COUNTS)
def test_agreement_pairs(jt, enc, K):
    """a == b, both orders, indices of -1 and n_sig, and no pairs at all; rows that agree on none, some and all columns."""
    rng = np.random.RandomState(K)
    sig = rng.randint(0, 4, size=(9, K)).astype(np.uint32) * np.uint32(0x40000001)
    sig[3] = sig[5]
    sig[7] = ~sig[6]
    b = enc.new_batch()                                                  # (no encode: the call needs none)
    pairs = mc.agree_pairs(9) + [(3, 5), (6, 7), (7, 6), (8, 4), (9, 9), (-1, -1), (1 << 40, 0)]
    want = mr.agree(sig, [p for p, _ in pairs], [q for _, q in pairs])
    assert want[0] == K and -1 in want and want[len(mc.agree_pairs(9))] == K and want[len(mc.agree_pairs(9)) + 1] == 0
    for shift in (0, 1, 2):
        assert np.array_equal(run_agree(b, sig, pairs, shift), want), shift
    assert len(run_agree(b, sig, [])) == 0
    N = jt._native
    assert N.lib().jtk_batch_minhash_agree(b._h, None, 0, K, None, None, 0, None, None) == N.JTK_OK
    b.close()


def test_a_callers_stream(jt, enc):
    import torch
    case = CASES["three_tiles"]
    s = torch.cuda.Stream()
    b = encode_case(jt, enc, case, "device", stream=s.cuda_stream)
    for params in case.params[:3] + case.params[-2:]:
        same(run_pass(b, params, stream=s.cuda_stream), ref(case, params), params[2], params)
    exp = ref(case, case.params[0])
    pairs = mc.agree_pairs(len(case.docs))
    assert np.array_equal(run_agree(b, exp.sig, pairs, stream=s.cuda_stream), mr.agree(exp.sig, [p for p, _ in pairs], [q for _, q in pairs]))
    b.close()


def test_invalid_arguments(jt, enc):
    import torch
    N = jt._native
    L = N.lib()
    case = CASES["lengths_n5"]
    text, doc_off = pack(case.docs)
    nd = len(case.docs)
    sig = torch.full((nd * 256 + 8,), GUARD32, dtype=torch.int32, device="cuda")
    keys = torch.full((nd * 256 + 8,), GUARD64, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()

    def call(b, n, K, bands, flags=0, d_sig=sig.data_ptr(), p=True):
        ps = N.MinhashParamsStruct(0, n, K, bands, flags)
        return L.jtk_batch_minhash(b._h, C.byref(ps) if p else None, d_sig, None, keys.data_ptr(), None)

    b = enc.new_batch()
    assert call(b, 5, 128, 16) == N.JTK_ERR_INVALID_ARGUMENT             # before any encode
    b.encode_host(text, doc_off, ordinary=True, count_only=True)
    assert call(b, 5, 128, 16) == N.JTK_ERR_INVALID_ARGUMENT             # after a count-only encode
    b.encode_host(text, doc_off, ordinary=True)
    for n, K, bands, flags in ((0, 128, 0, 0), (33, 128, 0, 0), (-5, 128, 0, 0), (5, 0, 0, 0), (5, 257, 0, 0), (5, -1, 0, 0),
                               (5, 128, -1, 0), (5, 128, 3, 0), (5, 100, 128, 0), (5, 63, 2, 0), (5, 128, 16, 1), (5, 128, 0, 1 << 31)):
        assert call(b, n, K, bands, flags) == N.JTK_ERR_INVALID_ARGUMENT, (n, K, bands, flags)
    assert call(b, 5, 128, 16, p=False) == N.JTK_ERR_INVALID_ARGUMENT
    assert call(b, 5, 128, 16, d_sig=None) == N.JTK_ERR_INVALID_ARGUMENT
    assert call(b, 5, 128, 16, d_sig=sig.data_ptr() + 2) == N.JTK_ERR_INVALID_ARGUMENT
    pa = torch.zeros(4, dtype=torch.int64, device="cuda")
    out = torch.zeros(4, dtype=torch.int32, device="cuda")
    for K in (0, 257, -1):
        assert L.jtk_batch_minhash_agree(b._h, sig.data_ptr(), nd, K, pa.data_ptr(), pa.data_ptr(), 4, out.data_ptr(), None) == N.JTK_ERR_INVALID_ARGUMENT
    assert L.jtk_batch_minhash_agree(b._h, sig.data_ptr(), -1, 128, pa.data_ptr(), pa.data_ptr(), 4, out.data_ptr(), None) == N.JTK_ERR_INVALID_ARGUMENT
    assert L.jtk_batch_minhash_agree(b._h, sig.data_ptr(), nd, 128, pa.data_ptr(), pa.data_ptr(), -1, out.data_ptr(), None) == N.JTK_ERR_INVALID_ARGUMENT
    assert L.jtk_batch_minhash_agree(b._h, sig.data_ptr(), nd, 128, None, pa.data_ptr(), 4, out.data_ptr(), None) == N.JTK_ERR_INVALID_ARGUMENT
    assert L.jtk_batch_minhash_agree(b._h, sig.data_ptr(), nd, 128, pa.data_ptr(), pa.data_ptr(), 4, None, None) == N.JTK_ERR_INVALID_ARGUMENT
    torch.cuda.synchronize()
    assert (sig.cpu().numpy() == GUARD32).all() and (keys.cpu().numpy() == GUARD64).all()      # a refused call wrote nothing
    # the batch is as it was, and the pass still runs on it
    check_ids(b, case)
    same(run_pass(b, case.params[0]), ref(case, case.params[0]), case.params[0][2], "after the refusals")
    b.close()


def test_other_results_of_the_encode_stay_intact(jt, enc):
    """fetch, pack_fetch and chunk_fetch give the same before and after the pass."""
    case = CASES["three_tiles"]
    text, doc_off = pack(case.docs)
    b = enc.new_batch()
    b.encode_host(text, doc_off, ordinary=True)
    b.chunk(100, 10)
    b.pack(64)
    before = (b.chunk_fetch(), b.pack_fetch(), b.fetch())
    for params in case.params[:2]:
        same(run_pass(b, params), ref(case, params), params[2], params)
    after = (b.chunk_fetch(), b.pack_fetch(), b.fetch())
    for x, y in zip(before[:2], after[:2]):
        assert x.keys() == y.keys() and all(np.array_equal(x[k], y[k]) for k in x)
    assert all(np.array_equal(getattr(before[2], k), getattr(after[2], k)) for k in ("tokens", "tok_off", "status"))
    b.close()


def test_python_surface_on_the_40_document_batch(jt, enc):
    import torch
    docs, labels = mc.near_dup_batch()
    o = mc.oracle()
    ids = [o.encode_ordinary(d) for d in docs]
    P = mc.NEAR
    exp = mr.minhash(ids, P["seed"], P["ngram"], P["num_hashes"], P["bands"])
    sig, nsh, keys = enc.minhash_batch(docs, ngram=P["ngram"], num_hashes=P["num_hashes"], bands=P["bands"], seed=P["seed"])
    assert sig.dtype == np.uint32 and nsh.dtype == np.int32 and keys.dtype == np.uint64
    same((sig, nsh, keys), exp, P["bands"], "minhash_batch")
    sig0, nsh0, none = enc.minhash_batch([d.decode() for d in docs], ngram=P["ngram"], num_hashes=P["num_hashes"], seed=P["seed"])
    assert none is None and np.array_equal(sig0, exp.sig) and np.array_equal(nsh0, exp.n_shingles)
    text, doc_off = pack(docs)
    d_text, d_off = device_copy(text, doc_off)
    out = enc.minhash_batch_device(d_text[:len(text)], d_off, ngram=P["ngram"], num_hashes=P["num_hashes"], bands=P["bands"], seed=P["seed"])
    d_sig, d_nsh, d_keys, d_tok_off, d_status = out
    torch.cuda.synchronize()
    assert d_sig.dtype == torch.int32 and d_sig.shape == (40, P["num_hashes"]) and d_keys.dtype == torch.int64 and d_keys.shape == (40, P["bands"])
    same((d_sig.cpu().numpy().view(np.uint32), d_nsh.cpu().numpy(), d_keys.cpu().numpy().view(np.uint64)), exp, P["bands"], "minhash_batch_device")
    assert d_tok_off.cpu().numpy().tolist() == np.concatenate([[0], np.cumsum([len(x) for x in ids])]).tolist()
    assert (d_status.cpu().numpy() == 0).all()
    assert enc.minhash_batch_device(d_text[:len(text)], d_off, ngram=P["ngram"], num_hashes=P["num_hashes"], seed=P["seed"])[2] is None
    # the clusters: equal to the reference's procedure, which the CPU tier holds to the expected partition
    want = mr.near_duplicates(ids, P["threshold"], P["seed"], P["ngram"], P["num_hashes"], P["bands"])
    got = enc.near_duplicates(docs, threshold=P["threshold"], ngram=P["ngram"], num_hashes=P["num_hashes"], bands=P["bands"], seed=P["seed"])
    assert got.dtype == np.int64 and np.array_equal(got, want) and np.array_equal(got, labels)
    # a threshold nothing reaches but exact copies
    strict = enc.near_duplicates(docs, threshold=1.0, ngram=P["ngram"], num_hashes=P["num_hashes"], bands=P["bands"], seed=P["seed"])
    assert np.array_equal(strict, mr.near_duplicates(ids, 1.0, P["seed"], P["ngram"], P["num_hashes"], P["bands"]))
    assert len(set(strict.tolist())) == 40 - 3
    assert enc.near_duplicates([]).tolist() == [] and enc.near_duplicates(["one"]).tolist() == [0]
    assert enc.near_duplicates(["", "", ""]).tolist() == [0, 1, 2]


def test_shard_independence(jt, enc):
    """The signatures of a batch equal those of its two halves encoded separately."""
    case = CASES["three_tiles"]
    docs = CASES["doc_edges"].docs + case.docs + CASES["lengths_n5"].docs
    params = (5, 128, 16, 99)
    whole = mc.Case("whole", docs, "ordinary", [params])
    b = encode_case(jt, enc, whole, "device")
    sig, nsh, keys = run_pass(b, params)
    b.close()
    exp = mr.minhash([mc.oracle().encode_ordinary(d) for d in docs], 99, 5, 128, 16)
    same((sig, nsh, keys), exp, 16, "whole")
    for cut in (1, len(docs) // 2, 7):
        parts = []
        for half in (docs[:cut], docs[cut:]):
            b = encode_case(jt, enc, mc.Case("half", half, "ordinary", [params]), "device")
            parts.append(run_pass(b, params))
            b.close()
        for k in range(3):
            assert np.array_equal(np.concatenate([parts[0][k], parts[1][k]]), (sig, nsh, keys)[k]), (cut, k)
