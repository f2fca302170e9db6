"""jtk_batch_minhash_cluster and the Python surface on it: hand-made signature and key matrices uploaded directly, labels and
representatives equal to the plain restatement tests/cluster_ref.py exactly.  Every test here needs a real MI355X (`-m gpu`)."""
import math

import numpy as np
import pytest

import cluster_ref as cr
import minhash_cases as mc

pytestmark = pytest.mark.gpu

GUARD = 0x5A5A5A5A5A5A5A5A
PAD = 4


def blank(n, K, B, seed=1):
    """n documents that share nothing: random rows, and keys that are distinct over the whole matrix (an odd multiplier)."""
    sig = np.random.default_rng(seed).integers(0, 1 << 32, size=(n, K), dtype=np.uint64).astype(np.uint32)
    keys = (np.arange(1, n * B + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)).reshape(n, B)
    return sig, keys


def link(sig, keys, e, d, j, agree):
    """d joins e's bucket of band j; its row equals e's in exactly the first `agree` columns."""
    keys[d, j] = keys[e, j]
    sig[d] = sig[e] ^ np.uint32(1)
    sig[d, :agree] = sig[e, :agree]


def flat(n, K=4, B=2):
    sig, keys = blank(n, K, B)
    sig[:], keys[:] = sig[:1], keys[:1]
    return sig, keys


def build_cases():                                           # name -> (sig, band_keys, n_shingles or None, min_agree)
    c = {"n0": blank(0, 4, 2) + (None, 4), "n1": blank(1, 4, 2) + (None, 4), "n2_equal": flat(2) + (None, 4), "n2_unequal": blank(2, 4, 2) + (None, 4)}
    for K in (1, 4, 63, 64, 65, 100, 256):
        for m in sorted({1, K}):
            sig, keys = blank(6, K, 2, K)
            link(sig, keys, 0, 1, 0, m)                      # exactly min_agree
            link(sig, keys, 2, 3, 1, m - 1)                  # one short
            link(sig, keys, 4, 5, 1, K)
            c["K%d_m%d" % (K, m)] = (sig, keys, None, m)
    for B in (1, 16, 64, 65, 256):                           # the band loop at the wave width: a pair in the last band, one in the first
        sig, keys = blank(5, 4, B, B)
        link(sig, keys, 0, 1, B - 1, 4)
        link(sig, keys, 2, 3, 0, 4)
        c["B%d" % B] = (sig, keys, None, 4)
    for extra in (False, True):                              # a ~ b, b ~ c, not a ~ c at min_agree 2, in one bucket
        sig, keys = blank(3, 4, 2)
        sig[:] = [[1, 2, 3, 4], [1, 2, 9, 9], [7, 8, 9, 9]]
        keys[1, 0] = keys[2, 0] = keys[0, 0]
        if extra:
            keys[2, 1] = keys[1, 1]                          # b and c share another bucket without a
        c["chain3_extra_band" if extra else "chain3"] = (sig, keys, None, 2)
    sig, keys = blank(200, 8, 16)
    for i in range(1, 200):                                  # i meets i - 1 in band i mod 16 only, and differs from it in one column
        keys[i, i % 16] = keys[i - 1, i % 16]
        sig[i] = sig[i - 1]
        sig[i, i % 8] += 1
    c["chain200"] = (sig, keys, None, 7)
    sig, keys = blank(1000, 4, 2)
    sig[:], keys[:, 0] = sig[:1], keys[0, 0]
    c["star1000"] = (sig, keys, None, 4)
    sig, keys = blank(600, 8, 3)
    for lo, cols in ((0, slice(0, 4)), (500, slice(4, 8))):
        sig[lo:lo + 100, cols], keys[lo:lo + 100, 0] = sig[lo, cols], keys[lo, 0]
    sig[599, :4], keys[599, 1] = sig[50, :4], keys[50, 1]    # the late pair (50, 599): 500's component relabels to 0
    c["two_components"] = (sig, keys, None, 4)
    c["bucket300"] = flat(300, 64, 65) + (None, 64)          # one representative in every band: the in-wave de-duplication
    sig, keys = flat(8)
    keys[:] = blank(8, 4, 2)[1]
    keys[0, 0] = keys[1, 0] = keys[4, 1] = 0                 # 4 has the value in the other band: no pair
    keys[2, 0] = keys[3, 0] = keys[5, 1] = 0xFFFFFFFFFFFFFFFF
    keys[6, 0] = keys[7, 1] = 12345                          # one value in two bands of two documents: no pair
    c["edge_keys"] = (sig, keys, None, 4)
    sig, keys = blank(40, 4, 2)                              # capacity 128: every key of band 0 has the home slot 126
    keys[:, 0] = ((np.arange(40, dtype=np.uint64) // np.uint64(2) + np.uint64(1)) << np.uint64(32)) | np.uint64(126)
    sig[1::2] = sig[0::2]                                    # pairs (2 k, 2 k + 1) along a run that wraps the table's end
    c["probe_runs"] = (sig, keys, None, 4)
    c["not_live"] = flat(6) + (np.array([0, 5, 0, 5, 5, -1], dtype=np.int32), 4)
    c["not_live_null"] = flat(6) + (None, 4)
    return c


CASES = build_cases()
EXPECT = {"chain3": [0, 0, 2], "chain3_extra_band": [0, 0, 0], "not_live": [0, 1, 2, 1, 1, 5], "not_live_null": [0] * 6,
          "edge_keys": [0, 0, 2, 2, 4, 5, 6, 7], "star1000": [0] * 1000, "bucket300": [0] * 300, "chain200": [0] * 200,
          "two_components": [0] * 100 + list(range(100, 500)) + [0] * 100, "K100_m100": [0, 0, 2, 3, 4, 4], "K100_m1": [0, 0, 2, 3, 4, 4]}
_REF = {}


def ref(name):
    """The case's inputs and the reference's (labels, rep), computed once and shared."""
    if name not in _REF:
        sig, keys, nsh, m = CASES[name]
        out = cr.cluster(sig, keys, m, nsh)
        for a in (sig, keys) + out:
            a.setflags(write=False)
        _REF[name] = (sig, keys, nsh, m) + out
    return _REF[name]


@pytest.fixture(scope="module")
def enc():
    import jtokkit_amd
    return jtokkit_amd.get_encoding("cl100k_base")


def run(b, sig, keys, nsh, m, shift=0, want_rep=True, stream=None, n=None, K=None, B=None):
    """jtk_batch_minhash_cluster with guard words around both outputs; shift: words of sig past the 16-byte boundary."""
    import torch
    n, K, B = (x if given is None else given for given, x in ((n, sig.shape[0]), (K, sig.shape[1]), (B, keys.shape[1])))
    sig_t = torch.zeros(sig.size + 8, dtype=torch.int32, device="cuda")
    sig_t[shift:shift + sig.size].copy_(torch.from_numpy(sig.view(np.int32).ravel().copy()))
    key_t = torch.from_numpy(np.append(keys.view(np.int64).ravel(), 0)).cuda()
    nsh_t = torch.from_numpy(nsh).cuda() if nsh is not None else None
    lab_t = torch.full((sig.shape[0] + 2 * PAD,), GUARD, dtype=torch.int64, device="cuda")
    rep_t = torch.full((keys.size + 2 * PAD,), GUARD, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    b.minhash_cluster(sig_t.data_ptr() + 4 * shift, key_t.data_ptr(), n, K, B, m, lab_t.data_ptr() + 8 * PAD,
                      nsh_t.data_ptr() if nsh is not None else None, rep_t.data_ptr() + 8 * PAD if want_rep else None, stream)
    torch.cuda.synchronize()
    return lab_t.cpu().numpy().view(np.uint64), rep_t.cpu().numpy().view(np.uint64)


def check(got, labels, rep, want_rep=True):
    lab, rp = got
    n = len(labels)
    assert (lab[:PAD] == GUARD).all() and (lab[PAD + n:] == GUARD).all() and (rp[:PAD] == GUARD).all() and (rp[PAD + rep.size:] == GUARD).all()
    assert np.array_equal(lab[PAD:PAD + n].view(np.int64), labels), np.flatnonzero(lab[PAD:PAD + n].view(np.int64) != labels)[:10]
    assert np.array_equal(rp[PAD:PAD + rep.size].view(np.int64).reshape(rep.shape), rep) if want_rep else (rp == GUARD).all()


@pytest.mark.parametrize("mode", ["aligned", "one_word_off", "callers_stream_no_rep"])
@pytest.mark.parametrize("name", list(CASES))
def test_every_case_equals_the_reference(enc, name, mode):
    import torch
    sig, keys, nsh, m, labels, rep = ref(name)
    assert name not in EXPECT or labels.tolist() == EXPECT[name]
    b = enc.new_batch()
    with_rep = mode != "callers_stream_no_rep"
    kw = dict(shift=mode == "one_word_off", want_rep=with_rep, stream=None if with_rep else torch.cuda.Stream().cuda_stream)
    first = run(b, sig, keys, nsh, m, **kw)
    check(first, labels, rep, with_rep)
    if name == "star1000":                                   # two runs of the largest case give the same
        assert all(np.array_equal(x, y) for x, y in zip(first, run(b, sig, keys, nsh, m, **kw)))
    b.close()


@pytest.mark.parametrize("name", ["chain200", "B16", "B256", "bucket300"])
def test_one_band_per_group_gives_the_same(enc, name):
    from jtokkit_amd import EncodingError, _native as N
    sig, keys, nsh, m, labels, rep = ref(name)
    cap = max(64, 1 << (2 * len(sig) - 1).bit_length())
    b = enc.new_batch()
    b.set_option(N.JTK_OPT_REPEAT_TABLE_BYTES, max(1280, cap * 16 + 8))
    check(run(b, sig, keys, nsh, m), labels, rep)
    if cap > 64:                                             # one byte less than a band
        b.set_option(N.JTK_OPT_REPEAT_TABLE_BYTES, cap * 16 + 7)
        with pytest.raises(EncodingError) as e:
            run(b, sig, keys, nsh, m)
        assert e.value.code == N.JTK_ERR_OUT_OF_MEMORY
    b.close()


def test_invalid_arguments(enc):
    import torch
    from jtokkit_amd import EncodingError, _native as N
    sig, keys, nsh, m, labels, rep = ref("K4_m4")
    b = enc.new_batch()
    for kw in (dict(n=-1), dict(K=0), dict(K=257), dict(B=0), dict(B=257), dict(m=0), dict(m=5), dict(m=-1)):
        with pytest.raises(EncodingError) as e:
            run(b, **dict(dict(sig=sig, keys=keys, nsh=nsh, m=m), **kw))
        assert e.value.code == N.JTK_ERR_INVALID_ARGUMENT, kw
    lab = torch.full((6,), GUARD, dtype=torch.int64, device="cuda")
    d_sig, d_keys = torch.zeros(24, dtype=torch.int32, device="cuda"), torch.zeros(12, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ps, pk, pl = d_sig.data_ptr(), d_keys.data_ptr(), lab.data_ptr()
    for h, a, k, l in ((b._h, None, pk, pl), (b._h, ps, None, pl), (b._h, ps, pk, None), (b._h, ps + 2, pk, pl), (b._h, ps, pk + 4, pl),
                       (b._h, ps, pk, pl + 4), (None, ps, pk, pl)):
        assert N.lib().jtk_batch_minhash_cluster(h, a, k, None, 6, 4, 2, 4, l, None, None) == N.JTK_ERR_INVALID_ARGUMENT
    torch.cuda.synchronize()
    assert (lab.cpu().numpy().view(np.uint64) == GUARD).all()                     # a refused call wrote nothing
    check(run(b, sig, keys, nsh, m), labels, rep)                                  # and the batch still works
    b.close()


def test_python_surface(enc):
    import torch
    docs, expected = mc.near_dup_batch()
    P = mc.NEAR
    kw = dict(ngram=P["ngram"], num_hashes=P["num_hashes"], bands=P["bands"], seed=P["seed"])
    got = enc.near_duplicate_clusters(docs, threshold=P["threshold"], **kw)
    sig, nsh, keys = enc.minhash_batch(docs, **kw)
    want, want_rep = cr.cluster(sig, keys, int(math.ceil(P["threshold"] * P["num_hashes"])), nsh)
    assert got.dtype == np.int64 and np.array_equal(got, expected) and np.array_equal(got, want)
    assert [enc.near_duplicate_clusters(t).tolist() for t in ([], ["one"], ["", "", ""])] == [[], [0], [0, 1, 2]]
    parts = [enc.minhash_batch(half, **kw) for half in (docs[:13], docs[13:])]
    d_sig, d_nsh, d_keys = (torch.from_numpy(np.concatenate([p[k] for p in parts]).view(t)).cuda() for k, t in ((0, np.int32), (1, np.int32), (2, np.int64)))
    labels, rep = enc.minhash_cluster_device(d_sig, d_keys, P["threshold"], d_nsh, return_rep=True)
    assert np.array_equal(labels.cpu().numpy(), want) and np.array_equal(rep.cpu().numpy(), want_rep)
