"""jtk_batch_pack_best_fit and pack_batch / pack_batch_device(fit="best"): best-fit-decreasing rows of whole documents, with
write, fetch and labels served by the existing entry points.  Every field is checked bit for bit against the one-rest-at-a-time
restatement of the rule (tests/pack_fit_ref.py) applied to the CPU oracle's tokens; documents are runs of one-token words, so
their unit lengths are exact.  Every test here needs a real MI355X (`-m gpu`)."""
import ctypes as C
import random

import numpy as np
import pytest

import label_ref
import oracle_lib
import pack_fit_ref
import pack_ref

pytestmark = pytest.mark.gpu

EOT = "<|endoftext|>"
EOT_ID = 100257
PAD = -3
WORDS = ("a", "b", "c", "the", "is", "on", "x", "we")
SEPS = [(EOT_ID, False), (EOT_ID, True), (-1, False)]               # EOS, BOS, no separator
REFUSED = -1                                                        # a length that stands for a document with a literal in it


def _lengths(kind, L, rng):
    if kind == "edges":                                             # l = L - 1, L, L + 1, k L, k L + 1 with and without separator
        return [rng.choice([0, 1, 2, L - 2, L - 1, L, L + 1, 2 * L - 1, 2 * L, 2 * L + 1, 3 * L, REFUSED, rng.randint(0, 3 * L)])
                for _ in range(70 if L < 1000 else 24)]
    if kind == "small":                                             # 3000 rests of at most L / 4: rows take several per step
        return [rng.randint(0, L // 4) for _ in range(3000)]
    if kind == "equal":
        return [L // 3] * 100
    return {"none": [], "one": [L // 2 + 1]}[kind]


CASES = [("edges", 4), ("edges", 7), ("small", 64), ("equal", 64), ("edges", 300), ("small", 300), ("edges", 4096), ("none", 7),
         ("one", 7)]


@pytest.fixture(scope="module")
def jt():
    import jtokkit_amd
    return jtokkit_amd


@pytest.fixture(scope="module")
def enc(jt):
    return jt.get_encoding("cl100k_base")


def _batch(kind, L, seed=0, refuse=True):
    """texts, and the oracle's (docs, status) for them: [] and -1 for a refused document (an empty one without `refuse`)."""
    rng = random.Random(1000 * L + seed)
    o = oracle_lib.get("cl100k_base")
    texts, docs, status = [], [], []
    for n in _lengths(kind, L, rng):
        n = 0 if n == REFUSED and not refuse else n
        t = "x" + EOT if n == REFUSED else " ".join(rng.choice(WORDS) for _ in range(n))
        texts.append(t)
        docs.append([] if n == REFUSED else o.encode(t.encode()))
        status.append(-1 if n == REFUSED else 0)
        assert n == REFUSED or len(docs[-1]) == n
    return texts, docs, status


def _encode(enc, texts):
    bs = [t.encode() for t in texts]
    doc_off = np.zeros(len(bs) + 1, dtype=np.int64)
    np.cumsum([len(x) for x in bs], out=doc_off[1:])
    text = np.frombuffer(b"".join(bs), dtype=np.uint8) if doc_off[-1] else np.zeros(0, dtype=np.uint8)
    b = enc.new_batch()
    b.encode_host(text, doc_off, ordinary=False)
    return b, text, doc_off


def _same(got, exp, what):
    for k in ("rows", "positions", "cu_seqlens", "seg_doc"):
        g = np.asarray(got[k])
        assert g.shape == exp[k].shape and np.array_equal(g, exp[k]), (k, what)
    assert got["max_seqlen"] == exp["max_seqlen"], what


@pytest.mark.parametrize("kind,L", CASES)
def test_c_abi_against_the_restatement(enc, kind, L):
    """Plan, write and fetch for every separator style; never more rows than next-fit of the same batch."""
    texts, docs, status = _batch(kind, L)
    b, _, _ = _encode(enc, texts)
    for sep, sep_first in SEPS:
        exp = pack_fit_ref.pack(docs, status, L, sep, sep_first, PAD)
        nr, ns, mx = b.pack(L, sep, sep_first=sep_first, fit="best")
        f = b.pack_fetch(PAD)
        assert f["rows"].shape == (nr, L) and len(f["cu_seqlens"]) == ns + 1 and nr == len(exp["rows"])
        f["max_seqlen"] = mx
        _same(f, exp, (kind, L, sep, sep_first))
        assert nr <= b.pack(L, sep, whole_docs=True, sep_first=sep_first)[0]
    b.close()


@pytest.mark.parametrize("kind,L", [("edges", 7), ("small", 300)])
def test_python_front_ends(enc, kind, L):
    """pack_batch and pack_batch_device with fit="best" (whole_docs may accompany it)."""
    import torch
    texts, docs, status = _batch(kind, L, seed=1)
    b, text, doc_off = _encode(enc, texts)
    b.close()
    exp = pack_fit_ref.pack(docs, status, L, EOT_ID, False, PAD)
    h = enc.pack_batch(texts, L, sep=EOT, pad_id=PAD, fit="best")
    _same(h, exp, "pack_batch")
    assert [s < 0 for s in h["status"]] == [s < 0 for s in status]
    out = enc.pack_batch_device(torch.from_numpy(text.copy()).cuda(), torch.from_numpy(doc_off).cuda(), L, sep=EOT, whole_docs=True,
                                pad_id=PAD, fit="best")
    torch.cuda.synchronize()
    _same({k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in out.items()}, exp, "pack_batch_device")


@pytest.mark.parametrize("shift,label_sep", [(False, False), (True, False), (False, True), (True, True)])
def test_labels_follow_the_label_rule(enc, shift, label_sep):
    """Labels of best-fit rows: label_ref's cell rule on the restatement's rows, with spans and with every token trainable."""
    L = 7
    texts, docs, status = _batch("edges", L, seed=2, refuse=False)    # (tok_span below is indexed by the oracle's tokens)
    spans = [[] if len(t) < 4 else [(1, len(t) // 2)] for t in texts]
    got = enc.pack_batch(texts, L, sep=EOT, pad_id=PAD, fit="best", train_spans=spans, span_rule="start", label_shift=shift,
                         label_sep=label_sep)
    packed = pack_fit_ref.pack(docs, status, L, EOT_ID, False, PAD)
    _same(got, packed, "rows")
    assert (got["tok_span"] >= 0).any() and (got["tok_span"] < 0).any()
    exp = label_ref.labels(docs, status, L, EOT_ID, tok_span=got["tok_span"], shift=shift, label_sep=label_sep, packed=packed)
    assert np.array_equal(got["labels"], exp), np.argwhere(got["labels"] != exp)[:8]
    b, _, _ = _encode(enc, texts)
    b.pack(L, EOT_ID, sep_first=True, fit="best")
    packed = pack_fit_ref.pack(docs, status, L, EOT_ID, True, PAD)
    exp = label_ref.labels(docs, status, L, EOT_ID, True, shift=shift, label_sep=label_sep, packed=packed)
    assert np.array_equal(b.pack_labels_fetch(None, -100, shift, label_sep), exp)
    b.close()


def test_bad_arguments_and_plan_replacement(jt, enc):
    N = jt._native
    lib = N.lib()
    INV = N.JTK_ERR_INVALID_ARGUMENT
    texts, docs, status = _batch("edges", 7, seed=3)
    b, text, doc_off = _encode(enc, texts)
    nr, ns, mx = C.c_int64(0), C.c_int64(0), C.c_int32(0)

    def pk(seq_len, sep=-1, flags=0):
        return lib.jtk_batch_pack_best_fit(b._h, seq_len, sep, flags, None, C.byref(nr), C.byref(ns), C.byref(mx))

    assert pk(N.JTK_PACK_FIT_MAX_LEN + 1) == INV and "JTK_PACK_FIT_MAX_LEN" in lib.jtk_last_error().decode()
    assert pk(N.JTK_PACK_FIT_MAX_LEN) == N.JTK_OK and nr.value == 1
    for bad in (0, -1, 1 << 40):
        assert pk(bad) == INV
    for flags in (N.JTK_PACK_WHOLE_DOCS, N.JTK_PACK_DROP_LAST, 8, 3):
        assert pk(7, -1, flags) == INV, flags
    assert pk(7, 100256) == INV and pk(7, -2) == INV
    # the best-fit plan and the next-fit plan replace each other
    assert pk(7, EOT_ID, N.JTK_PACK_SEP_FIRST) == N.JTK_OK
    b._pack = (nr.value, 7, ns.value)
    assert np.array_equal(b.pack_fetch(PAD)["rows"], pack_fit_ref.pack(docs, status, 7, EOT_ID, True, PAD)["rows"])
    b.pack(7, EOT_ID, whole_docs=True)
    assert np.array_equal(b.pack_fetch(PAD)["rows"], pack_ref.pack(docs, status, 7, EOT_ID, whole=True, pad_id=PAD)["rows"])
    b.encode_host(text, doc_off, count_only=True)
    assert pk(7) == INV
    b.close()
    for call in (lambda: enc.pack_batch(texts, 7, fit="best", drop_last=True), lambda: enc.pack_batch(texts, 7, fit="first")):
        with pytest.raises(ValueError):
            call()
