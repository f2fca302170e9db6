"""jtk_seen_set_* / jtk_batch_seen_mark and the Python surface on them (SeenSet, Batch.seen_mark, HipEncoding.exact_duplicates_batch,
exact_duplicates_batch_device): every per-unit and per-document output and the set's entries, sorted by key, equal to the plain
restatement tests/seen_ref.py exactly -- the pass is integer arithmetic only.  Every test here needs a real MI355X (`-m gpu`)."""
import numpy as np
import pytest

import seen_ref as sr

pytestmark = pytest.mark.gpu
BAD = b"bad \xff\xfe utf-8\nline one\n"                          # refused by JTK_ENCODE_VALIDATE_UTF8: no units


@pytest.fixture(scope="module")
def enc():
    import jtokkit_amd
    return jtokkit_amd.get_encoding("cl100k_base")


def mixed_docs():
    docs = [b"fifteen bytes.\n", b"x", b"y", b"", b" \t \r", b"\n\n\n", b"\n\n  lead and trail \t\n\n", b"crlf one\r\ncrlf two\r\n\r\ncrlf one\r\n", BAD,
            b"q" * 9000, b"  same after trim\n", b"same after trim  \n\n", b"same after trim!", b"line one\nline two\n\nline one\n \nline three"]
    docs += [b"doc %d\nline one\n\nshared paragraph\nof two lines\n\n" % (i % 7) for i in range(20)]
    docs.append(b"p" * (1023 - sum(map(len, docs)) % 1024))
    docs += [b"z", b"\n", b"line two\n", b"doc 3\nline one", b"q" * 9000]
    edges = set(np.cumsum([len(x) for x in docs]))
    assert {15, 16, 17} <= edges and {x % 1024 for x in edges} >= {1023, 0, 1} and 38 <= len(docs) <= 42
    return docs


def lines(lo, hi):
    return [b"".join(b"distinct line %d\n" % i for i in range(a, min(a + 50, hi))) for a in range(lo, hi, 50)]


def both(enc, S, R, docs, add=True, query=True, base=0, min_count=0):
    got = enc.exact_duplicates_batch(docs, S, add, query, base, min_count, validate=True)
    want = R.mark(docs, [-1 if d == BAD else 0 for d in docs], (sr.ADD if add else 0) | (sr.QUERY if query else 0), base, min_count)
    assert (got is None) == (want is None)
    for name in want or ():
        assert got[name].dtype == want[name].dtype and np.array_equal(got[name], want[name]), name
    same_entries(S, R)
    return got


def same_entries(S, R):
    k, f, c = S.entries()
    o = np.argsort(k)
    assert all(np.array_equal(g[o], w) for g, w in zip((k, f, c), R.entries())) and len(S) == len(R.d) and S.capacity == R.cap


def case_units(enc, unit, trim):
    S, R = enc.seen_set(unit, trim, seed=7), sr.Set({"line": sr.LINE, "paragraph": sr.PARAGRAPH, "document": sr.DOCUMENT}[unit], trim, 7)
    got = both(enc, S, R, mixed_docs(), base=5)
    assert got["unit_flags"].any() and got["unit_off"][9] == got["unit_off"][8]               # duplicates found; the refused document has no unit
    both(enc, S, R, mixed_docs()[10:], base=100)                                             # a second batch: everything seen before


def case_far_apart(enc):
    docs = [b"the repeated line\n" + b"".join(lines(0, 300)), b"".join(lines(300, 600)) + b"the repeated line\n", b"the repeated line"]
    got = both(enc, enc.seen_set(), sr.Set(), docs)
    assert list(got["unit_count"][[0, 601, 602]]) == [3, 3, 3] and list(got["unit_flags"][[0, 601, 602]]) == [0, 1, 1]


def case_one_line(enc):
    S, R, S2 = enc.seen_set(), sr.Set(), enc.seen_set()
    got = both(enc, S, R, [b"boilerplate\n" * 3000], base=9)
    assert len(S) == 1 and got["unit_count"][0] == 3000 and got["n_dup"][0] == 2999
    assert enc._b().seen_mark(S2, True, False, 9, combine=False) == 3000
    same_entries(S2, R)


def case_growth(enc):
    S, R, caps = enc.seen_set(), sr.Set(), []
    for base, (lo, hi) in enumerate(((0, 20), (20, 220), (220, 3220))):
        both(enc, S, R, lines(lo, hi), base=base * 100)
        caps.append(S.capacity)
    assert caps == [64, 512, 8192] and len(S) == 3220


def case_order(enc):
    A, B = mixed_docs()[:20], mixed_docs()[14:] + [b"only in B\nline one\n"]
    SAB, SBA, R = enc.seen_set("line", True), enc.seen_set("line", True), sr.Set(sr.LINE, True)
    for S, order in ((SAB, ((A, 0), (B, 20))), (SBA, ((B, 20), (A, 0)))):
        for docs, base in order:
            enc.exact_duplicates_batch(docs, S, True, False, base, validate=True)
    R.mark(A + B, [-1 if d == BAD else 0 for d in A + B], sr.ADD)
    for S in (SAB, SBA):
        both(enc, S, R, A, add=False, base=0, min_count=3)
        both(enc, S, R, B, add=False, base=20, min_count=3)


def case_shards(enc):
    docs = mixed_docs()
    S1, S2, R = enc.seen_set("paragraph"), enc.seen_set("paragraph"), sr.Set(sr.PARAGRAPH)
    enc.exact_duplicates_batch(docs[:17], S1, True, False, 0, validate=True)
    enc.exact_duplicates_batch(docs[17:], S2, True, False, 17, validate=True)
    S1.add_entries(*S2.entries())
    R.mark(docs, [-1 if d == BAD else 0 for d in docs], sr.ADD)
    R.cap = S1.capacity                                          # (the merged set's capacity follows its own history of adds)
    both(enc, S1, R, docs, add=False)


def case_probing(enc):
    keys = [((i + 1) << 8) | lo for i, lo in enumerate((63, 63, 63, 62, 62, 0))] + [(1 << 8) | 63, (4 << 8) | 62]
    S, R = enc.seen_set(), sr.Set()
    for X in (S, R):
        X.add_entries(keys, [70, 60, 50, 40, 30, 20, 7, 99], [1, 2, 3, 4, 5, 6, 10, 20])
    same_entries(S, R)
    assert len(S) == 6 and S.capacity == 64


def case_modes(enc):
    import torch
    docs = [b"once\ntwice\nthrice\n", b"twice\nthrice\n", b"thrice\n"]
    S, R = enc.seen_set(), sr.Set()
    got = both(enc, S, R, docs, add=False)                       # QUERY alone on an empty set
    assert (got["unit_first"] == sr.ABSENT).all() and not got["unit_count"].any() and not got["unit_flags"].any()
    guard = torch.full((16,), 0x5A, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert enc._b().seen_mark(S, True, False, unit_flags=guard.data_ptr()) == 6 and len(S) == 3          # ADD alone writes no output
    assert (guard.cpu().numpy() == 0x5A).all()
    R.mark(docs, [0, 0, 0], sr.ADD)
    assert list(both(enc, S, R, docs, add=False, min_count=0)["unit_flags"]) == [0, 0, 0, 1, 1, 1]
    assert list(both(enc, S, R, docs, add=False, min_count=2)["unit_flags"]) == [0, 2, 2, 3, 3, 3]


CASES = {"%s%s" % (u, "_trim" if t else ""): (lambda enc, u=u, t=t: case_units(enc, u, t)) for u in ("line", "paragraph", "document") for t in (False, True)}
CASES.update(far_apart=case_far_apart, one_line=case_one_line, growth=case_growth, order=case_order, shards=case_shards, probing=case_probing,
             modes=case_modes)


@pytest.mark.parametrize("name", list(CASES))
def test_seen_matches_reference(enc, name):
    CASES[name](enc)


def test_invalid_arguments_leave_the_set_unchanged(enc):
    import ctypes as C
    import jtokkit_amd
    from jtokkit_amd import _native as N
    from jtokkit_amd.encoding import _check
    S = enc.seen_set()
    enc.exact_duplicates_batch([b"a line\n"], S, query=False)
    before, b = S.entries(), enc._b()
    unknown_flags = lambda: _check(N.lib().jtk_seen_set_create(enc._h, C.byref(N.SeenParamsStruct(0, 0, 4)), C.byref(C.c_void_p())))
    calls = [lambda: enc.seen_set(3), unknown_flags, lambda: b.seen_mark(S, False, False), lambda: b.seen_mark(S, doc_index_base=1 << 40),
             lambda: S.add_entries([5, 0], [1, 1], [1, 1]), lambda: b.seen_mark(None), lambda: enc.new_batch().seen_mark(S)]
    for i, call in enumerate(calls):
        with pytest.raises(jtokkit_amd.EncodingError) as e:
            call()
        assert e.value.code == N.JTK_ERR_INVALID_ARGUMENT, i
    assert all(np.array_equal(x, y) for x, y in zip(before, S.entries())) and b.seen_mark(S, False, True) == 1


def test_device_surface_empty_batch_and_stream(enc):
    import torch
    docs = [d for d in mixed_docs() if d != BAD]              # (the device route does not validate)
    S, R = enc.seen_set("line", True), sr.Set(sr.LINE, True)
    want = R.mark(docs, [0] * len(docs), base=3, min_count=2)
    text = torch.frombuffer(bytearray(b"".join(docs)), dtype=torch.uint8).cuda()
    off = torch.tensor(np.concatenate([[0], np.cumsum([len(x) for x in docs])]), dtype=torch.int64, device="cuda")
    with torch.cuda.stream(torch.cuda.Stream()):                 # a caller's stream
        got = enc.exact_duplicates_batch_device(text, off, S, doc_index_base=3, min_count=2)
        torch.cuda.current_stream().synchronize()
    assert (got["status"].cpu().numpy() >= 0).all() and all(np.array_equal(got[n].cpu().numpy().view(want[n].dtype), want[n]) for n in want)
    same_entries(S, R)
    res = enc.exact_duplicates_batch([], S)
    assert len(res["unit_begin"]) == 0 and list(res["unit_off"]) == [0]
    same_entries(S, R)
