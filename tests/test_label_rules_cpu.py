"""CPU tier: the label rule of jtk_batch_token_spans / jtk_batch_pack_labels (jtokkit_amd/csrc/jtk_label_rules.h), run on the
CPU through the shim tests/label_sim, against the plain restatement tests/label_ref.py.  Every entry of tok_span and of labels
is compared, for the three span rules, the nine pack modes of test_pack_rules_cpu.py, shift x label_sep, tok_span given and
NULL.  The shim's span pass restarts its cursor every 8 tokens and its cell walk every `run` cells, as the kernels' lanes do."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import label_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEP = 100257
IGN = -100
RUNS = (0, 1, 4, 7)
RULES = (label_ref.WHOLE, label_ref.START, label_ref.ANY)
MODES = [(-1, False, False, False), (-1, False, False, True), (-1, False, True, False),
         (SEP, False, False, False), (SEP, False, False, True), (SEP, False, True, False),
         (SEP, True, False, False), (SEP, True, False, True), (SEP, True, True, False)]   # (sep, sep_first, whole, drop_last)


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("label_sim") / "liblabel_sim.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-o", out,
                           os.path.join(ROOT, "tests", "label_sim", "label_sim.cpp")])
    L = C.CDLL(out)
    head = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int, C.c_int, C.c_int]
    L.sim_pack_counts.restype = None
    L.sim_pack_counts.argtypes = head + [C.c_void_p]
    L.sim_tok_spans.restype = None
    L.sim_tok_spans.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int64,
                                C.c_void_p]
    L.sim_labels.restype = None
    L.sim_labels.argtypes = head + [C.c_void_p, C.c_int32, C.c_int, C.c_int, C.c_int64, C.c_void_p]
    return L


def _tok_off(docs):
    tok_off = np.zeros(len(docs) + 1, dtype=np.int64)
    np.cumsum([len(d) for d in docs], out=tok_off[1:])
    return tok_off


def _sim_spans(sim, doc_lens, doc_off, spans, rule, lane=8):
    lens = np.array([n for d in doc_lens for n in d] + [0], dtype=np.uint32)
    tok_off = _tok_off(doc_lens)
    off = np.asarray(doc_off, dtype=np.int64)
    B = np.array([s[0] for s in spans] + [0], dtype=np.int64)
    E = np.array([s[1] for s in spans] + [0], dtype=np.int64)
    out = np.full(int(tok_off[-1]) + 1, 12345, dtype=np.int32)
    sim.sim_tok_spans(lens.ctypes.data, tok_off.ctypes.data, off.ctypes.data, len(doc_lens), B.ctypes.data, E.ctypes.data,
                      len(spans), rule, lane, out.ctypes.data)
    assert out[-1] == 12345                                   # nothing past the output
    return out[:-1]


def _sim_labels(sim, docs, status, L, mode, tok_span, shift, label_sep, run):
    sep, sep_first, whole, drop = mode
    toks = np.array([t for d in docs for t in d] + [0], dtype=np.int32)
    tok_off = _tok_off(docs)
    st = np.array(list(status) + [0], dtype=np.int32)
    counts = np.zeros(3, dtype=np.int64)
    args = (toks.ctypes.data, tok_off.ctypes.data, st.ctypes.data, len(docs), L, sep, int(sep_first), int(whole), int(drop))
    sim.sim_pack_counts(*args, counts.ctypes.data)
    nr = int(counts[0])
    out = np.full(nr * L + 1, 12345, dtype=np.int32)
    ts = None if tok_span is None else np.ascontiguousarray(np.append(tok_span, 0), dtype=np.int32)
    sim.sim_labels(*args, None if ts is None else ts.ctypes.data, IGN, int(shift), int(label_sep), run, out.ctypes.data)
    assert out[-1] == 12345
    return out[:-1].reshape(nr, L)


def _check_spans(sim, doc_lens, doc_off, spans):
    """All three rules; returns the whole-rule tok_span."""
    for rule in RULES:
        exp = label_ref.token_spans(doc_lens, doc_off, spans, rule)
        for lane in (8, 1, 0):
            got = _sim_spans(sim, doc_lens, doc_off, spans, rule, lane)
            assert np.array_equal(got, exp), (rule, lane, spans, got.tolist(), exp.tolist())
    return label_ref.token_spans(doc_lens, doc_off, spans, label_ref.WHOLE)


def _check_labels(sim, docs, status, L, tok_span, modes=MODES, runs=RUNS):
    for mode in modes:
        sep, sep_first, whole, drop = mode
        for ts in (tok_span, None):
            for shift in (False, True):
                for label_sep in (False, True):
                    exp = label_ref.labels(docs, status, L, sep, sep_first, whole, drop, ts, IGN, shift, label_sep)
                    for run in runs:
                        got = _sim_labels(sim, docs, status, L, mode, ts, shift, label_sep, run)
                        assert got.shape == exp.shape and np.array_equal(got, exp), (L, mode, ts is None, shift, label_sep, run,
                                                                                     got.tolist(), exp.tolist())


def _docs(lengths, seed=0):
    return [[(d * 7919 + i * 31 + seed) % 100000 for i in range(n)] for d, n in enumerate(lengths)]


def _batch(rng, lengths, gap=False):
    """Token byte lengths 1..6 per token; doc_off back to back (gap: some documents hold bytes no token covers at their end,
    as a refused document may)."""
    doc_lens = [[rng.randint(1, 6) for _ in range(n)] for n in lengths]
    doc_off = [0]
    for lens in doc_lens:
        doc_off.append(doc_off[-1] + sum(lens) + (rng.randint(0, 3) if gap else 0))
    return doc_lens, doc_off


def _random_spans(rng, n_bytes, n_spans):
    """Sorted and disjoint; repeated cut points make empty spans and adjacent spans."""
    cuts = []
    for _ in range(2 * n_spans):
        cuts.append(rng.choice(cuts) if cuts and rng.random() < 0.25 else rng.randint(0, n_bytes))
    cuts.sort()
    return [(cuts[2 * i], cuts[2 * i + 1]) for i in range(n_spans)]


def test_random_documents_and_spans(sim):
    rng = random.Random(23)
    for L in (1, 7, 128):
        for _ in range(6):
            n = rng.randint(0, 24)
            lengths = [rng.choice([0, 1, max(L - 1, 0), L, L + 1, 2 * L, rng.randint(0, 3 * L)]) for _ in range(n)]
            lengths = [min(x, 300) for x in lengths]
            status = [-1 if rng.random() < 0.15 else 0 for _ in range(n)]
            doc_lens, doc_off = _batch(rng, lengths, gap=True)
            spans = _random_spans(rng, doc_off[-1], rng.randint(0, 12))
            _check_spans(sim, doc_lens, doc_off, spans)
            tok_span = label_ref.token_spans(doc_lens, doc_off, spans, rng.choice(RULES))
            _check_labels(sim, _docs(lengths, rng.randint(0, 99)), status, L, tok_span, runs=(0, 4) if L == 128 else RUNS)


def test_span_edges_separate_the_rules(sim):
    """One document of tokens [0,3) [3,5) [5,9) [9,10): a span ending at a token start, at a token end, one byte inside a token,
    empty spans, adjacent spans, a span covering everything, zero spans."""
    doc_lens, doc_off = [[3, 2, 4, 1]], [0, 10]
    cases = {
        ((0, 5),): ([0, 0, -1, -1], [0, 0, -1, -1], [0, 0, -1, -1]),            # ends exactly at a token end / start
        ((0, 6),): ([0, 0, -1, -1], [0, 0, 0, -1], [0, 0, 0, -1]),              # one byte inside token 2
        ((4, 9),): ([-1, -1, 0, -1], [-1, -1, 0, -1], [-1, 0, 0, -1]),          # begins one byte before token 1's end
        ((4, 4), (7, 7)): ([-1] * 4, [-1] * 4, [-1] * 4),                        # empty spans hold nothing, even inside a token
        ((0, 3), (3, 5), (5, 5), (5, 10)): ([0, 1, 3, 3], [0, 1, 3, 3], [0, 1, 3, 3]),   # adjacent, an empty one between
        ((0, 10),): ([0] * 4, [0] * 4, [0] * 4),
        ((0, 4), (4, 10)): ([0, -1, 1, 1], [0, 0, 1, 1], [0, 0, 1, 1]),         # token 1 straddles two spans: any takes the lowest
        ((1, 2), (2, 3)): ([-1] * 4, [-1] * 4, [0, -1, -1, -1]),                # two spans inside one token
        (): ([-1] * 4, [-1] * 4, [-1] * 4),
    }
    for spans, exp in cases.items():
        for rule, e in zip(RULES, exp):
            assert label_ref.token_spans(doc_lens, doc_off, list(spans), rule).tolist() == e, (spans, rule)
        _check_spans(sim, doc_lens, doc_off, list(spans))


def test_spans_across_documents_refused_and_empty_documents(sim):
    rng = random.Random(3)
    lengths = [5, 0, 9, 0, 0, 4, 12, 1]
    status = [0, 0, -2, 0, -1, 0, 0, 0]
    doc_lens, doc_off = _batch(rng, lengths)
    docs = _docs(lengths)
    n_bytes = doc_off[-1]
    for spans in ([(doc_off[0] + 1, doc_off[3] + 2)],                            # crosses documents 0 .. 2
                  [(doc_off[2], doc_off[3])],                                    # only in a refused document
                  [(doc_off[2] + 1, doc_off[2] + 3), (doc_off[4], doc_off[5])],  # refused and empty documents only
                  [(0, n_bytes)], [],
                  [(doc_off[5], doc_off[6]), (doc_off[6], doc_off[6] + 1), (doc_off[7], n_bytes)]):
        _check_spans(sim, doc_lens, doc_off, spans)
        for rule in RULES:
            _check_labels(sim, docs, status, 7, label_ref.token_spans(doc_lens, doc_off, spans, rule), runs=(0, 4))
    # documents with no tokens at all, with and without a separator
    _check_labels(sim, _docs([0, 0, 0]), [0, 0, 0], 3, np.zeros(0, dtype=np.int32))
    _check_labels(sim, [], [], 4, np.zeros(0, dtype=np.int32))


@pytest.mark.parametrize("L", [1, 7, 128])
def test_unit_length_edges(sim, L):
    """Unit lengths 0, L - 1, L, L + 1 and k * L, the last token of a unit trainable or not (label_sep), spans placed on the
    tokens at the segment edges."""
    rng = random.Random(L)
    edges = [0, L - 1, L, L + 1, 3 * L]
    for a in edges:
        for b in edges:
            lengths = [a, b, a]
            doc_lens, doc_off = _batch(rng, lengths)
            spans = _random_spans(rng, doc_off[-1], 5)
            tok_span = label_ref.token_spans(doc_lens, doc_off, spans, label_ref.ANY)
            _check_labels(sim, _docs(lengths), [0, 0, 0], L, tok_span, runs=(0, 4))
    lengths = edges + [L - 1] * 3 + [1] * 3
    doc_lens, doc_off = _batch(rng, lengths)
    for keep_last in (False, True):                     # every document's last token trainable, or only its first
        spans = []
        for d, lens in enumerate(doc_lens):
            if lens:
                spans.append((doc_off[d + 1] - lens[-1], doc_off[d + 1]) if keep_last else (doc_off[d], doc_off[d] + lens[0]))
        spans = sorted(set(spans))
        spans = [s for i, s in enumerate(spans) if i == 0 or s[0] >= spans[i - 1][1]]
        _check_spans(sim, doc_lens, doc_off, spans)
        _check_labels(sim, _docs(lengths), [0] * len(lengths), L, label_ref.token_spans(doc_lens, doc_off, spans, label_ref.WHOLE))


def test_restatement_by_hand():
    """label_ref itself on a case worked out by hand: L = 4, EOS 9, units [1 2 9] [3 9] [4 5 6 7 8 9]; tokens 2, 4 and 8
    trainable."""
    docs, status = [[1, 2], [3], [4, 5, 6, 7, 8]], [0, 0, 0]
    ts = np.array([-1, 0, -1, 1, -1, -1, -1, 2], dtype=np.int32)
    i = IGN
    # rows [[1, 2, 9, 3], [9, 4, 5, 6], [7, 8, 9, pad]]
    assert label_ref.labels(docs, status, 4, 9, tok_span=ts).tolist() == [[i, 2, i, i], [i, 4, i, i], [i, 8, i, i]]
    assert label_ref.labels(docs, status, 4, 9, tok_span=ts, label_sep=True).tolist() == [[i, 2, 9, i], [i, 4, i, i], [i, 8, 9, i]]
    assert label_ref.labels(docs, status, 4, 9, tok_span=ts, shift=True, label_sep=True).tolist() == \
        [[2, 9, i, i], [i, i, i, i], [8, 9, i, i]]
    assert label_ref.labels(docs, status, 4, 9, shift=True, label_sep=True).tolist() == [[2, 9, i, i], [i, 5, 6, i], [8, 9, i, i]]
    # BOS style: rows [[9, 1, 2, 9], [3, 9, 4, 5], [6, 7, 8, pad]]: the separator is never a label
    assert label_ref.labels(docs, status, 4, 9, sep_first=True, label_sep=True).tolist() == [[i, 1, 2, i], [3, i, 4, 5], [6, 7, 8, i]]
    assert label_ref.token_spans([[3, 2, 4, 1]], [0, 10], [(0, 6)], label_ref.WHOLE).tolist() == [0, 0, -1, -1]
