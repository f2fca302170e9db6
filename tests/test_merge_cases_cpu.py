"""CPU tier: what merge_cases.py feeds k_bpe_merge's eleven merge paths, asserted before any device runs
(tests/test_merge_paths_gpu.py relies on this).

- the lengths and queue sizes restated in merge_cases.py are those of jtk_kernels.h / jtk_kernels.hip;
- the oracle's merge of every case piece equals merge_ref.py (reference GptBytePairEncoding.java:200-275 written out on byte
  strings), and the lane merge of jtk_merge_core.h up to 64 bytes;
- per path: every edge length in every kind; each of merge_ref's three wrong variants (the last minimum wins a tie, the
  previous part's rank is stale, the merged part's rank is stale) changes the tokens of some piece, so a kernel with that
  error cannot equal the oracle on the device; result words of <= 6, 7 and 8 tokens and ids of more than 16 bits at every
  position of both result-word layouts; neighbours more than 64 bytes away; merges that touch two cached chunks of merge_giant;
  ties on both sides of slots 63, 511 and 8191; pair lookups that take the second round of lean_steps;
- per text: the per-shard and per-list counts at which the dispatch changes, and the split into the planned pieces.

What the cl100k_base vocabulary does not provide is asserted as such: a hard piece of a blank and one letter (every one is a
token), an 8-byte piece of 8 tokens of these kinds (printed if found), and a merge whose three parts lie in three different
chunks of 256 positions (no token is longer than 128 bytes).
"""
import os
import re
import time

import numpy as np
import pytest

import merge_cases as mc
import merge_ref
import oracle_lib

CSRC = os.path.join(oracle_lib.ROOT, "jtokkit_amd", "csrc")


@pytest.fixture(scope="module")
def plan():
    return mc.Plan()


@pytest.fixture(scope="module")
def P(plan):
    return plan.P


@pytest.fixture(scope="module")
def ref(plan):
    """piece -> (tokens, Trace) by merge_ref, for every case piece of up to 1100 bytes and one of each kind at 8193"""
    t0 = time.time()
    out = {}
    big = set()
    for e in plan.everything:
        first_giant = e.length == mc.LONG_CAP + 1 and e.place is None and e.kind not in big
        if e.length <= 1100 or first_giant:
            out[e.piece] = merge_ref.merge_ref(e.piece, plan.P.ranks)
            if first_giant:
                big.add(e.kind)
    assert big == set(mc.KINDS)
    print("merge_ref of %d pieces: %.1f s" % (len(out), time.time() - t0))
    return out


def test_constants_are_the_kernels():
    with open(os.path.join(CSRC, "jtk_kernels.h")) as f:
        h = f.read()
    with open(os.path.join(CSRC, "jtk_kernels.hip")) as f:
        hip = f.read()
    define = lambda src, name: int(eval(re.search(r"#define\s+%s\s+\(?([0-9x<> ]+)\)?" % name, src).group(1)))
    assert define(h, "JTK_TILE") == mc.T == mc.psc.T
    assert define(h, "JTK_Q_SHARDS") == mc.Q_SHARDS
    assert define(h, "JTK_M_WGS_PER_SHARD") == mc.M_WGS_PER_SHARD
    assert define(h, "JTK_MID_CAP") == mc.MID_CAP
    assert define(h, "JTK_LONG_CAP") == mc.LONG_CAP
    assert define(h, "JTK_GIANT_CHUNK") == mc.GIANT_CHUNK
    assert define(h, "JTK_BIN_MAXLEN") == mc.BIN_LAST[-1]
    assert define(h, "JTK_GIANT_CAP") >= mc.GIANT_TOP
    assert define(hip, "JTK_ML_THREADS") == mc.ML_THREADS
    assert int(re.search(r"constexpr int M_CHUNK = (\d+);", hip).group(1)) == mc.M_CHUNK
    assert int(re.search(r"constexpr int ML_WGS_PER_SHARD = (\d+);", hip).group(1)) == mc.M_WGS_PER_SHARD      # the grid of k_bpe_merge
    # bins by length: three bits per length up to 16, then one bin per power of two
    bin16 = eval(re.search(r"constexpr uint64_t BIN16 = ([^;]+);", hip).group(1).replace("ull", "").replace("\n", " "))
    assert re.search(r"len <= 16u \? \(uint32_t\)\(BIN16 >> \(3u \* len\)\) & 7u : 30u - \(uint32_t\)__builtin_clz\(len - 1u\)", hip)
    kernel_bin = lambda n: (bin16 >> (3 * n)) & 7 if n <= 16 else 30 - (32 - int(n - 1).bit_length())
    for n in range(2, mc.BIN_LAST[-1] + 1):
        assert kernel_bin(n) == mc.bin_of(n), n
        path = mc.path_of(n)
        assert mc.PATH_NAMES.index(path) == (0 if kernel_bin(n) == 7 else kernel_bin(n) + 1), n
    assert [hi for _, _, hi in mc.PATHS[:8]] == list(mc.BIN_LAST)
    # the one-pass sizes of the dispatch and the templates behind the path names
    for text in ("n0 <= (uint32_t)ML_THREADS && n1 <= (uint32_t)ML_THREADS && n2 <= (uint32_t)ML_THREADS",
                 "nt5 <= (uint32_t)ML_THREADS && n3 <= (uint32_t)(ML_THREADS / 2) && n4 <= (uint32_t)(ML_THREADS / 4)",
                 "lean_bin<16, ML_THREADS, 0>", "lean_bin<16, ML_THREADS, 1>", "lean_bin<16, ML_THREADS, 2>",
                 "lean_bin<32, ML_THREADS / 2, 3>", "lean_bin<64, ML_THREADS / 4, 4>", "merge_bin<128, ML_WORDS / 128, 5>",
                 "merge_bin<256, ML_WORDS / 256, 6>", "merge_long<JTK_MID_CAP>", "merge_long<JTK_LONG_CAP>",
                 "lean_piece16<8, THREADS>", "lean_piece16<12, THREADS>", "lean_piece16<16, THREADS>",
                 "dim3(JTK_Q_SHARDS * ML_WGS_PER_SHARD), dim3(ML_THREADS)"):
        assert text in hip, text
    assert mc.GRID_WGS == 256 and mc.GRID_WAVES == 4096


def test_oracle_equals_reference(plan, P, ref):
    """... on every case piece of up to 1100 bytes, one 8193-byte piece of each kind, and a sample of the crowded and list texts'
    pieces; up to 64 bytes the lane merge of jtk_merge_core.h gives the same (sim_merge_piece, and the counting variant)."""
    for p, (tokens, _) in ref.items():
        assert P.tokens(p) == tokens, p[:60]
        if len(p) <= 64:
            assert P.sim.merge(p) == tokens and P.sim.stats(p)[0] == tokens, p
    n = 0
    for t in (mc.crowded(P)[0], mc.lists(P, n_giant=4)):
        for _, e in t.cases[::16]:
            if e.length <= 1100:
                assert P.tokens(e.piece) == merge_ref.merge_ref(e.piece, P.ranks)[0], e
                n += 1
    assert n > 700


def _by_path(plan):
    out = {path: [] for path in mc.PATH_NAMES}
    for e in plan.everything:
        out[e.path].append(e)
    return out


def test_every_length_in_every_kind(plan, P):
    """condition 1; what is lacking is lacking in the vocabulary: every blank + letter is a token"""
    have = {(e.kind, e.length) for e in plan.everything}
    lacking = set(P.lacking)
    assert lacking == {("rare", 2), ("words", 2)}
    assert all(bytes([32, c]) in P.ranks for c in b"abcdefghijklmnopqrstuvwxyz")
    for path in mc.PATH_NAMES:
        for length in mc.lengths_of(path):
            for kind in mc.kinds_of(path):
                assert (kind, length) in have or (kind, length) in lacking, (path, kind, length)
    for e in plan.everything:
        assert e.length > P.max_token or P.count(e.piece) >= 2, e
    assert any(max(P.tokens(e.piece)) >= 65536 for e in plan.everything if e.kind == "multi")


def test_every_mutant_changes_some_piece_of_every_path(plan, P, ref):
    """condition 2, against the oracle: were a kernel wrong in that way, its tokens would differ from the oracle's"""
    todo = {(path, m) for path in mc.PATH_NAMES for m in merge_ref.MUTANTS if path != "tiny" or m == "rightmost"}
    hits = {}
    for e in plan.everything:
        if e.piece not in ref:
            continue
        for m in merge_ref.MUTANTS:
            if (e.path, m) in todo and hits.get((e.path, m), 0) < 3:
                if merge_ref.merge_ref(e.piece, P.ranks, m)[0] != P.tokens(e.piece):
                    hits[(e.path, m)] = hits.get((e.path, m), 0) + 1
    assert set(hits) == todo, sorted(todo - set(hits))
    # ... and the kinds are both needed: some piece is blind to each mutant
    assert any(merge_ref.merge_ref(e.piece, P.ranks, "rightmost")[0] == P.tokens(e.piece) for e in plan.base if e.kind == "words")


def test_result_words(plan, P):
    """condition 3: token counts around the seven ids of a result word, and ids of 17 bits at each of its positions"""
    by = _by_path(plan)
    for path in mc.LEAN + mc.STATE:
        counts = {P.count(e.piece) for e in by[path]}
        print(path, "token counts:", sorted(counts))
        assert min(counts) <= 6 and 7 in counts, (path, sorted(counts))
        assert 8 in counts or path == "b0", (path, sorted(counts))
    for writer, paths in (("lean_bin", mc.LEAN), ("merge_bin", mc.STATE)):
        high = set()
        for path in paths:
            for e in by[path]:
                tk = P.tokens(e.piece)
                if len(tk) <= 7:
                    high |= {k for k, t in enumerate(tk) if t >= 65536}
        assert high == set(range(7)), (writer, sorted(high))


def _chunks(tr, k):
    prev = tr.pos[k] - tr.prev_len[k]
    return len({int(tr.pos[k]) // mc.GIANT_CHUNK, int(tr.removed[k]) // mc.GIANT_CHUNK, int(prev) // mc.GIANT_CHUNK})


def test_far_neighbours_and_chunks(plan, P, ref):
    """condition 4"""
    by = _by_path(plan)
    for path in ("mid", "long", "giant"):
        traces = [ref[e.piece][1] for e in by[path] if e.piece in ref]
        assert traces
        assert any(tr.ahead.max() > 64 for tr in traces), path
        assert any(tr.prev_len.max() > 64 for tr in traces), path
    spans = set()
    for tr in (ref[e.piece][1] for e in by["giant"] if e.piece in ref):
        spans |= {_chunks(tr, k) for k in range(len(tr))}
    # three chunks would take a chosen and a previous part of 257 bytes together: no token is that long
    assert spans == {1, 2} and 2 * P.max_token < mc.GIANT_CHUNK + 1, (spans, P.max_token)


def test_defect_ties_straddle_the_edges(plan, P):
    """condition 5: a step whose minimum stands at or before slot `edge` and again after it, in a piece whose tokens depend on
    which of the tied positions goes first"""
    found = set()
    for e in plan.defect:
        unit, edge = re.search(r"/(\w+)-edge(\d+)@", e.label).groups()
        tokens, tr = merge_ref.merge_ref(e.piece, P.ranks)
        assert tokens == P.tokens(e.piece)
        if np.any(tr.tie & (tr.pos <= int(edge)) & (tr.last > int(edge))):
            found.add((unit == "ab", int(edge), P.mutant_changes(e.piece, "rightmost")))
    # the issue's "ab" pieces tie across every edge, and so do pieces whose tokens depend on which tied position goes first
    assert {(ab, edge) for ab, edge, _ in found} >= {(True, 63), (True, 511), (True, 8191)}, found
    assert {edge for _, edge, shows in found if shows} == {63, 511, 8191}, found


def test_lean_paths_take_the_second_lookup_round(plan, P):
    """condition 6"""
    by = _by_path(plan)
    for path in mc.LEAN:
        st = [P.sim.stats(e.piece) for e in by[path]]
        assert any(s[1] for s in st) and any(s[2] for s in st), path


@pytest.fixture(scope="module")
def per_piece(plan):
    return plan.per_piece()


def _shard_counts(P, t):
    """hard pieces per shard (tile % 64) and path"""
    n = mc.tile_counts(P, t)
    per = np.zeros((mc.Q_SHARDS, n.shape[1]), dtype=np.int64)
    for tile in range(len(n)):
        per[tile % mc.Q_SHARDS] += n[tile]
    return per


def test_texts_split_as_planned(plan, P, per_piece):
    """per_piece, its tails, one_document and second_chunk; every text-reading edge length stands at every placement"""
    n = mc.check_splits(P, per_piece)
    assert len(per_piece.cases) == len(plan.entries) + 1 and n > len(per_piece.cases)
    seen = {(e.path, e.length, e.place) for _, e in per_piece.cases}
    for path in mc.TEXT_READERS:
        for length in mc.lengths_of(path):
            assert all((path, length, place) in seen for place in mc.PLACES + (None,)), (path, length)
    for at, e in per_piece.cases:
        if e.place in ("a0", "a1", "a15"):
            assert at & 15 == int(e.place[1:]), e
        if e.place == "tile_end":
            assert at % mc.T >= mc.T - 16, e
        if e.place in ("doc_first", "doc_whole"):
            assert at in per_piece.doc_off, e
        if e.place in ("doc_last", "doc_whole"):
            assert at + e.length in per_piece.doc_off, e
    tails = plan.tail_texts()
    assert {(e.path, e.length) for t in tails for _, e in t.cases} == {(p, n) for p in mc.TEXT_READERS for n in mc.lengths_of(p)}
    for t in tails:
        mc.check_splits(P, t)
    one = plan.one_document()
    mc.check_splits(P, one)
    assert len(one.cases) >= len(per_piece.cases) - 12
    second = plan.second_chunk()
    mc.check_splits(P, second)
    kept = {e.path for _, e in second.cases}
    assert kept == set(mc.PATH_NAMES) and second.left_out, kept
    print("second_chunk leaves out %d of %d: %s ..." % (len(second.left_out), len(plan.entries), ", ".join(second.left_out[:6])))


def test_sliced_text_leaves_side_by_side(plan, P):
    """condition 7"""
    t = plan.sliced()
    mc.check_splits(P, t)
    per = _shard_counts(P, t)
    assert t.ballast == 3 * mc.Q_SHARDS * mc.T and t.cases[0][0] > t.ballast
    holding = sorted({at // mc.T % mc.Q_SHARDS for at, _ in t.cases})
    assert len(holding) > mc.Q_SHARDS // 2 and per[holding, 1].min() > mc.ML_THREADS, per[:, 1].min()


def test_crowded_shards_and_long_lists(P):
    """condition 8"""
    t, shards = mc.crowded(P)
    assert len(t.text) < 9 << 20
    mc.check_splits(P, t)
    per = _shard_counts(P, t)
    for path, shard in shards.items():
        assert per[shard, mc.PATH_NAMES.index(path)] > mc.ONE_PASS[path], (path, per[shard].tolist())
    # the same count by pack_stage_cases.profile (bins 0..6, tiny in column 7)
    _, nq = mc.profile(P.w, t.text, t.doc_off)
    assert np.array_equal(nq[:, [7, 0, 1, 2, 3, 4, 5, 6]], mc.tile_counts(P, t)[:, :8])
    assert len({e.piece for _, e in t.cases}) == len(t.cases)
    t = mc.lists(P)
    mc.check_splits(P, t)
    n = {path: sum(e.path == path for _, e in t.cases) for path in ("mid", "long", "giant")}
    assert n["mid"] > mc.GRID_WAVES and n["long"] > mc.GRID_WGS and n["giant"] > mc.GRID_WGS, n
    assert len({e.piece for _, e in t.cases}) == len(t.cases)
