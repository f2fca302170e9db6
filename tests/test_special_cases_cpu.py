"""CPU tier of the allow-special case set (tests/special_cases.py, run on the GPU by tests/test_special_edges_gpu.py): the model --
the batch walked as the kernels of jtk_special.hip walk it, tests/special_sim's batch entry points on the shared rule header --
returns the restatement's answer (tests/special_ref.py) on every document of every case, allowed set and mode, and the oracle
refuses no segment, so that the GPU tier skips nothing; the set reaches every edge it names, read from the model's answer, so
that the GPU tier cannot pass by missing one; and the set tells every wrong version of the batch logic (the sim's mutants) from
the right one, each in the group built for it.  No GPU.

M_no_tail_mask cannot be told from the rule by any text: jtk_special_scan_at refuses every start at or behind its `end`, and
both scans end at n_bytes or before, so the `left < 16` mask of k_sp_find only spares work.  The test asserts exactly that (no
disagreement with the padding bytes supplied), and kills the wrong rule next to it that does change answers, M_pad_end: the mask
off and the batch taken to end where its last granule does."""
import os
import re
import subprocess

import pytest

import special_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = sc.cases()
NAMES = [c.name for c in CASES]
BY_NAME = sc.by_name()
GROUPS = ("find/lane", "find/wave", "find/block", "find/doc-boundary", "find/batch-end", "docs/empties", "chains", "stitch")


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("special_sim") / "libspecial_sim.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-o", out,
                           os.path.join(ROOT, "tests", "special_sim", "special_sim.cpp")])
    return sc.load_sim(out)


_models = {}


def _model(sim, c, allowed, ordinary):
    key = (c.name, allowed, ordinary)
    if key not in _models:
        _models[key] = sc.model(sim, c, allowed, ordinary)
    return _models[key]


def _group(kind):
    return [c for c in CASES if c.kind == kind]


# ---- (a) the set itself
def test_case_set_shape():
    assert {c.kind for c in CASES} == set(GROUPS)
    assert all(sum(len(d) for d in c.docs) < sc.LIMIT for c in CASES)
    big = [c for c in CASES if sum(len(d) for d in c.docs) > 4096]
    assert len(big) <= 48, len(big)                               # (the batch-end batches are 64..79 bytes each)
    for c in CASES:
        assert c.modes == (False, True) and len(c.allowed) >= 1
        assert c.enc == sc.CL100K or c.enc in sc.CUSTOM
        assert [d for d in range(len(c.docs)) if not sc.valid_utf8(c.docs[d])] == list(c.invalid)
        assert not c.invalid or c.validate
    text = b"".join(d for c in CASES if c.enc == "sp_find" for d in c.docs)
    for decoy in (b"< ", b"<| ", b"<|endoftext| ", b"# ", b"{s ", b"[q ", b"( "):
        assert decoy in text, decoy


def test_partition_constants_are_the_sources():
    src = lambda f: open(os.path.join(ROOT, "jtokkit_amd", "csrc", f)).read()
    k = src("jtk_special.hip")
    block = int(re.search(r"^#define\s+JTK_SPECIAL_BLOCK\s+(\d+)", src("jtk_kernels.h"), re.M).group(1))
    ft = int(re.search(r"constexpr int FT = (\d+);", k).group(1))
    gt, gper = map(int, re.search(r"constexpr int GT = (\d+), GPER = (\d+);", k).groups())
    assert (block, ft, gt, gper) == (sc.BLOCK, sc.FT, sc.GT, sc.GPER)
    assert sc.LANE * ft == block and sc.WAVE == 64 * sc.LANE and sc.GATHER_WG == gt * gper
    assert "(int64_t)tid * 16" in k and "left < 16" in k
    assert "w.n_bytes / (4 * GT * GPER) + 1" in k and sc.GATHER_BYTES == 4 * gt * gper
    for kern in ("k_sp_resolve", "k_sp_walk", "k_sp_docs", "k_sp_subs", "k_sp_count"):
        assert "__launch_bounds__(%d) %s" % (sc.LAUNCH, kern) in k
    assert "value < (1 << 16)" in src("jtk_abi.cpp") and sc.MIN_CHUNK == 1 << 16


# ---- (b) the model against the restatement, and nothing skipped
@pytest.mark.parametrize("kind", GROUPS)
def test_model_equals_the_restatement_on_every_document(sim, kind):
    """(sc.model raises where the oracle refuses a segment: no document but the declared invalid ones goes unencoded)"""
    runs = 0
    for c in _group(kind):
        for allowed, ordinary in sc.combos(c):
            m = _model(sim, c, allowed, ordinary)
            exp = sc.expected(c, allowed, ordinary)
            for d in range(len(c.docs)):
                assert (m.status[d], m.docs[d]) == (exp[d][0], list(exp[d][1])), (c.name, allowed, ordinary, d, c.docs[d][:60])
            assert [d for d in range(len(c.docs)) if m.status[d] == -6] == list(c.invalid)
            assert m.tok_off[-1] == m.total == sum(len(t) for _, t in exp)
            assert (sc.np.diff(m.sub_off) >= 0).all(), c.name                # sub_off non-decreasing over the whole batch
            runs += 1
    assert runs >= 2


def test_refusals_are_the_ones_built():
    c = BY_NAME["find_doc_boundary"]
    # the prefix literal outside the allowed set: -2 for exactly the documents that hold it whole
    st = [s for s, _ in sc.expected(c, (sc.EOT,), False)]
    assert [d for d, s in enumerate(st) if s == -2] == [d for d, doc in enumerate(c.docs) if sc.PRE in doc]
    assert st[0] == st[1] == st[2] == st[3] == 0 and st[4] == -2 and st[5] == 0          # `<` | `|e…`, `<|` | `e…`, `<|e` | `nd…`
    # the long literal outside the allowed set straddles every boundary: nothing is refused, the prefix literal matches
    exp = sc.expected(c, (sc.PRE,), False)
    assert [d for d, (s, _) in enumerate(exp) if s == -2] == [len(c.docs) - 2]
    for k in range(3, 13):
        assert exp[2 * (k - 1)][1][-1] == 100300 if k == 3 else 100300 in exp[2 * (k - 1)][1]
    for name, status in (("stitch_refused_special", -2), ("stitch_refused_utf8", -6)):
        c = BY_NAME[name]
        exp = sc.expected(c, c.allowed[0], False)
        assert [s for s, _ in exp] == [0, status, 0, 0, 0]
        assert c.docs[1].count(sc.L1) >= 20
        c = BY_NAME[name + "_no_candidate"]                         # refused, and no allowed literal in the whole batch
        exp = sc.expected(c, c.allowed[0], False)
        assert [s for s, _ in exp] == [0, status, 0, 0] and not any(x in d for d in c.docs for x in sc.amap(c.enc, c.allowed[0]))


# ---- (c) reach, from the model's answer
def test_find_sweeps_reach_every_offset(sim):
    for kind, edges in (("find/lane", (sc.LANE,)), ("find/wave", (sc.WAVE,)), ("find/block", (sc.BLOCK, 2 * sc.BLOCK))):
        got = {}
        for c in _group(kind):
            lits = list(sc.specials(c.enc))
            for key, deltas in sc.sweep_reached(_model(sim, c, None, True), lits).items():
                got.setdefault(key, set()).update(deltas)
        for edge in edges:
            for lit in sc.SWEEP_LITS:
                missing = sc.sweep_required(lit) - got.get((edge, lit), set())
                assert not missing, (kind, edge, lit[:16], sorted(missing))
    assert [len(x) for x in sc.SWEEP_LITS] == [13, 1, 2, 17, 300]


def test_find_dense_shapes(sim):
    c = BY_NAME["find_dense"]
    m = _model(sim, c, None, True)
    pos = m.cand_pos
    per_lane = sc.np.bincount(pos // sc.LANE)
    assert per_lane.max() == 16 and (per_lane[sc.BLOCK // sc.LANE:2 * sc.BLOCK // sc.LANE] == 16).all()     # a lane, a whole block
    per_wave = sc.np.bincount(pos // sc.WAVE, minlength=12)
    w = 2 * sc.BLOCK // sc.WAVE
    assert per_wave[w] > 0 and per_wave[w + 1] == 0 and per_wave[w + 2] > 0          # an empty wave between two that hold some
    first = set(b"<@#{[(")
    text = b"".join(c.docs)
    assert not first & set(text[(w + 1) * sc.WAVE:(w + 2) * sc.WAVE])                 # (not even a decoy: the ballot skips it)
    lits = list(sc.specials(c.enc))
    long = [int(p) for p, li in zip(pos, m.cand_lit) if lits[li] == sc.L4100]
    assert long == list(sc.LONG_STARTS) and len(sc.L4100) == 4100 and long[0] % sc.BLOCK == sc.BLOCK - 6
    assert (long[1] + 4100 - 1) // sc.BLOCK - long[1] // sc.BLOCK == 2               # three find blocks


def test_batch_end_reaches_every_remainder():
    exact, short = {}, {}
    for c in _group("find/batch-end"):
        text = b"".join(c.docs)
        if c.pad:
            assert not text.endswith(sc.EOT) and (text + c.pad).endswith(sc.EOT) and 1 <= len(c.pad) <= 3
            short[len(text) % 16] = len(c.pad)
        else:
            assert text.endswith(sc.EOT)
            exact[len(text) % 16] = True
    assert sorted(exact) == sorted(short) == list(range(16)) and set(short.values()) == {1, 2, 3}


def test_doc_boundary_cuts_every_position(sim):
    c = BY_NAME["find_doc_boundary"]
    cuts = set()
    for a, b in zip(c.docs, c.docs[1:]):
        for k in range(1, len(sc.EOT)):
            if a.endswith(sc.EOT[:k]) and b.startswith(sc.EOT[k:]):
                cuts.add(k)
    assert cuts == set(range(1, 13))
    m = _model(sim, c, None, True)
    lits = list(sc.specials(c.enc))
    off = sc._pack(c.docs)[1]
    ends = m.cand_pos + m.cand_len
    assert (ends <= off[m.cand_doc + 1]).all()
    assert sum(1 for li in m.cand_lit if lits[li] == sc.EOT) == 1 and sum(1 for li in m.cand_lit if lits[li] == sc.PRE) == 11


def test_docs_group_reach(sim):
    counts = {len(c.docs) for c in _group("docs/empties")}
    assert set(sc.DOC_COUNTS) <= counts
    for r in sc.EMPTY_RUNS:
        c = BY_NAME["docs_empties_%d" % r]
        lens = [len(d) for d in c.docs]
        assert lens[:r] == [0] * r and lens[-r:] == [0] * r and lens[r] > 0 and lens[2 * r + 1] > 0 and lens[r + 1:2 * r + 1] == [0] * r
        assert c.docs[r].endswith(sc.EOT) and c.docs[2 * r + 1].startswith(sc.EOT) and sc.EOT in c.docs
        m = _model(sim, c, None, True)
        off = sc._pack(c.docs)[1]
        assert (off[m.cand_doc] <= m.cand_pos).all() and (m.cand_pos < off[m.cand_doc + 1]).all()
        assert (m.cand_pos == off[m.cand_doc]).sum() >= 3                                      # candidates exactly at doc_off[d]
    off = set(sc._pack(BY_NAME["docs_aligned"].docs)[1].tolist())
    assert {16, 32, 1024, 4096, 8192} <= off


def test_two_chunk_cases_cut_behind_a_literal_slot(sim):
    """The chunk plan cuts at the first sub-document that starts at or behind a multiple of the chunk size."""
    for name, empties in (("chains_two_chunks", 4), ("docs_two_chunks", 300)):
        c = BY_NAME[name]
        assert sum(len(d) for d in c.docs) > sc.MIN_CHUNK + sc.MIN_CHUNK // 4
        m = _model(sim, c, None, True)
        k = int(sc.np.searchsorted(m.sub_off[:-1], sc.MIN_CHUNK))
        assert m.sub_lit[k - 1] >= 0 and m.sub_off[k - 1] < sc.MIN_CHUNK < m.sub_off[k] and m.sub_lit[k] == -1      # literal | its segment
        assert (m.sub_off[k:k + 1 + empties] == m.sub_off[k]).all()                      # ... and the empty slots behind it
        assert (m.sub_lit[k + 1:k + 1 + empties] == (-2 if name.startswith("chains") else -1)).all()


def test_chains_cross_the_launch_blocks_and_a_find_block(sim):
    for c in _group("chains"):
        if c.name == "chains_two_chunks":
            continue
        m = _model(sim, c, None, True)
        ch = sc.chains(m)
        for edge in (sc.LAUNCH, 2 * sc.LAUNCH):
            assert any(a <= edge - 1 and edge <= b for a, b in ch), (c.name, edge)
        assert any(m.cand_pos[a] < sc.BLOCK <= m.cand_pos[b] for a, b in ch), c.name
        # the pair of documents that cuts a run: the second one's first candidate is certain although the candidate before it
        # starts fewer than maxlen bytes before
        off = sc._pack(c.docs)[1]
        i = int(sc.np.searchsorted(m.cand_pos, off[3]))
        maxlen = max(len(x) for x in sc.specials(c.enc))
        assert m.cand_pos[i] == off[3] and m.keep[i] == 1 and m.cand_pos[i] - m.cand_pos[i - 1] < maxlen, c.name
    m = _model(sim, BY_NAME["chains_aba"], None, True)
    exact = [i for i in range(1, len(m.keep)) if m.cand_len[i - 1] == 3 and m.cand_pos[i] - m.cand_pos[i - 1] == 2 and m.cand_len[i] == 1
             and m.keep[i] == 0 and (i + 1 == len(m.keep) or m.cand_pos[i + 1] > m.cand_pos[i] + 2) and m.keep[i - 1] == 1]
    assert len(exact) >= 10                                       # starts maxlen - 1 before p, ends at p + 1: the look-back's limit


def test_stitch_totals_rounds_and_empty_runs(sim):
    totals = [_model(sim, BY_NAME["stitch_total_%d" % t], None, True).total for t in sc.STITCH_TOTALS]
    assert totals == list(sc.STITCH_TOTALS) == [sc.GATHER_WG - 1, sc.GATHER_WG, sc.GATHER_WG + 1, 2 * sc.GATHER_WG - 1, 2 * sc.GATHER_WG,
                                                2 * sc.GATHER_WG + 1]
    second_round = [t for t in sc.STITCH_TOTALS
                    if t > sc.GATHER_WG * (sum(len(d) for d in BY_NAME["stitch_total_%d" % t].docs) // sc.GATHER_BYTES + 1)]
    assert second_round == [4097, 8191, 8192, 8193]
    m = _model(sim, BY_NAME["stitch_empty_run"], None, True)
    assert sc.longest_flat_run(m) >= 600 and int((m.keep == 0).sum()) >= 300
    for name in ("stitch_refused_special", "stitch_refused_utf8"):
        c = BY_NAME[name]
        m = _model(sim, c, c.allowed[0], False)
        assert int((m.cand_doc == 1).sum()) >= 20 and m.status[1] < 0 and m.tok_off[1] == m.tok_off[2] > 0 and m.total > m.tok_off[2]


# ---- (d) the set tells every wrong rule from the right one
KILLED_BY = dict(M_batch_end="find/doc-boundary", M_doc_ge="docs/empties", M_first_match="chains", M_window="chains",
                 M_chain_docs="chains", M_empty_at_self="chains", M_keep_j="stitch", M_pad_end="find/batch-end")


def _disagreements(sim, kind, mutant):
    out = []
    for c in _group(kind):
        for allowed, ordinary in sc.combos(c):
            out += [(c.name, allowed, ordinary, d) for d in sc.wrong(sim, c, allowed, ordinary, sc.MUTANTS[mutant])]
    return out


@pytest.mark.parametrize("mutant", sorted(KILLED_BY))
def test_mutant_is_killed_by_its_group(sim, mutant):
    bad = _disagreements(sim, KILLED_BY[mutant], mutant)
    assert bad, mutant
    if mutant == "M_window":
        assert "chains_aba" in {n for n, _, _, _ in bad}
    if mutant == "M_chain_docs":                                  # the document behind the cut of a run, in every chain set
        assert {(n, d) for n, a, o, d in bad if a is None} >= {(n, 3) for n in ("chains_a", "chains_abab", "chains_aba")}
    if mutant == "M_pad_end":
        assert {n for n, _, _, _ in bad} == {c.name for c in _group("find/batch-end") if c.pad and sum(map(len, c.docs)) % 16}
    if mutant == "M_keep_j":
        assert {n for n, _, _, _ in bad} >= {"stitch_total_%d" % t for t in sc.STITCH_TOTALS}


def test_tail_mask_mutant_is_equivalent(sim):
    """See the module's docstring: with the padding bytes that complete the literal supplied, the answer does not change."""
    assert set(sc.MUTANTS) == set(KILLED_BY) | {"M_no_tail_mask"}
    assert _disagreements(sim, "find/batch-end", "M_no_tail_mask") == []
    assert sum(1 for c in _group("find/batch-end") if c.pad) == 16
