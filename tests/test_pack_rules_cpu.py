"""CPU tier: the packing rule of jtk_batch_pack (jtokkit_amd/csrc/jtk_pack_rules.h), run on the CPU through the shim
tests/pack_sim, against the plain restatement of the rule (tests/pack_ref.py): random unit lengths and the edges -- lengths 0,
L - 1, L, L + 1 and k * L, L = 1, every document refused, one huge unit --, the golden prompts' token lists, with the separator
after (EOS), before (BOS) or absent, in both modes and with drop_last.  Every field is compared: rows, positions, cu_seqlens,
seg_doc and max_seqlen.  The shim restarts its cursors every `run` cells as the lanes of the write kernel do."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import golden_util
import pack_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEP = 100257
PAD = -7
RUNS = (0, 1, 4, 7)
MODES = [(-1, False, False, False), (-1, False, False, True), (-1, False, True, False),
         (SEP, False, False, False), (SEP, False, False, True), (SEP, False, True, False),
         (SEP, True, False, False), (SEP, True, False, True), (SEP, True, True, False)]   # (sep, sep_first, whole, drop_last)


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("pack_sim") / "libpack_sim.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-o", out,
                           os.path.join(ROOT, "tests", "pack_sim", "pack_sim.cpp")])
    L = C.CDLL(out)
    head = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int, C.c_int, C.c_int]
    L.sim_pack_counts.restype = None
    L.sim_pack_counts.argtypes = head + [C.c_void_p]
    L.sim_pack.restype = None
    L.sim_pack.argtypes = head + [C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return L


def _sim(sim, docs, status, L, sep, sep_first, whole, drop, run):
    toks = np.array([t for d in docs for t in d] + [0], dtype=np.int32)
    tok_off = np.zeros(len(docs) + 1, dtype=np.int64)
    np.cumsum([len(d) for d in docs], out=tok_off[1:])
    st = np.array(list(status) + [0], dtype=np.int32)
    counts = np.zeros(3, dtype=np.int64)
    args = (toks.ctypes.data, tok_off.ctypes.data, st.ctypes.data, len(docs), L, sep, int(sep_first), int(whole), int(drop))
    sim.sim_pack_counts(*args, counts.ctypes.data)
    nr, ns, mx = (int(x) for x in counts)
    rows = np.full(nr * L + 1, 12345, dtype=np.int32)
    pos = np.full(nr * L + 1, 12345, dtype=np.int32)
    cu = np.full(ns + 2, 12345, dtype=np.int32)
    sd = np.full(ns + 1, 12345, dtype=np.int64)
    sim.sim_pack(*args, PAD, run, rows.ctypes.data, pos.ctypes.data, cu.ctypes.data, sd.ctypes.data)
    assert rows[-1] == 12345 and pos[-1] == 12345 and cu[-1] == 12345 and sd[-1] == 12345     # nothing past the outputs
    return dict(rows=rows[:-1].reshape(nr, L), positions=pos[:-1].reshape(nr, L), cu_seqlens=cu[:-1], seg_doc=sd[:-1],
                max_seqlen=mx)


def _check(sim, docs, status, L, modes=MODES, runs=RUNS):
    for sep, sep_first, whole, drop in modes:
        exp = pack_ref.pack(docs, status, L, sep, sep_first, whole, drop, PAD)
        for run in runs:
            got = _sim(sim, docs, status, L, sep, sep_first, whole, drop, run)
            for k in ("rows", "positions", "cu_seqlens", "seg_doc"):
                assert np.array_equal(got[k], exp[k]), (k, L, sep, sep_first, whole, drop, run, got[k], exp[k])
            assert got["max_seqlen"] == exp["max_seqlen"], (L, sep, sep_first, whole, drop)


def _docs(lengths, seed=0):
    """Documents of the given lengths with ids that tell every token apart."""
    return [[(d * 7919 + i * 31 + seed) % 100000 for i in range(n)] for d, n in enumerate(lengths)]


def test_random_unit_lengths(sim):
    rng = random.Random(11)
    for L in (1, 2, 3, 5, 8, 16, 64):
        for _ in range(12):
            n = rng.randint(0, 30)
            lengths = [rng.choice([0, 1, max(L - 2, 0), L - 1, L, L + 1, 2 * L, 3 * L - 1, rng.randint(0, 3 * L)]) for _ in range(n)]
            status = [-1 if rng.random() < 0.1 else 0 for _ in range(n)]
            _check(sim, _docs(lengths, rng.randint(0, 99)), status, L)


@pytest.mark.parametrize("L", [1, 4, 7])
def test_edge_lengths(sim, L):
    """Lengths 0, L - 1, L, L + 1, k * L in every order that matters for next-fit and for row boundaries."""
    edges = [0, L - 1, L, L + 1, 3 * L]
    for a in edges:
        for b in edges:
            _check(sim, _docs([a, b, a]), [0, 0, 0], L, runs=(0, 4))
    _check(sim, _docs(edges), [0] * len(edges), L)
    _check(sim, _docs([L - 1] * 5 + [1] * 5 + [L] * 3), [0] * 13, L)


def test_all_documents_refused_and_no_documents(sim):
    for sep, sep_first, whole, drop in MODES:
        got = _sim(sim, _docs([3, 0, 9]), [-1, -2, -1], 4, sep, sep_first, whole, drop, 0)
        assert got["rows"].shape == (0, 4) and got["cu_seqlens"].tolist() == [0] and len(got["seg_doc"]) == 0
        assert got["max_seqlen"] == 0
        got = _sim(sim, [], [], 4, sep, sep_first, whole, drop, 0)
        assert got["rows"].shape == (0, 4) and got["cu_seqlens"].tolist() == [0]
    _check(sim, _docs([0, 0, 0]), [0, 0, 0], 3)              # empty units without a separator are dropped


def test_one_huge_unit(sim):
    _check(sim, _docs([20000]), [0], 128, runs=(0, 4))
    _check(sim, _docs([5, 20000, 3]), [0, 0, 0], 2048, runs=(0, 4))
    _check(sim, _docs([1000]), [0], 1, runs=(0, 7))


def test_drop_last_leaves_out_a_short_stream(sim):
    got = _sim(sim, _docs([2, 3]), [0, 0], 8, -1, False, False, True, 0)
    assert got["rows"].shape == (0, 8) and got["max_seqlen"] == 0 and got["cu_seqlens"].tolist() == [0]


def test_golden_prompts(sim):
    docs = [toks for (_, toks, _) in golden_util.load_rows("cl100k_base")]
    for L in (1, 7, 128):
        _check(sim, docs, [0] * len(docs), L, runs=(0, 4))


def test_restatement_by_hand():
    """pack_ref itself on a case worked out by hand: L = 4, EOS 9, units [1 2 9] [3 9] [4 5 6 7 8 9]."""
    docs, status = [[1, 2], [3], [4, 5, 6, 7, 8]], [0, 0, 0]
    c = pack_ref.pack(docs, status, 4, 9, pad_id=0)
    assert c["rows"].tolist() == [[1, 2, 9, 3], [9, 4, 5, 6], [7, 8, 9, 0]]
    assert c["positions"].tolist() == [[0, 1, 2, 0], [0, 0, 1, 2], [0, 1, 2, 0]]
    assert c["cu_seqlens"].tolist() == [0, 3, 4, 5, 8, 11, 12] and c["seg_doc"].tolist() == [0, 1, 1, 2, 2, -1]
    assert c["max_seqlen"] == 3
    w = pack_ref.pack(docs, status, 4, 9, whole=True, pad_id=0)
    assert w["rows"].tolist() == [[1, 2, 9, 0], [3, 9, 0, 0], [4, 5, 6, 7], [8, 9, 0, 0]]
    assert w["cu_seqlens"].tolist() == [0, 3, 4, 6, 8, 12, 14, 16] and w["seg_doc"].tolist() == [0, -1, 1, -1, 2, 2, -1]
    b = pack_ref.pack(docs, status, 4, 9, sep_first=True, drop_last=True, pad_id=0)
    assert b["rows"].tolist() == [[9, 1, 2, 9], [3, 9, 4, 5]]


def test_large_batch_restatement_agrees():
    """pack_ref.row_starts / segments / row (the restatement the 200k-document GPU test uses) against pack_ref.pack."""
    rng = random.Random(5)
    for L in (1, 3, 16):
        for whole, drop in ((False, False), (False, True), (True, False)):
            for _ in range(10):
                lengths = [rng.choice([1, L, L + 1, rng.randint(1, 3 * L)]) for _ in range(rng.randint(0, 25))]
                docs = _docs(lengths)
                exp = pack_ref.pack(docs, [0] * len(docs), L, whole=whole, drop_last=drop, pad_id=PAD)
                a = pack_ref.row_starts(lengths, L, whole, drop)
                U = np.concatenate([[0], np.cumsum(lengths)])[:-1].astype(np.int64)
                cu, sd, mx = pack_ref.segments(U, np.arange(len(docs)), a, L)
                assert np.array_equal(cu, exp["cu_seqlens"]) and np.array_equal(sd, exp["seg_doc"]) and mx == exp["max_seqlen"]
                S = np.array([t for d in docs for t in d], dtype=np.int64)
                for r in range(len(a) - 1):
                    ids, pos = pack_ref.row(S, U, a, r, L, PAD)
                    assert np.array_equal(ids, exp["rows"][r]) and np.array_equal(pos, exp["positions"][r])
