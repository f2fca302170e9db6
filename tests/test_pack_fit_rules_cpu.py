"""CPU tier: the batched best-fit step of jtk_batch_pack_best_fit (jtokkit_amd/csrc/jtk_pack_fit_rules.h), run on the CPU
through the shim tests/pack_fit_sim, against the one-rest-at-a-time restatement (tests/pack_fit_ref.py): random unit lengths
skewed small, so that rows absorb several rests and runs split.  Every field is compared: rows (contents and order), positions,
cu_seqlens, seg_doc and max_seqlen.  The shim restarts its cursor every `run` cells as the lanes of the write kernel do."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import pack_fit_ref
import pack_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEP = 100257
PAD = -7
SEPS = [(-1, False), (SEP, False), (SEP, True)]


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("pack_fit_sim") / "libpack_fit_sim.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-o", out,
                           os.path.join(ROOT, "tests", "pack_fit_sim", "pack_fit_sim.cpp")])
    L = C.CDLL(out)
    head = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int]
    L.sim_fit_counts.restype = None
    L.sim_fit_counts.argtypes = head + [C.c_void_p]
    L.sim_fit.restype = None
    L.sim_fit.argtypes = head + [C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return L


def _sim(sim, docs, status, L, sep, sep_first, run):
    toks = np.array([t for d in docs for t in d] + [0], dtype=np.int32)
    tok_off = np.zeros(len(docs) + 1, dtype=np.int64)
    np.cumsum([len(d) for d in docs], out=tok_off[1:])
    st = np.array(list(status) + [0], dtype=np.int32)
    counts = np.zeros(4, dtype=np.int64)
    args = (toks.ctypes.data, tok_off.ctypes.data, st.ctypes.data, len(docs), L, sep, int(sep_first))
    sim.sim_fit_counts(*args, counts.ctypes.data)
    nr, ns, mx, steps = (int(x) for x in counts)
    rows = np.full(nr * L + 1, 12345, dtype=np.int32)
    pos = np.full(nr * L + 1, 12345, dtype=np.int32)
    cu = np.full(ns + 2, 12345, dtype=np.int32)
    sd = np.full(ns + 1, 12345, dtype=np.int64)
    sim.sim_fit(*args, PAD, run, rows.ctypes.data, pos.ctypes.data, cu.ctypes.data, sd.ctypes.data)
    assert rows[-1] == 12345 and pos[-1] == 12345 and cu[-1] == 12345 and sd[-1] == 12345     # nothing past the outputs
    return dict(rows=rows[:-1].reshape(nr, L), positions=pos[:-1].reshape(nr, L), cu_seqlens=cu[:-1], seg_doc=sd[:-1],
                max_seqlen=mx, steps=steps)


def _check(sim, docs, status, L, runs=(0, 4)):
    steps = 0
    for sep, sep_first in SEPS:
        exp = pack_fit_ref.pack(docs, status, L, sep, sep_first, PAD)
        for run in runs:
            got = _sim(sim, docs, status, L, sep, sep_first, run)
            for k in ("rows", "positions", "cu_seqlens", "seg_doc"):
                assert np.array_equal(got[k], exp[k]), (k, L, sep, sep_first, run, got[k], exp[k])
            assert got["max_seqlen"] == exp["max_seqlen"], (L, sep, sep_first)
            steps = got["steps"]
    return steps


def _docs(lengths, seed=0):
    """Documents of the given lengths with ids that tell every token apart."""
    return [[(d * 7919 + i * 31 + seed) % 100000 for i in range(n)] for d, n in enumerate(lengths)]


@pytest.mark.parametrize("L", [4, 7, 8, 16, 33, 64])
def test_random_lengths_skewed_small(sim, L):
    rng = random.Random(100 + L)
    for _ in range(40):
        n = rng.randint(0, 60)
        lengths = [rng.choice([0, 1, 1, 2, rng.randint(0, max(L // 4, 1)), rng.randint(0, L), L - 1, L, L + 1, 2 * L,
                               rng.randint(0, 3 * L)]) for _ in range(n)]
        status = [-1 if rng.random() < 0.1 else 0 for _ in range(n)]
        _check(sim, _docs(lengths, rng.randint(0, 99)), status, L)


def test_a_step_takes_a_whole_group_of_equal_rests(sim):
    """3000 rests of 5 lengths: the batched driver needs a handful of steps, not one per rest; all-distinct rests longer than
    L / 2 need one step each."""
    lengths = [(3, 5, 9, 17, 30)[d % 5] for d in range(3000)]
    assert _check(sim, _docs(lengths), [0] * 3000, 64, runs=(0,)) <= 16
    lengths = list(range(32, 63))                                      # (the count is that of the last mode: units 33 .. 63)
    assert _check(sim, _docs(lengths), [0] * len(lengths), 64, runs=(0,)) == len(lengths)


def test_restatement_by_hand_and_never_more_rows_than_next_fit():
    """L = 8, no separator, lengths 5 3 3 6 2 9: the full piece of the last document is row 0; the rests 6 5 3 3 2 1 go to
    rows 6|2, 5|3, 3|1 (best fit closes the tightest row first)."""
    docs = _docs([5, 3, 3, 6, 2, 9])
    c = pack_fit_ref.pack(docs, [0] * 6, 8, pad_id=PAD)
    assert c["seg_doc"].tolist() == [5, 3, 4, 0, 1, 2, 5, -1]
    assert c["cu_seqlens"].tolist() == [0, 8, 14, 16, 21, 24, 27, 28, 32] and c["max_seqlen"] == 8
    rng = random.Random(9)
    for L in (4, 16, 64):
        for _ in range(30):
            docs = _docs([rng.randint(0, 2 * L) for _ in range(rng.randint(0, 50))])
            best = pack_fit_ref.pack(docs, [0] * len(docs), L, SEP)
            nxt = pack_ref.pack(docs, [0] * len(docs), L, SEP, whole=True)
            assert len(best["rows"]) <= len(nxt["rows"])
