"""CPU tier: where k_pack_tokens keeps a tile's merge results in LDS (jtokkit_amd/csrc/jtk_stage_rules.h), run on the CPU
through the shim tests/stage_sim.  Every token total 0..800 against result counts at and around the heads' caps and the free
room: the extension slots are whole 16-byte slots inside the array, disjoint from each other and from the words the tile's
tokens take, never more than a bin has beyond its head, handed out in bin order until the room is gone -- and equal to a
plain restatement of the rule.  Every comparison is exact."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN_CAP = (512, 256, 160, 128, 64, 32, 16)      # JTK_BIN_CAP0..6: the most results a 2 KiB tile can have per bin
CAP = (32, 16, 16, 8, 8, 8, 8)                  # the heads, as k_piece_resolve marks them (JTK_PACK_CAP)
HEAD = (0, 32, 48, 64, 72, 80, 88)              # JTK_PACK_OFF
SLOTS, OUT_SLOTS, STAGE, NB = 96, 192, 768, 7


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("stage_sim") / "libstage_sim.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-o", out,
                           os.path.join(ROOT, "tests", "stage_sim", "stage_sim.cpp")])
    L = C.CDLL(out)
    for f in (L.sim_stage_const, L.sim_stage_cap, L.sim_stage_head):
        f.restype, f.argtypes = C.c_int, [C.c_int]
    L.sim_stage_rules.restype = None
    L.sim_stage_rules.argtypes = [C.c_int64] + [C.c_void_p] * 5
    return L


def _run(sim, total, nq):
    total = np.ascontiguousarray(total, dtype=np.uint32)
    nq = np.ascontiguousarray(nq, dtype=np.uint32)
    m = len(total)
    assert nq.shape == (m, NB)
    off, n, word = (np.full((m, NB), 0xFFFFFFFF, dtype=np.uint32) for _ in range(3))
    sim.sim_stage_rules(m, total.ctypes.data, nq.ctypes.data, off.ctypes.data, n.ctypes.data, word.ctypes.data)
    return off.astype(np.int64), n.astype(np.int64), word.astype(np.int64)


def _first_free(total):
    total = np.asarray(total, dtype=np.int64)
    return np.where(total > STAGE, 0, (total + 3) // 4)


def _restated(total, nq):
    """The rule, said again: greedy in bin order over the free slots."""
    over = np.maximum(nq.astype(np.int64) - np.array(CAP), 0)
    first = _first_free(total)[:, None]
    room = OUT_SLOTS - first
    cum = np.cumsum(over, axis=1)
    start, end = np.minimum(cum - over, room), np.minimum(cum, room)
    return SLOTS + first + start, end - start


def _nq_vectors(total):
    """Counts at and around every edge for a tile of `total` tokens: bins 0..2 in all combinations, the longer bins together."""
    room = OUT_SLOTS - int(_first_free(total))
    cand = [sorted({min(v, BIN_CAP[b]) for v in (0, CAP[b] - 1, CAP[b], CAP[b] + 1, CAP[b] + room, CAP[b] + room + 1, BIN_CAP[b])
                    if v >= 0}) for b in range(NB)]
    tails = [tuple(0 for _ in range(3, NB)), tuple(CAP[b] for b in range(3, NB)), tuple(CAP[b] + 1 for b in range(3, NB)),
             tuple(BIN_CAP[b] for b in range(3, NB)), (CAP[3] + room, 0, 0, BIN_CAP[6])]
    tails = [tuple(min(v, BIN_CAP[3 + i]) for i, v in enumerate(t)) for t in tails]
    return [h + t for h in itertools.product(cand[0], cand[1], cand[2]) for t in tails]


def test_constants_are_what_the_list_entries_assume(sim):
    assert [sim.sim_stage_const(k) for k in range(4)] == [SLOTS, OUT_SLOTS, STAGE, NB]
    assert tuple(sim.sim_stage_cap(b) for b in range(NB)) == CAP
    assert tuple(sim.sim_stage_head(b) for b in range(NB)) == HEAD
    assert HEAD[-1] + CAP[-1] == SLOTS and OUT_SLOTS * 4 == STAGE
    for b in range(NB - 1):                                   # the heads tile the head slots
        assert HEAD[b] + CAP[b] == HEAD[b + 1]


def test_every_total_against_counts_at_the_edges(sim):
    totals, nqs = [], []
    for total in range(0, 801):
        v = _nq_vectors(total)
        totals += [total] * len(v)
        nqs += v
    total = np.array(totals, dtype=np.int64)
    nq = np.array(nqs, dtype=np.int64)
    assert len(total) > 300000
    off, n, word = _run(sim, total, nq)
    over = np.maximum(nq - np.array(CAP), 0)
    first = _first_free(total)
    room = OUT_SLOTS - first
    # whole slots inside the array, above the words [0, total) of a staged tile (an unstaged tile assembles nothing in LDS)
    assert (n >= 0).all() and (off >= SLOTS).all() and (off + n <= SLOTS + OUT_SLOTS).all()
    staged = total <= STAGE
    assert ((off[staged] - SLOTS) * 4 >= total[staged, None]).all()
    assert (off[~staged, 0] == SLOTS).all()
    # disjoint, in bin order, back to back from the first free slot
    assert (off[:, 0] == SLOTS + first).all()
    assert (off[:, 1:] >= off[:, :-1] + n[:, :-1]).all()
    # never more than the bin has beyond its head
    assert (n <= over).all()
    # in order until the room is gone: a bin that is cut short leaves nothing for the bins after it, and no slot stays
    # free while a result waits
    short = n < over
    after_short = np.cumsum(short, axis=1) - short > 0
    assert (n[after_short] == 0).all()
    assert (n.sum(axis=1) == np.minimum(over.sum(axis=1), room)).all()
    # the restatement
    eo, en = _restated(total, nq)
    assert np.array_equal(n, en) and np.array_equal(off, eo)
    # the word a step reads: result i of a bin is in LDS iff cap <= i < cap + n, at slot off + i - cap
    cap = np.array(CAP)
    has = n > 0
    assert (word[~has] == 0).all()
    assert np.array_equal((word >> 16)[has], (cap + n)[has]) and np.array_equal((word & 0xFFFF)[has], (off - cap)[has])
    # the targeted edges were reached: a bin cut short, a bin that got nothing, exactly full, one slot left
    assert short.any() and (after_short & (over > 0)).any()
    assert (over.sum(axis=1) == room).any() and (over.sum(axis=1) == room - 1).any() and (over.sum(axis=1) == room + 1).any()
    assert (room == 0).any() and (room == 1).any()


def test_768_is_staged_and_769_is_not(sim):
    nq = np.array([[300, 40, 20, 9, 0, 0, 0]] * 4, dtype=np.int64)
    off, n, _ = _run(sim, np.array([765, 768, 769, 5000]), nq)
    # 765..768 tokens fill all 192 slots of the assembly area: no room
    assert (n[:2] == 0).all()
    # one token more: the tile writes to memory and all 192 slots are free
    assert n[2].tolist() == [192, 0, 0, 0, 0, 0, 0] and off[2, 0] == SLOTS
    assert np.array_equal(n[2], n[3]) and np.array_equal(off[2], off[3])
    nq = np.array([[40, 20, 18, 9, 8, 0, 12]] * 3, dtype=np.int64)
    off, n, _ = _run(sim, np.array([764, 760, 769]), nq)
    assert n[0].tolist() == [1, 0, 0, 0, 0, 0, 0] and off[0, 0] == SLOTS + 191          # a staged tile with one free slot
    assert n[1].tolist() == [2, 0, 0, 0, 0, 0, 0] and off[1, 0] == SLOTS + 190
    assert n[2].tolist() == [8, 4, 2, 1, 0, 0, 4]
    assert off[2].tolist() == [96, 104, 108, 110, 111, 111, 111]
