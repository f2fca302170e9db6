"""resolve_cases.py builds what it says, by the CPU oracle's own split and merges: every case has the stated number of pieces in
the stated tile (and so the stated chunk passes), the edge pieces stand at the stated places of their tile's list and are table
entries or not as stated, the bin tiles queue the stated number of pieces, and every adjacent byte pair inside a piece occurs in
a table entry (pieces_per_tile asserts it), so pretok_split adds no cut of its own."""
import pytest

import resolve_cases as rc


@pytest.fixture(scope="module")
def g():
    return rc.Gen()


def _check(g, case):
    n = rc.pieces_per_tile(g, case.text, case.doc_off)
    for tile, want in case.want.items():
        assert n[tile] == want, (case.label, tile, int(n[tile]), want)
    assert int(n.sum()) == len(case.parts), (case.label, int(n.sum()), len(case.parts))      # the split is the planned pieces
    assert case.text.max() < 128
    return n


def passes(n_pieces, wave):
    """(pair passes, single passes) of one wave over a tile's list: the kernel's loop restated"""
    c, pairs = wave, 0
    while (c + rc.RES_WAVES) * 64 < n_pieces:
        pairs, c = pairs + 1, c + 2 * rc.RES_WAVES
    return pairs, int(c * 64 < n_pieces)


def test_counts_stand_on_both_sides_of_every_pass_edge():
    """np = 64 k + 1 starts chunk k: for k < 4 a wave's first single pass, for k = 4..7 it turns that wave's single pass into a
    pair pass, for k = 8 it adds a single pass behind a pair pass; np = 64 k leaves it out"""
    counts = rc.np_counts()
    for k in (1, 4, 5, 6, 7, 8, 12):
        assert 64 * k in counts and 64 * k + 1 in counts, k
        assert passes(64 * k, k % 4) != passes(64 * k + 1, k % 4), k
    assert passes(256, 0) == (0, 1) and passes(257, 0) == (1, 0) and passes(513, 0) == (1, 1) and passes(1024, 3) == (2, 0)
    assert passes(rc.EDGE_NP, 0) == (1, 1)
    assert rc.EDGE_AT == (0, 63, 4 * 64, 4 * 64 + 63, 8 * 64, 8 * 64 + 63)


@pytest.mark.parametrize("n_pieces", rc.np_counts())
def test_one_tile(g, n_pieces):
    case = rc.one_tile(g, n_pieces)
    n = _check(g, case)
    assert len(n) == 1 and len(case.text) == (rc.T if n_pieces % 2 == 0 else rc.T - 1)


def test_middle_tiles(g):
    case = rc.middle_tiles(g)
    n = _check(g, case)
    assert sorted(case.want.values()) == sorted(rc.np_counts() + (0,))
    raw = case.text.tobytes()
    for tile, want in case.want.items():
        if 0 < want < rc.NP_MOST:                                  # the last piece ends inside the next tile
            assert raw[(tile + 1) * rc.T] != 32 and raw[(tile + 1) * rc.T + 1] == 32, tile
    assert len(n) == len(case.text) // rc.T


def test_length_edges(g):
    case = rc.length_edges(g)
    _check(g, case)
    assert [w[:2] for w in case.what] == [(length, e) for length in rc.EDGE_LENGTHS for e in (True, False)]
    for tile, (length, is_entry, pieces) in enumerate(case.what):
        lst = case.parts[tile * rc.EDGE_NP:(tile + 1) * rc.EDGE_NP]
        assert sum(len(p) for p in lst) == rc.T
        for at, p in zip(rc.EDGE_AT, pieces):
            assert lst[at] == p and len(p) == length and g.o.split(p) == [p]
            assert (p in g.ranks) == is_entry and (g.w.count(p) == 1) == is_entry, (length, is_entry, p)


def test_bin_edges(g):
    case = rc.bin_edges(g)
    _check(g, case)
    q = rc.queued_per_tile(g, case.text, case.doc_off)
    assert len(case.want_q) == 24
    for tile, (b, count) in case.want_q.items():
        assert q[tile, b] == count and q[tile].sum() == count, (tile, b, q[tile].tolist(), count)
        assert count - rc.PACK_CAP[b] in (-1, 0, 1)
    assert rc.PACK_CAP == rc.psc.CAP + (128,) and [rc.psc.bin_of(n) for n in rc.BIN_LEN] == [0, 1, 2, 3, 4, 5, 6, rc.TINY]


def test_rare_chunk(g):
    case = rc.rare_chunk(g)
    _check(g, case)
    lengths = [len(p) for p in case.parts]
    lo, hi = case.second_chunk
    assert lo == 64 and hi <= 128 and max(lengths[:64]) <= 16                   # chunk 0: ordinary pieces only
    assert 300 in lengths[lo:hi] and 600 in lengths[lo:hi] and lengths[case.want[0] - 1] == 9000 and case.want[0] <= 128
    assert lo <= case.gap < hi and lengths[case.gap] <= 16
    assert sum(lengths[:case.want[0] - 1]) < rc.T <= sum(lengths[:case.want[0]])


def test_secondary_slots(g):
    """the shipped <= 8-byte table has entries that share a primary slot; the text holds such entries and absent pieces that must
    look at their secondary slot"""
    import merge_cases
    sim = merge_cases.Sim(rc.NAME)
    sim.L.sim_tok8_bits.argtypes = [merge_cases.C.c_void_p]
    n_slots = sim.L.sim_tok8_bits(sim.h)
    sim.L.sim_tok8_displaced.restype = merge_cases.C.c_double
    sim.L.sim_tok8_displaced.argtypes = [merge_cases.C.c_void_p]
    print("tok8: %d slots, %.2f %% of the entries displaced" % (n_slots, 100 * sim.L.sim_tok8_displaced(sim.h)))
    case = rc.secondary_case(g, n_slots)
    print("entries that share a primary slot: %d; absent pieces at a flagged slot with their filter bit set: %d" % (case.n_displaced, case.n_absent))
    assert case.n_displaced >= 2 and case.n_absent >= 1
    _check(g, case)
