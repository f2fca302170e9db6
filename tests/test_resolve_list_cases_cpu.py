"""resolve_list_cases.py builds what it says, by the CPU oracle's own split and merges: the mask words hold the stated numbers of
piece starts at the stated bits, the one-word tiles have all their pieces in the stated word, and the miss tiles have their
queued pieces at the stated places of the tile's list, in the stated chunks and lanes, and in the stated bin."""
import numpy as np
import pytest

import resolve_list_cases as lc
import resolve_cases as rc


def passes(n_pieces, wave):
    """(pair passes, single passes) of one wave over a tile's list: the kernel's loop restated"""
    c, pairs = wave, 0
    while (c + rc.RES_WAVES) * 64 < n_pieces:
        pairs, c = pairs + 1, c + 2 * rc.RES_WAVES
    return pairs, int(c * 64 < n_pieces)


@pytest.fixture(scope="module")
def g():
    return rc.Gen()


def _planned(g, case):
    """the oracle's split is the planned pieces"""
    st = lc.starts(g, case)
    want = np.cumsum([0] + [len(p) for p in case.parts[:-1]])
    assert np.array_equal(st, want), (case.label, len(st), len(want))
    assert case.text.max() < 128
    return st


def test_word_shapes(g):
    case = lc.word_shapes(g)
    st = _planned(g, case)
    n = lc.word_counts(g, case)
    assert n[:5].tolist() == [64, 63, 1, 0, 1]
    assert 2 * 64 in st and 4 * 64 + 63 in st                      # bit 0 of word 2, bit 63 of word 4
    assert n[0] > 0 and n[lc.TW - 1] > 0 and lc.T - 1 in st         # the tile's first and last word; bit 63 of the last
    assert n[lc.TW] > 0 and lc.T not in st                          # tile 1 begins inside a piece
    assert len(case.text) % 64 != 0 and lc.T < len(case.text) < 2 * lc.T
    assert n[:lc.TW].sum() == 64 + 63 + 1 + 288 + 1                  # (word 4's start is the first of the 288 fillers)


def test_one_word_tiles(g):
    case = lc.one_word_tiles(g)
    _planned(g, case)
    n = lc.word_counts(g, case).reshape(-1, lc.TW)
    assert lc.WORDS_PER_WAVE == 8 and [wd // lc.WORDS_PER_WAVE for wd in lc.ONE_WORD] == list(range(lc.RES_WAVES))   # the kernel's waves
    assert sorted(wd % lc.RES_WAVES for wd in lc.ONE_WORD) == list(range(lc.RES_WAVES))                              # words dealt in turn
    for tile, wd in case.tiles.items():
        assert n[tile, wd] == 6 and n[tile].sum() == 6, (tile, wd, n[tile].tolist())
        own = wd // lc.WORDS_PER_WAVE                              # every other wave's eight words are empty
        assert all(n[tile, 8 * v:8 * v + 8].sum() == (6 if v == own else 0) for v in range(lc.RES_WAVES))
    assert n[case.inside].sum() == 0 and n[case.inside - 1].sum() > 0 and n[case.inside + 1].sum() > 0


def test_second_chunk(g):
    case = lc.second_chunk(g)
    _planned(g, case)
    assert case.doc_off.tolist() == [0, lc.SECOND_BASE, len(case.text)]
    assert lc.CHUNK < lc.SECOND_BASE and len(case.text) <= 2 * lc.CHUNK and lc.SECOND_BASE % lc.T not in (0, lc.T - 1)
    n = lc.word_counts(g, case)
    lead_word = lc.SECOND_BASE // 64
    assert lc.SECOND_BASE % 64 != 0 and n[lead_word] > 1             # starts of both documents in the word that holds the lead
    assert n[lead_word // lc.TW * lc.TW:lead_word].sum() > 0         # ... and the first document's in the words before it


@pytest.mark.parametrize("label", sorted(lc.MISS_TILES))
def test_miss_tiles(g, label):
    case = lc.miss_case(g, label)
    _planned(g, case)
    m = lc.misses(g, case)
    assert len(m) == 1 and len(m[0]) == case.n_pieces
    at = set(np.nonzero(m[0] >= 0)[0].tolist())
    assert at == case.miss_at, (label, sorted(at ^ case.miss_at)[:8])
    want_bin = lc.psc.bin_of(case.hard_len)
    assert all(m[0][i] == want_bin for i in at)


def test_miss_tiles_are_what_their_names_say(g):
    per_chunk = lambda label: np.bincount(np.array(sorted(lc.miss_case(g, label).miss_at)) // 64, minlength=11).tolist()
    assert per_chunk("per_chunk_0_1_63_64")[:5] == [0, 1, 63, 64, 0] and passes(320, 0) == (1, 0) and passes(320, 1) == (0, 1)
    assert per_chunk("pair_all")[:6] == [64, 0, 0, 0, 64, 0] and passes(330, 0) == (1, 0)
    assert {i % 64 for i in lc.miss_case(g, "lanes_0_63").miss_at} == {0, 63} and per_chunk("lanes_0_63")[:6] == [2, 2, 2, 2, 2, 0]
    assert per_chunk("single_pass_only") == [0] * 8 + [64, 0, 0] and passes(600, 0) == (1, 1)
    assert per_chunk("wave3_only")[:8] == [0, 0, 0, 32, 0, 0, 0, 32] and passes(512, 3) == (1, 0)
    assert len(lc.miss_case(g, "queued_64").miss_at) == lc.ALL_WAVES_AT and len(lc.miss_case(g, "queued_65").miss_at) == lc.ALL_WAVES_AT + 1
    # nothing splits into more: a miss has at least 2 bytes... and a piece of 2 bytes (a blank and a letter) is a table entry
    assert len(lc.miss_case(g, "most_of_3").miss_at) == (lc.T - 2) // 3 and len(lc.miss_case(g, "most_of_4").miss_at) == lc.T // 4
