"""CPU tier: the texts of pack_stage_cases.py hold what they set out to hold -- hard pieces per bin at the staged heads' caps, at
the end of the free room and beyond, token totals at the stage's edge -- by the oracle's own split and merges of the finished
text, alone and as the second chunk of a two-chunk job.  tests/test_pack_stage_gpu.py relies on this."""
import numpy as np
import pytest

import pack_stage_cases as psc


@pytest.fixture(scope="module")
def words():
    return psc.Words()


def test_every_case_reaches_its_counts(words):
    cs = psc.cases(words)
    assert set(cs) == {"cap", "room", "worst", "stage", "free", "counts", "docs"}
    for label, (case, want) in cs.items():
        assert 1 <= len(case.tiles) <= 4                      # 3..6 tiles with the filler tile before and the partial one after
        plain = psc.check_targets(words, case, want, 0)
        second = psc.check_targets(words, case, want, psc.SECOND_BASE)
        # the second-chunk form: one document up to SECOND_BASE, which is past the chunk size and not on a tile edge
        assert second[1][1] == psc.SECOND_BASE > psc.CHUNK and psc.SECOND_BASE % psc.T != 0
        assert len(second[0]) < 2 * psc.CHUNK
        assert plain[1][-1] == len(plain[0])


def test_pieces_of_every_kind(words):
    """The pools: hard pieces of each length class become two or more tokens, the ones with a stated count have it, and the
    fillers are single tokens of every length from 2 bytes."""
    for length, lo, hi in ((3, 2, 99), (4, 2, 2), (10, 2, 5), (14, 2, 7), (14, 7, 7), (16, 8, 99), (24, 2, 99)):
        for p in words.hard(length, 6, lo, hi):
            toks = words.o.merge_piece(p)
            assert len(p) == length and lo <= len(toks) <= hi and len(toks) >= 2
            assert words.o.encode_ordinary(p.decode()) == toks
    assert all(len(words.o.merge_piece(words.fill[k])) == 1 for k in range(2, words.max_fill + 1))


def test_documents_start_where_the_docs_case_says(words):
    case, _ = psc.cases(words)["docs"]
    text, doc_off = case.batch(0)
    raw = text.tobytes()
    t0 = case.first_tile(0) * psc.T
    starts = [int(d) for d in doc_off if t0 <= d < t0 + psc.T]
    hard = sum(words.count(p) >= 2 for p in case.tiles[0])
    assert len(starts) == hard == 32 + psc.room_for(640) + 6   # more than head and extension hold: some start after the room's end
    assert all(words.count(raw[s:s + 4]) == 2 for s in starts)
    assert np.all(np.diff(doc_off) > 0)
