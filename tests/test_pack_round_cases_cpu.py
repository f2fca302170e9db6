"""CPU tier: the texts of pack_round_cases.py hold what they set out to hold -- pieces per tile at the edges of k_pack_tokens'
steps (64 pieces) and rounds (512), token totals around the LDS assembly's 768, hard pieces of every token count in chosen
lanes of chosen steps, tiny pieces across step edges, document starts at chosen pieces -- by the oracle's own split and
merges of the finished text, alone and as the second chunk of a two-chunk job.  tests/test_pack_rounds_gpu.py relies on this."""
import pytest

import pack_round_cases as prc
import pack_stage_cases as psc

LABELS = {"counts_small_staged", "counts_round_staged", "counts_small_direct", "counts_round_direct", "counts_big", "edge_512",
          "edge_576", "lanes_staged", "lanes_direct", "general", "tiny", "docs"}


@pytest.fixture(scope="module")
def words():
    return psc.Words()


@pytest.fixture(scope="module")
def texts(words):
    return {t.label: t for t in prc.texts(words)}


def test_one_byte_pieces(words):
    """The oracle splits a digit and a letter in turn into one-byte pieces of one token each."""
    raw = b"a1" * 1024
    pieces = words.o.split(raw)
    assert len(pieces) == 2048 and all(len(p) == 1 for p in pieces)
    assert all(words.count(p) == 1 for p in (b"a", b"1", b"."))


def test_pools(words):
    pl = prc.Pools(words)
    for k, pool in pl.kinds.items():
        for p in pool:
            c = words.count(p)
            assert (c == k if k < 8 else c > 7) and words.o.split(p) == [p]
    assert all(len(p) == 3 and words.count(p) >= 2 for p in pl.tiny)            # 3 bytes and not in the table: the tiny queue
    assert all(psc.bin_of(len(p)) == 0 for p in pl.two + pl.three + pl.four) and all(psc.bin_of(len(p)) == 1 for p in pl.mid)


def test_every_text_reaches_its_counts(words, texts):
    assert set(texts) == LABELS
    for txt in texts.values():
        assert 1 <= len(txt.case.tiles) <= 10
        plain = prc.check(words, txt, 0)
        second = prc.check(words, txt, prc.SECOND_BASE)
        assert second[1][1] == prc.SECOND_BASE > prc.CHUNK and prc.SECOND_BASE % prc.T != 0
        assert prc.CHUNK < len(second[0]) < 2 * prc.CHUNK
        assert plain[1][-1] == len(plain[0])


def test_every_piece_count_in_a_staged_and_in_a_direct_tile(texts):
    staged, direct = set(), set()
    for txt in texts.values():
        if txt.label.startswith("counts"):
            for wnt in txt.want:
                (staged if ("le" in wnt or wnt.get("total", 10 ** 6) <= prc.STAGE) else direct).add(wnt["pieces"])
    assert staged == set(prc.COUNTS_SMALL + prc.COUNTS_ROUND)                      # (a tile of more than 768 pieces has more tokens)
    assert direct == set(prc.COUNTS_SMALL + prc.COUNTS_ROUND + prc.COUNTS_BIG)


def test_stage_edge_totals(texts):
    for a in (512, 576):
        got = sorted((w["pieces"], w["total"]) for w in texts["edge_%d" % a].want)
        assert got == [(n, t) for n in (a, a + 1) for t in (767, 768, 769)]


def test_hard_pieces_in_the_lanes(words, texts):
    places = {0, 63, 448, 511, 512, 575}          # lanes 0 and 63 of the first and last step of a round and of step 8
    for label in ("lanes_staged", "lanes_direct"):
        seen = []
        for wnt in texts[label].want:
            c = {wnt["hard"][i] for i in places}
            assert len(c) == 1 or min(c) > 7
            seen.append(min(min(c), 8))
        assert seen == [2, 3, 4, 7, 8]


def test_general_steps(words, texts):
    """In the staged tile the steps 1, 4 and 6 hold one hard piece, of more than 7 tokens, and the steps 2, 3 and 7 beside them
    only pieces of 2 to 4 tokens; the direct tiles hold more tiny pieces and more pieces of 4 to 8 bytes than are staged."""
    staged, direct, bin0 = texts["general"].want
    by_step = {}
    for i, c in staged["hard"].items():
        by_step.setdefault(i // prc.STEP, []).append(c)
    assert sorted(by_step) == [1, 2, 3, 4, 6, 7]
    assert all(len(by_step[s]) == 1 and by_step[s][0] > 7 for s in (1, 4, 6))
    assert all(sorted(by_step[s]) == [2, 2, 3, 4] for s in (2, 3, 7))
    tiny = [i for i in direct["hard"] if len(texts["general"].case.tiles[1][i]) == 3]
    assert len(tiny) == 194 > prc.TINY_STAGED and tiny[-2:] == [3 * 64 + 17, 6 * 64]
    short = [i for i in bin0["hard"] if len(texts["general"].case.tiles[2][i]) <= 8]
    assert len(short) == 240 > psc.CAP[0] + psc.OUT_SLOTS and short[-2:] == [8 * 64 + 9, 10 * 64 + 50]


def test_tiny_pieces_at_step_edges(texts):
    tiles = texts["tiny"].case.tiles
    for k in (0, 1):
        tiny = [i for i, p in enumerate(tiles[k]) if i in texts["tiny"].want[k]["hard"] and len(p) == 3]
        assert tiny == [63, 64, 127, 128, 511, 512, 575, 576]
    many = [i for i, p in enumerate(tiles[2]) if i in texts["tiny"].want[2]["hard"] and len(p) == 3]
    assert len(many) == 142 > prc.TINY_STAGED and many[-2:] == [5 * 64 + 63, 6 * 64]
