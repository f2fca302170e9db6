"""What test_merge_entry16_gpu.py says of its texts (merge_entry16_cases.py), asserted with the oracle alone (no GPU)."""
import numpy as np

import merge_entry16_cases as mc

NAME = "cl100k_base"


def test_every_length_of_the_bin_is_there():
    P = mc.pieces(NAME)
    for n in range(4, 9):
        assert len(P.pool[n]) == mc.POOL and len(set(P.pool[n])) == mc.POOL
        for p in P.pool[n]:
            assert len(p) == n and len(P.o.merge_piece(p)) >= 2 and P.o.split(p) == [p]
    two = mc.two_byte_tokens(NAME)
    for p in P.nomerge:
        assert len(p) == 8 and not any(p[i:i + 2] in two for i in range(7)) and len(P.o.merge_piece(p)) == 8


def test_patterns_reach_every_number_of_slots():
    """the longest piece of a round of a window, by the order rule: rounds within 5 slots, within 6 and beyond, and the class edges"""
    tops = {}
    for pattern in ("all4", "all5", "all8", "ascending", "four_five", "five_six", "one_seven", "mixed", "short", "eights"):
        for R in (2, 4):
            lens = sorted(mc.length(pattern, i) for i in range(64 * R))
            tops[(pattern, R)] = [lens[64 * r + 63] for r in range(R)]
    assert tops[("all4", 4)] == [4] * 4 and tops[("all5", 2)] == [5] * 2 and tops[("all8", 2)] == [8] * 2
    assert tops[("ascending", 4)] == [5, 6, 7, 8] and tops[("four_five", 4)] == [4, 4, 5, 5] and tops[("five_six", 2)] == [5, 6]
    assert tops[("one_seven", 2)] == [5, 7]
    assert set(sum(tops.values(), [])) == {4, 5, 6, 7, 8}


def test_shard_counts():
    spec = mc.MAIN_SPEC
    counts = sorted(n for n, _ in spec.values())
    assert counts[:5] == [1, 63, 64, 65, 65] and len(spec) < mc.Q_SHARDS            # (some shards hold no entry at all)
    for n in (mc.S2 - 1, mc.S2, mc.S2 + 1, mc.S2 + 63, mc.S4 + 1, mc.S4 + 63):
        assert n in counts
    assert mc.rounds(mc.S2 - 1) == 1 and mc.rounds(mc.S2) == 2 and mc.rounds(mc.S4) == 4
    t = mc.Shards(NAME, spec, mc.tiles_needed(spec))                                 # (asserts its own layout against the oracle's split)
    assert t.count == {s: n for s, (n, _) in spec.items()}
    assert len(t.text) <= 7 << 20


def test_dense_text_and_its_chunks():
    d = mc.dense(NAME)
    (lead, per), = d.per_shard()
    assert lead == 0 and per.min() >= mc.WINDOWS_FROM
    b = mc.below(d)
    (_, per_b), = b.per_shard()
    assert mc.WINDOWS_FROM - 400 < per_b.max() < mc.WINDOWS_FROM
    small = d.per_shard(1 << 20)
    assert len(small) >= 4 and all(lead != 0 for lead, _ in small[1:]) and all(per.max() < mc.WINDOWS_FROM for _, per in small)
    big = d.per_shard(mc.WINDOW_CHUNK)
    assert len(big) == 2 and big[1][0] != 0 and all(per.max() >= mc.WINDOWS_FROM for _, per in big)
    # pieces that merge nothing in every chunk
    starts = set(d.starts.tolist())
    raw = d.text.tobytes()
    hits = [i for i in d.starts.tolist() if raw[i:i + 8] in d.P.nomerge]
    for first, last in zip(d.chunks(1 << 20), d.chunks(1 << 20)[1:] + [len(d.doc_off) - 1]):
        assert any(d.doc_off[first] <= i < d.doc_off[last] for i in hits)


def test_placed_pieces():
    p = mc.Placed(NAME)                                                              # (asserts the pieces' places against the oracle's split)
    T = mc.T
    assert any(s % T == 0 for s in p.STARTS) and any((s + 8) % T == 0 for s in p.STARTS)
    assert sum(1 for s in p.STARTS if s // T != (s + 7) // T) >= 3 and int(p.doc_off[2]) in p.STARTS
