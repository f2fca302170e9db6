"""The queue bounds of jtk_scratch_rules.h against a brute-force count (no GPU): for every bin, text that the oracle splits into
that bin's hard pieces, counted per tile and per queue shard with the header's own binning function, never exceeds the bound --
and text made of the bin's shortest piece back to back meets it to within the one entry a tile edge can cost."""
import pytest

import scratch_cases as sc

SIZES = (1, 2, 3)                                   # tiles
R = None


def r():
    global R
    if R is None:
        R = sc.rules(sc.GIB, *(t * 2048 for t in SIZES), *(t * 2048 + 1 for t in SIZES))
    return R


def check(text, exact_bin=None):
    rr = r()
    T, S = rr["tile"], rr["shards"]
    n_tiles = (len(text) + 1 + T - 1) // T
    tps = (n_tiles + S - 1) // S
    q = sc.queued(rr, text)
    assert q, "the text queues nothing"
    per_shard = {}
    for (b, tile), n in q.items():
        assert n <= rr["tile_cap"][b], (b, tile, n)
        assert n <= rr["lds_cap"][b], (b, tile, n)
        per_shard[(b, tile % S)] = per_shard.get((b, tile % S), 0) + n
    for (b, shard), n in per_shard.items():
        assert n <= tps * rr["tile_cap"][b], (b, shard, n)
    if exact_bin is not None:
        whole = len(text) // T                      # tiles that the text covers to their last byte
        for tile in range(whole):
            assert rr["tile_cap"][exact_bin] - q.get((exact_bin, tile), 0) <= 1, (exact_bin, tile, q.get((exact_bin, tile), 0))
        assert q.get((exact_bin, 0), 0) == rr["tile_cap"][exact_bin] or text[:1] == b"\n"
    return q


def test_header_constants():
    rr = r()
    assert rr["sets_default_device"] == 3 and rr["sets_default"] == 2 and rr["sets_max"] == 4
    assert rr["min_len"] == [4, 9, 13, 17, 33, 65, 129, 2]
    assert rr["tile_cap"] == [-(-rr["tile"] // m) for m in rr["min_len"]]
    assert all(l >= c for l, c in zip(rr["lds_cap"], rr["tile_cap"]))
    z = rr["sizes"][str(sc.GIB)]
    assert z["shard_cap"] == [(-(-z["n_tiles"] // rr["shards"])) * c for c in rr["tile_cap"]]
    assert z["queues"] == sum(c * rr["shards"] * (8 if b == rr["tiny"] else 24) for b, c in enumerate(z["shard_cap"]))
    # three sets of the new size against two of the old one (every bin at its LDS figure): what the third set costs
    old_queues = (-(-z["n_tiles"] // rr["shards"])) * rr["shards"] * (sum(rr["lds_cap"][:7]) * 24 + rr["lds_cap"][7] * 8)
    assert z["total"] < z["total"] - z["queues"] + old_queues
    assert 29.0 < z["total"] / sc.GIB < 30.0


@pytest.mark.parametrize("b", range(8))
@pytest.mark.parametrize("tiles", SIZES)
def test_shortest_piece_back_to_back_meets_the_bound(b, tiles):
    lo, _ = sc.bin_lengths(r(), b)
    p = sc.hard_piece(lo)
    check(sc.back_to_back(p, tiles * 2048), exact_bin=b)
    check(sc.back_to_back(p, tiles * 2048, shift=1), exact_bin=b)      # a piece straddles every tile edge one byte later


@pytest.mark.parametrize("b", range(8))
@pytest.mark.parametrize("tiles", SIZES)
def test_longest_piece_stays_below(b, tiles):
    _, hi = sc.bin_lengths(r(), b)
    p = sc.hard_piece(hi)
    for shift in (0, 1):
        q = check(sc.back_to_back(p, tiles * 2048, shift=shift))
        assert set(k[0] for k in q) == {b}


@pytest.mark.parametrize("b", [7, 0, 1, 2, 3, 4, 5])
@pytest.mark.parametrize("tiles", SIZES)
def test_two_adjacent_bins_at_once(b, tiles):
    """the shortest pieces of a bin and of the next longer one, alternating: as many of both as their lengths allow"""
    nxt = 0 if b == 7 else b + 1
    pa, pb = sc.hard_piece(sc.bin_lengths(r(), b)[0]), sc.hard_piece(sc.bin_lengths(r(), nxt)[0])
    for shift in (0, 1):
        q = check(sc.back_to_back(pa + pb, tiles * 2048, shift=shift))
        assert set(k[0] for k in q) == {b, nxt}
