"""What merge_exit_cases.py holds, asserted on the CPU, so that no case of test_merge_exit_gpu.py can silently stop exercising the
early exit of lean_steps: the replay of want1 / want2 agrees with merge_ref.py on every piece, every wave is what its label says
by that replay, the lane rule the exit rests on holds for every piece of this plan and of merge_cases, and the texts queue the
planned numbers of entries in the planned shards by the oracle's own split."""
import pytest

import merge_cases as mc
import merge_exit_cases as mx
import merge_ref

_cache = {}


@pytest.fixture(scope="module")
def plan():
    if "plan" not in _cache:
        _cache["plan"] = mx.Plan()
    return _cache["plan"]


def _pieces(plan):
    return sorted({p for s in mx.SLOTS for v in plan.waves[s] for p in v.pieces})


def test_replay_is_the_plain_merge(plan):
    """same tokens and as many steps as merge_ref, and as the oracle; a piece of up to 16 bytes is no table entry"""
    for p in _pieces(plan):
        steps, tokens = plan.steps(p)
        ref_tokens, trace = merge_ref.merge_ref(p, plan.ranks)
        assert tokens == ref_tokens == plan.P.tokens(p) and len(steps) == len(trace) == len(p) - len(tokens), p
        assert len(p) > 16 or p not in plan.ranks
        # what the replay calls the sides is what the trace calls a part after next and a part before
        for k, (w1, w2) in enumerate(steps):
            assert (not w1 or trace.ahead[k] > 0) and (not w2 or trace.prev_len[k] > 0), (p, k)


def test_lane_rule(plan):
    """a step that is `act` and wants nothing is the piece's last step -- for both values of SKIP_WHOLE, over every piece of this
    plan and every piece of merge_cases' plan that runs through lean_steps"""
    other = [e.piece for e in mc.Plan().everything if 4 <= e.length <= 64 and (e.length > 16 or e.piece not in plan.ranks)]
    assert len(other) > 100
    n_quiet = 0
    for p in _pieces(plan) + other:
        steps, tokens = mx.replay(p, plan.ranks, mx.SKIP_WHOLE[mx.slots_of(len(p))])
        for k, wants in enumerate(steps):
            if wants == (False, False):
                assert k == len(steps) - 1, (p, k, len(steps))
                n_quiet += 1
        # and which pieces end so: two parts left in the bins of up to 16 bytes, one in the others
        if steps:
            assert mx.ends_quietly(steps) == (len(tokens) == (2 if len(p) <= 16 else 1)), p
    assert n_quiet > 50


@pytest.mark.parametrize("slots", mx.SLOTS)
def test_waves_are_what_their_labels_say(plan, slots):
    skip = mx.SKIP_WHOLE[slots]
    L = mx.A_LEN[slots]
    S = L - 2 if skip else L - 1
    labels = [v.label for v in plan.waves[slots]]
    want = ["a"] + ["b.%s.%s" % (s, p) for s in mx.SIDES for p in mx.PLACES] + ["c", "d"] + ([] if skip else ["e"]) + ["f"]
    assert labels == want
    prof = lambda v: [plan.steps(p)[0] for p in v.pieces]
    # a: 64 pieces, all with their last merge in step S, which wants nothing: the exit is taken in step S
    a = plan.wave(slots, "a")
    assert len(a.pieces) == 64 and len(set(a.pieces)) >= 4
    assert all(len(st) == S and mx.ends_quietly(st) for st in prof(a)) and plan.exit_step(a) == (S, True)
    # b: one lane still wants a lookup in step S -- side 1 only, side 2 only, both -- first, in the middle and last
    for side, wants in mx.SIDES.items():
        for place, at in mx.PLACES.items():
            b = plan.wave(slots, "b.%s.%s" % (side, place))
            assert len(b.pieces) == 64 and [i for i in range(64) if b.pieces[i] != a.pieces[i]] == [at]
            st = plan.steps(b.pieces[at])[0]
            assert len(st) >= S and st[S - 1] == wants
            n, quiet = plan.exit_step(b)
            assert n > S or (n == S and not quiet)
    # c: one lane runs two or more steps further and ends quietly: the exit is taken there
    c = plan.wave(slots, "c")
    diff = [i for i in range(64) if c.pieces[i] != a.pieces[i]]
    assert diff == [mx.PLACES["middle"]]
    st = plan.steps(c.pieces[diff[0]])[0]
    assert len(st) >= S + 2 and mx.ends_quietly(st) and plan.exit_step(c) == (len(st), True)
    # d: every piece ends with three or more parts, so the wave's last step wants a lookup
    d = plan.wave(slots, "d")
    assert len(d.pieces) == 64 and len(set(d.pieces)) == 64
    assert all(len(plan.steps(p)[1]) >= 3 and not mx.ends_quietly(plan.steps(p)[0]) for p in d.pieces)
    assert plan.exit_step(d)[1] is False
    # e: table entries of the bin's lengths that merge down to one token, among pieces that do not
    if not skip:
        e = plan.wave(slots, "e")
        ent = [p for p in e.pieces if p in plan.ranks]
        assert len(set(ent)) >= 4 and all(plan.steps(p)[1] == [plan.ranks[p]] and mx.ends_quietly(plan.steps(p)[0]) for p in ent)
        assert any(p not in plan.ranks for p in e.pieces) and len(e.pieces) == 64
        # (waves a, c and f of these bins are entries too)
        assert all(p in plan.ranks for p in a.pieces)
    # f: fewer than 64 entries
    f = plan.wave(slots, "f")
    assert f.pieces == a.pieces[:mx.PARTIAL] and plan.exit_step(f) == (S, True)


@pytest.mark.parametrize("slots", mx.SLOTS)
def test_texts_queue_what_they_plan(plan, slots):
    """by the oracle's split of the finished tiles: small() one wave per shard and every bin within one workgroup pass; large()
    more than three passes' worth in one shard, in whole waves"""
    t = plan.small(slots)
    n = mx.queue_counts(plan.P, t)
    waves = plan.waves[slots]
    assert n == {(slots, s): len(v.pieces) for s, v in enumerate(waves)}
    assert len(t.text) <= 2 * 64 * mx.T and len(t.doc_off) - 1 == len(t.text) // mx.T
    t = plan.large(slots)
    n = mx.queue_counts(plan.P, t)
    assert list(n) == [(slots, 3)] and n[(slots, 3)] % 64 == 0
    assert (mx.WGS_PER_SHARD - 1) * mx.LANES[slots] < n[(slots, 3)] <= (mx.WGS_PER_SHARD - 1) * mx.LANES[slots] + 64
    assert len(t.text) < 4 << 20


@pytest.mark.parametrize("R", [2, 4])
def test_windows(plan, R):
    """exactly R x 4096 entries of the 4..8-byte bin in one shard, 64 R per tile; sorted by length (stably) a tile's rounds are
    waves of the kinds a, b and c"""
    t = plan.windows(R)
    assert mx.queue_counts(plan.P, t) == {(8, 5): R * mx.SPAN}
    assert len(t.by_shard[5]) == mx.SPAN // 64 and len(t.text) == mx.SPAN // 64 * 64 * mx.T
    seen = set()
    for kind in t.window_kinds:
        assert len(kind) == 64 * R
        order = sorted(kind, key=len)                              # (stable, as jtk_merge_order_rules.h orders a window)
        for r in range(1, R):
            # a round's edge falls between two length classes, so the order inside the tile cannot move a piece to another
            # round (the 128 eight-byte pieces of kind d fill two rounds: any 64 of them are a wave of kind d)
            assert len(order[64 * r - 1]) != len(order[64 * r]) or len(order[64 * r]) == 8
        for r in range(R):
            pieces = order[64 * r:64 * r + 64]
            lengths = sorted(set(len(p) for p in pieces))
            n, quiet = plan.exit_step(mx.Wave(8, "round", pieces))
            prof = [plan.steps(p)[0] for p in pieces]
            if len(lengths) == 1 and quiet and all(len(st) == n for st in prof):
                seen.add("a")
            elif len(lengths) == 2 and sum(len(p) == lengths[1] for p in pieces) == 1:
                S = lengths[0] - 2
                assert all(len(st) == S and mx.ends_quietly(st) for p, st in zip(pieces, prof) if len(p) == lengths[0])
                st = next(st for p, st in zip(pieces, prof) if len(p) == lengths[1])
                if len(st) >= S + 2 and mx.ends_quietly(st):
                    assert (n, quiet) == (len(st), True)
                    seen.add("c")
                else:
                    assert st[S - 1] == (True, True) and (n > S or not quiet)
                    seen.add("b")
    assert seen == {"a", "b", "c"}
