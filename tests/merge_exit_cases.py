"""Waves for the early exit of the lean merge steps (lean_steps in jtokkit_amd/csrc/jtk_kernels.hip): a step in which no lane of
the wave wants a pair lookup is finished without its two gathers and leaves the loop.  Built with merge_ref.py, the CPU oracle
and the generators of merge_cases.py over cl100k_base; test_merge_exit_cases_cpu.py asserts what the plan holds and
test_merge_exit_gpu.py runs its texts on the device.

replay() is lean_steps' rule for want1 / want2 in plain Python, on a list of parts: with `i` the chosen part of `n`,
    want1 = there is a part after next                    and not (SKIP_WHOLE and i == 0 and n == 3)
    want2 = there is a part before                        and not (SKIP_WHOLE and i == 1 and n == 3)
(slot 0 never dies, so the kernel's `mini == 0` and `pv == 0` are i == 0 and i == 1).  SKIP_WHOLE holds in the bins of up to 16
bytes (8, 12, 16 slots: the piece is no table entry), not in the 32- and 64-slot bins, whose pieces may be entries.

A wave is a list of up to 64 pieces of one slot count; per slot count the plan holds
    a       64 pieces whose last merge falls in the same step S (counted from 1) and wants nothing: the exit is taken in step S
    b.*     wave a with one piece replaced by one that is still merging in step S and wants side 1 only, side 2 only or both,
            standing first, last or in the middle (nine waves): the exit is not taken in step S
    c       wave a with one piece that ends like the others, two or more steps later: the exit is taken on that piece's last step
    d       64 pieces that end with three or more parts: their last step wants a lookup, and the wave leaves only when the scan
            after it finds no lane merging
    e       (32 and 64 slots) table entries of 17..64 bytes, which merge down to one token, among pieces that do not
    f       37 pieces of wave a: lanes without a piece
In the bins of up to 16 bytes a piece whose last step wants nothing ends with two parts; in the 32- and 64-slot bins it is a
table entry (its last two parts merge into one), so waves a, c and f of those bins are made of table entries.

Texts.  Every tile is one document of exactly 2048 bytes, and tile g feeds the queues of shard g % 64.  Which lane gets which
piece follows the order in which k_piece_resolve's lanes and tiles claimed queue space, so a text fixes what it can: a wave's
pieces stand together at the start of a tile (64-slot waves: of two tiles of one shard, 32 pieces each), in the bins of up to 16
bytes as whole 64-piece chunks of the tile's piece list, which one wave of k_piece_resolve claims with one LDS atomic -- first,
last and middle are positions in that order.  Whatever the order, the 64 entries are the wave's set in small() and windows().
    small(slots)    one wave per shard, every bin of every shard within one workgroup pass: the side-by-side dispatch
    large(slots)    one shard with 3 x (lanes of a workgroup in that bin) + 64 entries of the bin, in whole waves: all four
                    workgroups of the shard take a slice, 64 consecutive entries per wave
    windows(R)      the 4..8-byte bin with exactly R x 4096 entries in one shard (R = 2, 4): one pass of R-round windows.  Each
                    tile holds one window (64 R entries) whose length classes fill whole rounds, so that after the stable order
                    by length the rounds are waves a, b (the odd piece the only one of its length in the window) and c
"""
import random

import numpy as np

import merge_cases as mc
import pack_stage_cases as psc

NAME = "cl100k_base"
T, Q_SHARDS = psc.T, 64
SLOTS = (8, 12, 16, 32, 64)
BYTES = {8: (4, 8), 12: (9, 12), 16: (13, 16), 32: (17, 32), 64: (33, 64)}
SKIP_WHOLE = {8: True, 12: True, 16: True, 32: False, 64: False}
LANES = {8: 1024, 12: 1024, 16: 1024, 32: 512, 64: 256}      # lanes of a workgroup in the bin = entries of one pass
WGS_PER_SHARD = 4
SPAN = WGS_PER_SHARD * 1024                                      # entries of the 4..8-byte bin that a shard takes per round
A_LEN = {8: 5, 12: 9, 16: 13, 32: 17, 64: 33}                    # length of wave a's pieces
SIDES = {"side1": (True, False), "side2": (False, True), "both": (True, True)}
PLACES = {"first": 0, "middle": 29, "last": 63}
PARTIAL = 37


def slots_of(length):
    return next(s for s in SLOTS if BYTES[s][0] <= length <= BYTES[s][1])


def replay(piece, ranks, skip_whole):
    """([(want1, want2) per merge step], token ids) of one piece by lean_steps' rules"""
    parts = [piece[i:i + 1] for i in range(len(piece))]
    rk = [ranks.get(parts[i] + parts[i + 1]) for i in range(len(parts) - 1)]
    steps = []
    while True:
        i = None
        for j, r in enumerate(rk):
            if r is not None and (i is None or r < rk[i]):
                i = j                                              # the first of equal minima
        if i is None:
            break
        n = len(parts)
        has_nn, has_pv = i + 2 < n, i > 0
        want1 = has_nn and not (skip_whole and i == 0 and n == 3)
        want2 = has_pv and not (skip_whole and i == 1 and n == 3)
        steps.append((want1, want2))
        parts[i:i + 2] = [parts[i] + parts[i + 1]]
        del rk[i]
        if has_nn:
            rk[i] = ranks.get(parts[i] + parts[i + 1])
        if has_pv:
            rk[i - 1] = ranks.get(parts[i - 1] + parts[i])
    return steps, [ranks[p] for p in parts]


def ends_quietly(steps):
    """the piece's last step is `act` and wants nothing: the lane alone would take the exit there"""
    return bool(steps) and steps[-1] == (False, False)


class Wave:
    def __init__(self, slots, label, pieces):
        assert 1 <= len(pieces) <= 64 and all(slots_of(len(p)) == slots for p in pieces), (slots, label)
        self.slots, self.label, self.pieces = slots, label, list(pieces)

    def __repr__(self):
        return "wave %s of the %d-slot bin (%d pieces)" % (self.label, self.slots, len(self.pieces))


class Plan:
    """All waves, made once (seeded: the same every run)."""

    def __init__(self, name=NAME):
        self.P = P = mc.Pieces(name)
        self.w = P.w
        self.ranks = P.ranks
        self._steps = {}
        self._long = None
        self.waves = {s: self._waves(s) for s in SLOTS}

    def steps(self, p):
        if p not in self._steps:
            self._steps[p] = replay(p, self.ranks, SKIP_WHOLE[slots_of(len(p))])
        return self._steps[p]

    # ---- pieces -----------------------------------------------------------------------------------------------------------
    def _letters(self, length, rnd):
        """a blank and lowercase letters: one pre-token wherever it stands among its like"""
        kind = rnd.randrange(3)
        if kind == 0:
            return self.P.gen("words", length, rnd)
        if kind == 1:
            return self.P.gen("rare", length, rnd)
        return b" " + "".join(rnd.choice("abcdefghijklmnopqrstuvwxyz") for _ in range(length - 1)).encode()

    def find(self, label, lengths, want, k, tries=60000):
        """k different pieces of those lengths that are no table entries and for which want(steps, tokens) holds"""
        rnd = random.Random("exit/" + label)
        out, seen = [], set()
        for _ in range(tries):
            if len(out) == k:
                return out
            p = self._letters(rnd.choice(lengths), rnd)
            if p in seen or p in self.ranks:
                continue
            seen.add(p)
            steps, tokens = self.steps(p)
            if want(steps, tokens) and self.P.o.split(p) == [p]:
                out.append(p)
        raise AssertionError("%s: %d of %d pieces found" % (label, len(out), k))

    def entries(self, length, k):
        """up to k table entries of that length that stand alone between fillers and merge down to their one token"""
        if self._long is None:
            self._long = {}
            for p in sorted(self.ranks, key=lambda q: self.ranks[q]):
                if 17 <= len(p) <= 64:
                    self._long.setdefault(len(p), []).append(p)
        out = []
        for p in self._long.get(length, ()):
            if self.P.stands_alone(p) and self.steps(p)[1] == [self.ranks[p]]:
                out.append(p)
                if len(out) == k:
                    break
        return out

    # ---- waves ------------------------------------------------------------------------------------------------------------
    def _waves(self, slots):
        lo, hi = BYTES[slots]
        L = A_LEN[slots]
        skip = SKIP_WHOLE[slots]
        tag = "%d/" % slots
        if skip:
            S = L - 2                                              # two parts are left
            quiet = psc.cycle(self.find(tag + "a", [L], lambda st, tk: len(tk) == 2, 64), 64)
            # (8 slots: exactly two bytes longer, and the odd pieces below exactly one, so that windows() can use them)
            later = self.find(tag + "c", [L + 2] if slots == 8 else list(range(L + 2, hi + 1)), lambda st, tk: len(tk) == 2, 1)[0]
        else:
            S = L - 1                                              # one part is left: a table entry
            pool = self.entries(L, 64)
            assert len(pool) >= 4, (slots, len(pool))
            quiet = psc.cycle(pool, 64)
            later = next(e[0] for e in (self.entries(n, 1) for n in range(L + 2, hi + 1)) if e)
        out = [Wave(slots, "a", quiet)]
        for side, wants in SIDES.items():
            odd = self.find(tag + side, [L + 1] if slots == 8 else list(range(L + 1, hi + 1)), lambda st, tk: len(st) >= S and st[S - 1] == wants, 1)[0]
            for place, at in PLACES.items():
                out.append(Wave(slots, "b.%s.%s" % (side, place), quiet[:at] + [odd] + quiet[at + 1:]))
        out.append(Wave(slots, "c", quiet[:PLACES["middle"]] + [later] + quiet[PLACES["middle"] + 1:]))
        many = self.find(tag + "d", list(range(lo, min(hi, lo + 7) + 1)), lambda st, tk: len(tk) >= 3 and len(st) >= 1, 64)
        out.append(Wave(slots, "d", many))
        if not skip:
            found = [e[0] for e in (self.entries(n, 1) for n in range(lo, hi + 1)) if e][:16]
            mixed = [found[i // 4 % len(found)] if i % 4 == 1 else many[i] for i in range(64)]
            out.append(Wave(slots, "e", mixed))
        out.append(Wave(slots, "f", quiet[:PARTIAL]))
        return out

    def wave(self, slots, label):
        return next(v for v in self.waves[slots] if v.label == label)

    def exit_step(self, wave):
        """(steps the wave runs, whether its last step is one that no lane wants a lookup in) by the replay"""
        prof = [self.steps(p)[0] for p in wave.pieces]
        n = max(len(st) for st in prof)
        return n, n > 0 and not any(len(st) >= n and (st[n - 1][0] or st[n - 1][1]) for st in prof)

    # ---- texts ------------------------------------------------------------------------------------------------------------
    def _tile(self, pieces, spaced):
        """one tile: the pieces (each followed by a four-byte filler if `spaced`), then fillers to 2048 bytes"""
        parts = []
        for p in pieces:
            parts.append(p)
            if spaced:
                parts.append(self.w.fill[4])
        used = sum(len(p) for p in parts)
        rest = T - used
        assert rest >= 0, (used, len(pieces))
        if rest == 1:                                              # (no one-byte filler: the last filler grows by one)
            assert spaced and parts[-1] == self.w.fill[4]
            parts[-1] = self.w.fill[5]
            rest = 0
        parts += self.w.fillers(rest, (rest + 9) // 10)
        return b"".join(parts)

    def per_tile(self, slots):
        """waves of that slot count in one tile"""
        return {8: 4, 12: 2, 16: 2, 32: 1, 64: 0.5}[slots]

    def _tiles_of(self, slots, waves):
        """the tiles (in order, all of one shard) that hold these waves"""
        spaced = not SKIP_WHOLE[slots]
        if slots == 64:
            return [self._tile(v.pieces[h:h + 32], spaced) for v in waves for h in (0, 32) if v.pieces[h:h + 32]]
        n = int(self.per_tile(slots))
        return [self._tile([p for v in waves[i:i + n] for p in v.pieces], spaced) for i in range(0, len(waves), n)]

    def _text(self, label, by_shard):
        """by_shard: shard -> its tiles, top down; every other tile is one of fillers"""
        filler = self._tile([], False)
        rows = max(len(v) for v in by_shard.values())
        parts = [by_shard[g % Q_SHARDS][g // Q_SHARDS] if g % Q_SHARDS in by_shard and g // Q_SHARDS < len(by_shard[g % Q_SHARDS])
                 else filler for g in range(rows * Q_SHARDS)]
        assert all(len(p) == T for p in parts)
        text = np.frombuffer(b"".join(parts), dtype=np.uint8).copy()
        return ExitText(label, text, np.arange(len(parts) + 1, dtype=np.int64) * T, by_shard)

    def small(self, slots):
        waves = self.waves[slots]
        assert len(waves) <= Q_SHARDS
        # (wave f, the partial one, has a shard of its own like every other: its lanes 37..63 have no piece)
        return self._text("small/%d" % slots, {s: self._tiles_of(slots, [v]) for s, v in enumerate(waves)})

    def large(self, slots, shard=3):
        full = [v for v in self.waves[slots] if len(v.pieces) == 64]
        n = WGS_PER_SHARD - 1
        n = n * LANES[slots] // 64 + 1                             # whole waves: 3 passes' worth and one more
        return self._text("large/%d" % slots, {shard: self._tiles_of(slots, psc.cycle(full, n))})

    def windows(self, R, shard=5):
        """tiles of 64 R entries of the 4..8-byte bin, R x 4096 entries in all; see the module text"""
        a5, odd, later = self.wave(8, "a").pieces, self.wave(8, "b.both.middle").pieces[PLACES["middle"]], self.wave(8, "c").pieces[PLACES["middle"]]
        assert len(a5[0]) == 5 and len(odd) == 6 and len(later) == 7, (len(odd), len(later))
        a4 = psc.cycle(self.find("win/4", [4], lambda st, tk: len(tk) == 2, 48), 64)
        a6 = psc.cycle(self.find("win/6", [6], lambda st, tk: len(tk) == 2, 48), 64)
        a7 = psc.cycle(self.find("win/7", [7], lambda st, tk: len(tk) == 2, 48), 64)
        d8 = psc.cycle(self.find("win/8", [8], lambda st, tk: len(tk) >= 3, 48), 128)
        if R == 4:
            kinds = [a4 + a5 + a6 + a7,                            # rounds: a (S = 2), a (3), a (4), a (5)
                     a4 + a5[:63] + [odd] + d8,                    # a, b, d, d
                     a4 + a5[:63] + [later] + d8]                  # a, c, d, d
        else:
            assert R == 2
            kinds = [a5 + a7, a5[:63] + [odd] + d8[:64], a5[:63] + [later] + d8[:64]]
        rnd = random.Random("windows/%d" % R)
        tiles = []
        for k in range(R * SPAN // (64 * R)):
            pieces = list(kinds[k % 3])
            rnd.shuffle(pieces)                                    # (the order inside a window is the kernel's to undo)
            tiles.append(self._tile(pieces, False))
        t = self._text("windows/R%d" % R, {shard: tiles})
        t.window_kinds = kinds
        return t


class ExitText:
    def __init__(self, label, text, doc_off, by_shard):
        self.label, self.text, self.doc_off, self.by_shard = label, text, doc_off, by_shard

    def where(self, doc):
        s = doc % Q_SHARDS
        return "%s: tile %d (shard %d, row %d%s)" % (self.label, doc, s, doc // Q_SHARDS, "" if s in self.by_shard else ", fillers")


def queue_counts(P, t):
    """entries per (slot count, shard) that the text queues: the oracle's split, pieces of 4..64 bytes that are not resolved as
    one table lookup (up to 16 bytes: no table entry; longer: all)"""
    n = {}
    raw = t.text.tobytes()
    for d in range(len(t.doc_off) - 1):
        if d % Q_SHARDS not in t.by_shard:
            continue
        for p in P.o.split(raw[int(t.doc_off[d]):int(t.doc_off[d + 1])]):
            if 4 <= len(p) <= 64 and (len(p) > 16 or p not in P.ranks):
                key = (slots_of(len(p)), d % Q_SHARDS)
                n[key] = n.get(key, 0) + 1
    return n
