"""Small texts for k_piece_resolve's chunk passes (jtokkit_amd/csrc/jtk_kernels.hip): tiles with a chosen number of pieces, pieces
of chosen lengths at chosen places of a tile's piece list, and chosen numbers of queued pieces per bin -- built and counted with
the CPU oracle alone.  test_resolve_cases_cpu.py asserts the counts; test_resolve_passes_gpu.py runs the texts on the device.

The kernel takes a tile's pieces in chunks of 64 (chunk c: pieces 64 c .. 64 c + 63).  With RES_WAVES = 4 waves, wave v takes
chunks v, v + 4, ...: two at a time (a pair pass) while (c + 4) * 64 < np, then at most one alone (a single pass).

The texts are ASCII.  A piece is a blank and lowercase letters (so every blank starts a piece, whatever stands around it), or,
for the fullest tile, a single digit or letter.  Every adjacent byte pair inside a piece occurs in some table entry: pretok_split
cuts a piece where two bytes never stand together in the table, and with none of those cuts the device's piece list of a tile is
the oracle's split.  pieces_per_tile() recounts that from the oracle's split of the finished text.
"""
import random

import numpy as np

import merge_ref
import pack_stage_cases as psc

NAME = "cl100k_base"
T = 2048                                  # JTK_TILE
RES_WAVES = 4                             # JTK_RES_WAVES
BIN_MAXLEN = 256                          # JTK_BIN_MAXLEN
PACK_CAP = (32, 16, 16, 8, 8, 8, 8, 128)  # JTK_PACK_CAP(0..6), JTK_PACK_TINY: results of a tile that pack stages, per bin
TINY = 7                                  # index of the tiny bin here (pack_stage_cases.bin_of)
BIN_LEN = (4, 10, 14, 24, 40, 70, 130, 3)  # a length of each bin
NP_EDGES = (1, 63, 64, 65, 255, 256, 257, 320, 321, 384, 385, 448, 449, 511, 512, 513, 768, 769, 1023, 1024)
NP_MOST = T                               # a digit and a letter in turn: every byte is a piece
EDGE_LENGTHS = (8, 9, 16, 17)
EDGE_NP = 600                             # wave 0: a pair pass over chunks 0 and 4, then chunk 8 alone
EDGE_AT = (0, 63, 256, 319, 512, 575)     # lanes 0 and 63 of those three chunks
_LETTERS = b"abcdefghijklmnopqrstuvwxyz"


class Gen:
    """Pieces by length, found with the oracle and the rank table (seeded: the same every run)."""

    def __init__(self, name=NAME):
        self.name = name
        self.w = psc.Words(name)
        self.o = self.w.o
        self.ranks = merge_ref.load_ranks(name)
        self.pairs = set()
        for k in self.ranks:
            for i in range(len(k) - 1):
                self.pairs.add(k[i:i + 2])
        self.first = [c for c in _LETTERS if bytes([32, c]) in self.pairs]
        self.after = {a: [c for c in _LETTERS if bytes([a, c]) in self.pairs] for a in _LETTERS}
        assert len(self.first) >= 20 and all(len(v) >= 10 for v in self.after.values())
        self._entries = {}

    def pairs_ok(self, piece):
        return all(piece[i:i + 2] in self.pairs for i in range(len(piece) - 1))

    def word(self, length, rnd):
        """a blank and length - 1 letters, every adjacent pair from the table"""
        out = [32, rnd.choice(self.first)] if length >= 2 else [32]
        while len(out) < length:
            out.append(rnd.choice(self.after[out[-1]]))
        return bytes(out[:length])

    def hard(self, length, rnd):
        """... that is no table entry (length >= 3: a blank and one letter always is one)"""
        assert length >= 3
        for _ in range(10000):
            p = self.word(length, rnd)
            if length > 40 or self.w.count(p) >= 2:
                return p
        raise AssertionError(length)

    def entry(self, length, k=0):
        """the k-th table entry of that length that is a blank and lowercase letters"""
        if length not in self._entries:
            self._entries[length] = sorted(p for p in self.ranks if len(p) == length and p[:1] == b" " and p[1:].isalpha()
                                           and p[1:].islower() and p[1:].isascii() and self.o.split(p) == [p])
        found = self._entries[length]
        assert found, "no table entry of %d bytes that is a blank and letters" % length
        return found[k % len(found)]

    def some(self, length, i, rnd):
        """an ordinary piece: table entries and others in turn"""
        if length == 2 or (i % 3 and length in self.w.fill):
            return self.w.fill[length] if length in self.w.fill else self.word(length, rnd)
        return self.word(length, rnd)

    def tile(self, n_pieces, total, rnd, fixed=None):
        """n_pieces pieces of `total` bytes together, lengths as even as they come, the longest last; fixed: {index: piece}"""
        fixed = fixed or {}
        if n_pieces * 2 > total:
            assert n_pieces == total and not fixed
            return [b"1a"[i & 1:(i & 1) + 1] for i in range(total)]
        rest, k = total - sum(len(p) for p in fixed.values()), n_pieces - len(fixed)
        base, rem = divmod(rest, k)
        assert base >= 2, (n_pieces, total)
        lengths = [base] * (k - rem) + [base + 1] * rem
        head = lengths[:-1]
        rnd.shuffle(head)
        lengths = head + lengths[-1:]
        out, j = [], 0
        for i in range(n_pieces):
            if i in fixed:
                out.append(fixed[i])
            else:
                out.append(self.some(lengths[j], i, rnd))
                j += 1
        assert len(out) == n_pieces and sum(len(p) for p in out) == total
        return out

    def fillers(self, n_bytes):
        return self.w.fillers(n_bytes, (n_bytes + 7) // 8)


class Case:
    def __init__(self, label, parts, want, docs=None):
        """parts: the pieces in text order; want: {tile: pieces that start in it}"""
        self.label, self.want = label, want
        self.text = np.frombuffer(b"".join(parts), dtype=np.uint8).copy()
        self.doc_off = np.array(sorted(set([0, len(self.text)] + list(docs or []))), dtype=np.int64)
        self.parts = parts


def pieces_per_tile(g, text, doc_off):
    """pieces that start in each tile, from the oracle's split; every piece is checked for its byte pairs"""
    n = np.zeros((len(text) + T - 1) // T, dtype=np.int64)
    raw = text.tobytes()
    for d in range(len(doc_off) - 1):
        pos = int(doc_off[d])
        for p in g.o.split(raw[pos:int(doc_off[d + 1])]):
            assert g.pairs_ok(p), p[:40]
            n[pos // T] += 1
            pos += len(p)
    return n


def queued_per_tile(g, text, doc_off):
    """pieces of two or more tokens that start in each tile, by bin (index 7: tiny); pieces past BIN_MAXLEN are not counted"""
    n = np.zeros(((len(text) + T - 1) // T, 8), dtype=np.int64)
    raw = text.tobytes()
    for d in range(len(doc_off) - 1):
        pos = int(doc_off[d])
        for p in g.o.split(raw[pos:int(doc_off[d + 1])]):
            if len(p) <= BIN_MAXLEN and g.w.count(p) >= 2:
                n[pos // T, psc.bin_of(len(p))] += 1
            pos += len(p)
    return n


def np_counts():
    return NP_EDGES + (NP_MOST,)


def one_tile(g, n_pieces):
    """A text of one tile with that many pieces: T bytes for an even count, one fewer for an odd one (the end of the text lies
    inside the tile)."""
    rnd = random.Random("one_tile%d" % n_pieces)
    total = T if n_pieces % 2 == 0 else T - 1
    return Case("one_tile/%d" % n_pieces, g.tile(n_pieces, total, rnd), {0: n_pieces})


def middle_tiles(g):
    """Every count in the middle tile of three -- fillers, the tile, fillers -- in one text.  The tile's last piece ends one byte
    into the next tile (not for the fullest tile: its pieces are single bytes).  Then a tile that lies inside one long piece."""
    parts, want, pos = [], {}, 0
    for n_pieces in np_counts():
        rnd = random.Random("middle%d" % n_pieces)
        over = 0 if n_pieces == NP_MOST else 1
        parts += g.fillers(T)
        want[pos // T + 1] = n_pieces
        parts += g.tile(n_pieces, T + over, rnd)
        parts += g.fillers(T - over)
        pos += 3 * T
    rnd = random.Random("inside")
    parts += g.fillers(T - 50) + [g.word(50 + T + 100, rnd)] + g.fillers(T - 100)
    want[pos // T + 1] = 0
    return Case("middle_tiles", parts, want)


def length_edges(g):
    """One tile of EDGE_NP pieces per (length, table entry or not): the piece at EDGE_AT, short ordinary pieces around it."""
    parts, want, what = [], {}, []
    for length in EDGE_LENGTHS:
        for is_entry in (True, False):
            rnd = random.Random("edge%d%d" % (length, is_entry))
            fixed = {at: (g.entry(length, j) if is_entry else g.hard(length, rnd)) for j, at in enumerate(EDGE_AT)}
            want[len(what)] = EDGE_NP
            what.append((length, is_entry, list(fixed.values())))
            parts += g.tile(EDGE_NP, T, rnd, fixed)
    c = Case("length_edges", parts, want)
    c.what = what
    return c


def bin_edges(g):
    """Per bin, three tiles with one fewer queued piece than pack stages of that bin, as many, and one more, among fillers."""
    parts, want_q = [], {}
    for b in range(8):
        for d in (-1, 0, 1):
            rnd = random.Random("bin%d%d" % (b, d))
            pool = [g.hard(BIN_LEN[b], rnd) for _ in range(12)]
            want_q[len(parts)] = (b, PACK_CAP[b] + d)
            parts.append(psc.tile(g.w, psc.cycle(pool, PACK_CAP[b] + d)))
    c = Case("bin_edges", [p for tl in parts for p in tl], {})
    c.want_q = want_q
    return c


def rare_chunk(g):
    """One tile: a chunk of 64 ordinary pieces, then a chunk that holds ordinary pieces, a piece of 300 bytes, one of 600 and, as
    the tile's last, one of 9,000; fillers after it.  `gap` is the index (in the split) of an ordinary piece of the second chunk,
    for a caller's pattern to leave out."""
    rnd = random.Random("rare")
    first = g.tile(64, 64 * 12, rnd)
    second = g.tile(20, 200, rnd) + [g.word(300, rnd)] + g.tile(10, 60, rnd) + [g.word(600, rnd)] + g.tile(8, 48, rnd)
    used = sum(len(p) for p in first + second)
    assert used < T - 40
    tail = g.fillers(T - 40 - used)
    giant = g.word(9000, rnd)
    end = used + len(b"".join(tail)) + 9000
    parts = first + second + tail + [giant] + g.fillers((-end) % T + T)
    c = Case("rare_chunk", parts, {0: len(first + second + tail) + 1})
    c.gap = 64 + 5
    c.second_chunk = (64, 64 + len(second))
    return c


# ---- the <= 8-byte table's secondary slots, from the builder's own hashes ---------------------------------------------------------

def _mix(piece):
    k = [int.from_bytes(piece[i:i + 4].ljust(4, b"\0"), "little") for i in (0, 4, 8, 12)]
    M = 0xFFFFFFFF
    h = (k[0] * 0x9E3779B1 + k[1] * 0x85EBCA77 + k[2] * 0xC2B2AE3D + (k[3] ^ ((len(piece) << 27) & M)) * 0x27D4EB2F) & M
    h ^= h >> 16
    h = (h * 0x2C1B3C6D) & M
    h ^= h >> 13
    return h


def _mix_many(k0, k1, length):
    """_mix for arrays of pieces of one length <= 8: k0, k1 = bytes 0..3 and 4..7 (uint64 arrays holding 32-bit values)"""
    M = np.uint64(0xFFFFFFFF)
    h = (k0 * np.uint64(0x9E3779B1) + k1 * np.uint64(0x85EBCA77) + np.uint64(((length << 27) & 0xFFFFFFFF) * 0x27D4EB2F & 0xFFFFFFFF)) & M
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x2C1B3C6D)) & M
    h ^= h >> np.uint64(13)
    return h


def secondary(g, n_slots):
    """jtk_common.h restated for pieces of <= 8 bytes: primary slot = mix * n_slots >> 32.  Of the entries that share a primary
    slot all, or all but one, live in their secondary slot, and the shared slot carries the overflow flag and a filter bit
    (mix & 15) for each of those.  Returns (entries that share a primary slot and are a blank and letters; absent pieces whose
    primary slot is such a one and whose filter bit is that of two of its entries -- one of which was turned away, whichever
    stayed --, so the device must read the piece's secondary slot)."""
    by_slot = {}
    for p in g.ranks:
        if len(p) <= 8:
            m = _mix(p)
            by_slot.setdefault(m * n_slots >> 32, []).append((m & 15, p))
    sure = np.zeros(n_slots, dtype=np.uint16)                         # filter bits that the slot certainly carries
    displaced = []
    for slot, ps in by_slot.items():
        if len(ps) >= 2:
            nib = [n for n, _ in ps]
            for n in set(nib):
                if nib.count(n) >= 2:
                    sure[slot] |= 1 << n
            displaced += [p for _, p in ps if p[:1] == b" " and p[1:].isalpha() and p[1:].islower() and p[1:].isascii() and len(p) >= 2]
    displaced = sorted(p for p in displaced if g.o.split(p) == [p])
    rng = np.random.default_rng(11)
    absent = []
    for length in (5, 6, 7, 8):
        by = rng.integers(97, 123, size=(1 << 20, 8), dtype=np.uint64)
        by[:, 0] = 32
        by[:, length:] = 0
        k0 = by[:, 0] | by[:, 1] << np.uint64(8) | by[:, 2] << np.uint64(16) | by[:, 3] << np.uint64(24)
        k1 = by[:, 4] | by[:, 5] << np.uint64(8) | by[:, 6] << np.uint64(16) | by[:, 7] << np.uint64(24)
        m = _mix_many(k0, k1, length)
        slot = (m * np.uint64(n_slots)) >> np.uint64(32)
        hit = np.nonzero((sure[slot] >> (m & np.uint64(15)).astype(np.uint16)) & 1)[0]
        for i in hit:
            p = bytes(by[i, :length].astype(np.uint8))
            assert _mix(p) == int(m[i])
            if p not in g.ranks and g.pairs_ok(p) and len(absent) < 64:
                absent.append(p)
    return displaced, absent


def secondary_case(g, n_slots):
    displaced, absent = secondary(g, n_slots)
    rnd = random.Random("secondary-text")
    parts = []
    for i, p in enumerate(displaced[:1500] + absent):
        parts.append(p)
        if i % 5 == 4:
            parts.append(g.w.fill[rnd.randint(3, 9)])
    c = Case("secondary", parts, {})
    c.n_displaced, c.n_absent = len(displaced), len(absent)
    return c
