"""Texts whose 2 KiB tiles hold chosen numbers of merged ("hard") pieces per length class and a chosen number of tokens, for
k_pack_tokens' LDS staging of merge results (jtokkit_amd/csrc/jtk_stage_rules.h): built and checked with the CPU oracle alone.

Every piece is a blank and a run of lowercase letters, so each is one pre-token wherever it stands and any sequence of them
splits back into exactly these pieces.  Hard pieces are words the oracle encodes to two or more tokens; fillers are words that
are one token.  A tile is a list of pieces of exactly 2048 bytes; profile() recounts, from the oracle's split and merges of the
finished text, what each tile holds, and the tests assert the targeted counts on that before anything runs on a device.

Which of a bin's results the kernel finds in the staged head, in the extension or in neither follows the order in which
k_piece_resolve's lanes claimed queue indices, not text order: a case that needs a piece of some kind in one of those places
has more pieces of that kind than the other places can hold.
"""
import random

import numpy as np

import oracle_lib

T = 2048
CAP = (32, 16, 16, 8, 8, 8, 8)          # heads staged per bin (JTK_PACK_CAP)
SLOTS, OUT_SLOTS, STAGE = 96, 192, 768
TINY = 7
CHUNK = 1 << 16                         # the smallest JTK_OPT_CHUNK_BYTES
SECOND_BASE = CHUNK + 1000              # where the case starts as the second chunk of a job: not on a tile edge (lead = 1000)
NAME = "cl100k_base"

_FILLER_WORDS = ("a", "of", "the", "with", "which", "people", "between", "children", "different", "government", "information",
                 "development", "organization", "international", "understanding", "responsibility", "characteristics",
                 "to", "and", "that", "there", "should", "because", "important", "something", "university", "environment",
                 "relationship", "particularly", "administration", "recommendations")


def bin_of(length):
    if length <= 3:
        return TINY
    if length <= 16:
        return 0 if length <= 8 else 1 if length <= 12 else 2
    return 3 + (int(length - 1).bit_length() - 5)            # 17..32: 3, 33..64: 4, ...


class Words:
    """Fillers by byte length and hard words by length and token count, found with the oracle (seeded: the same every run)."""

    def __init__(self, name=NAME):
        self.o = oracle_lib.get(name)
        self._count = {}
        self.fill = {}
        for wd in _FILLER_WORDS:
            p = b" " + wd.encode()
            if len(p) not in self.fill and self.count(p) == 1 and self.o.split(p) == [p]:
                self.fill[len(p)] = p
        self.max_fill = max(n for n in range(2, 20) if all(k in self.fill for k in range(2, n + 1)))
        assert self.max_fill >= 12, sorted(self.fill)
        self._hard = {}

    def count(self, piece):
        if piece not in self._count:
            self._count[piece] = len(self.o.merge_piece(piece))
        return self._count[piece]

    def hard(self, length, k, lo=2, hi=99, letters="qxzjvkwy"):
        """k distinct hard pieces of `length` bytes that become lo..hi tokens."""
        key = (length, k, lo, hi, letters)
        if key in self._hard:
            return self._hard[key]
        want = lambda c: lo <= c <= hi
        rnd = random.Random(length * 1000 + k + sum(map(ord, letters)))
        out, seen = [], set()
        for _ in range(200000):
            if len(out) == k:
                self._hard[key] = out
                return out
            p = b" " + "".join(rnd.choice(letters) for _ in range(length - 1)).encode()
            if p in seen:
                continue
            seen.add(p)
            if want(self.count(p)) and self.o.split(p) == [p]:
                out.append(p)
        raise AssertionError("no %d hard pieces of %d bytes" % (k, length))

    def fillers(self, n_bytes, n):
        """n one-token pieces of n_bytes bytes together."""
        if n == 0:
            assert n_bytes == 0
            return []
        base, rem = divmod(n_bytes, n)
        assert 2 <= base and base + (1 if rem else 0) <= self.max_fill, (n_bytes, n)
        return [self.fill[base + 1]] * rem + [self.fill[base]] * (n - rem)


def cycle(pool, n):
    return [pool[i % len(pool)] for i in range(n)]


def tile(words, hard, total=None):
    """A tile of exactly T bytes: the hard pieces spread evenly among one-token fillers; `total` tokens in all (default: fillers
    of about ten bytes)."""
    hb, ht = sum(len(p) for p in hard), sum(words.count(p) for p in hard)
    rest = T - hb
    assert rest >= 0
    k = (rest + 9) // 10 if total is None else total - ht
    if rest == 0:
        assert k == 0
    fill = words.fillers(rest, k)
    # spread: a hard piece after every len(fill) / len(hard) fillers
    out, fi = [], 0
    for i, p in enumerate(hard):
        upto = (i + 1) * len(fill) // (len(hard) + 1)
        out += fill[fi:upto]
        fi = upto
        out.append(p)
    out += fill[fi:]
    assert sum(len(p) for p in out) == T
    return out


def room_for(total):
    return OUT_SLOTS - (0 if total > STAGE else (total + 3) // 4)


def placement(total, nq):
    """jtk_stage_rules restated: (n[b], first slot) per bin."""
    over = [max(nq[b] - CAP[b], 0) for b in range(7)]
    room, before, n = room_for(total), 0, []
    for b in range(7):
        n.append(min(before + over[b], room) - min(before, room))
        before += over[b]
    return n, over


class Case:
    """tiles: lists of pieces (each T bytes); doc_at(tile index, piece index in tile, piece) -> a document starts there."""

    def __init__(self, label, words, tiles, doc_at=None):
        self.label, self.words, self.tiles = label, words, tiles
        self.doc_at = doc_at or (lambda t, i, p: i % 37 == 11)

    def batch(self, base=0):
        """(text, doc_off).  base = 0: the case alone, its tiles on tile edges after one tile of fillers.  base = SECOND_BASE:
        behind one filler document of that many bytes, padded to the next tile edge: the tiles are the same."""
        w = self.words
        parts, docs, pos = [], [0], 0
        if base:
            assert base % 4 == 0
            parts.append(w.fill[4] * (base // 4))
            pos = base
            docs.append(pos)
            pad = (-pos) % T
            lead = w.fillers(pad, (pad + 7) // 8)
            parts += lead
            pos += pad
        for ti, tl in enumerate([tile(w, [])] + self.tiles):
            for i, p in enumerate(tl):
                if ti > 0 and self.doc_at(ti - 1, i, p) and pos not in docs:
                    docs.append(pos)
                parts.append(p)
                pos += len(p)
        tail = w.fillers(700, 70)                                  # a partial last tile
        parts += tail
        pos += 700
        docs.append(pos)
        text = np.frombuffer(b"".join(parts), dtype=np.uint8).copy()
        assert len(text) == pos
        return text, np.array(docs, dtype=np.int64)

    def first_tile(self, base=0):
        """index (in the whole text) of the tile that self.tiles[0] fills"""
        return (base + T - 1) // T + 1


def profile(words, text, doc_off):
    """Per tile of the text: tokens of the pieces that start in it, and hard pieces per bin (index 7: tiny) -- from the oracle's
    own split and merges."""
    n_tiles = (len(text) + T - 1) // T
    total = np.zeros(n_tiles, dtype=np.int64)
    nq = np.zeros((n_tiles, 8), dtype=np.int64)
    raw = text.tobytes()
    for d in range(len(doc_off) - 1):
        pos = int(doc_off[d])
        for p in words.o.split(raw[pos:int(doc_off[d + 1])]):
            c = words.count(p)
            total[pos // T] += c
            if c >= 2:
                nq[pos // T, bin_of(len(p))] += 1
            pos += len(p)
    return total, nq


def bin0_tile(words, h, total):
    """h hard pieces of 4 bytes and 2 tokens, `total` tokens in the tile"""
    return tile(words, cycle(words.hard(4, 24, 2, 2), h), total)


def cases(words):
    """label -> (Case, what the target tiles must hold: a list of checks on (total, nq) per target tile)"""
    out = {}
    w = words
    h4 = lambda n: cycle(w.hard(4, 24, 2, 2), n)
    h10 = lambda n: cycle(w.hard(10, 12, 2, 5), n)
    h14 = lambda n: cycle(w.hard(14, 12, 2, 7), n)
    h14_7 = lambda n: cycle(w.hard(14, 6, 7, 7), n)
    h16_big = lambda n: cycle(w.hard(16, 6, 8), n)
    h24 = lambda n: cycle(w.hard(24, 6), n)
    h3 = lambda n: cycle(w.hard(3, 8), n)

    # bin 0 at the head's cap: 31 / 32 / 33 hard pieces
    out["cap"] = Case("cap", w, [bin0_tile(w, h, 300) for h in (31, 32, 33)]), [
        dict(total=300, nq0=31), dict(total=300, nq0=32), dict(total=300, nq0=33)]
    # ... at the end of the room: total 400 -> 92 free slots -> 32 + 92 - 1 / + 0 / + 1
    r = room_for(400)
    out["room"] = Case("room", w, [bin0_tile(w, 32 + r + d, 400) for d in (-1, 0, 1)]), [
        dict(total=400, nq0=32 + r - 1, ext0=r - 1), dict(total=400, nq0=32 + r, ext0=r), dict(total=400, nq0=32 + r + 1, ext0=r)]
    # the worst the text allows: 512 hard pieces of 4 bytes (1024 tokens: unstaged, 192 slots); then bins 0, 1 and 2 overflowing
    # in one tile with the room running out inside bin 1; then the same with tiny and long pieces around
    mixed = h4(60) + h10(40) + h14(30)
    t_mixed = 640
    out["worst"] = Case("worst", w, [h4(512), tile(w, mixed, t_mixed), tile(w, h4(50) + h10(30) + h14(20) + h24(12) + h3(30))]), [
        dict(total=1024, nq0=512, ext0=192), dict(total=t_mixed, nq0=60, nq1=40, nq2=30, mid=1), dict(nq0=50, nq1=30, nq2=20, nq3=12, nq7=30)]
    # token totals around the stage, each with an overflowing bin 0
    out["stage"] = Case("stage", w, [bin0_tile(w, 80, t) for t in (767, 768, 769)]), [
        dict(total=767, nq0=80, ext0=0), dict(total=768, nq0=80, ext0=0), dict(total=769, nq0=80, ext0=48)]
    # a staged tile with no free slot and with one (total 764 -> slot 191 free), and with two
    out["free"] = Case("free", w, [bin0_tile(w, 40, t) for t in (765, 764, 760)]), [
        dict(total=765, nq0=40, ext0=0), dict(total=764, nq0=40, ext0=1), dict(total=760, nq0=40, ext0=2)]
    # bin 2 in the extension: pieces of more than 7 tokens (tokens in htok) beside ones of fewer -- 20 of each kind, 16 head
    # slots: at least 4 of either kind are served from the extension --, and pieces of exactly 7 tokens likewise
    big = [p for pair in zip(h16_big(20), h14(20)) for p in pair]
    sev = [p for pair in zip(h14_7(20), h14(20)) for p in pair]
    out["counts"] = Case("counts", w, [tile(w, big + h4(40)), tile(w, sev + h4(40))]), [
        dict(nq0=40, nq2=40, ext2=24), dict(nq0=40, nq2=40, ext2=24)]
    # a document starts on every hard piece: on staged ones, on extension-served ones and on those after the room's end
    r = room_for(640)
    out["docs"] = Case("docs", w, [bin0_tile(w, 32 + r + 6, 640), bin0_tile(w, 32 + r + 6, 640)],
                       doc_at=lambda t, i, p: (w.count(p) >= 2) if t == 0 else i % 3 == 0), [
        dict(total=640, nq0=32 + r + 6, ext0=r), dict(total=640, nq0=32 + r + 6, ext0=r)]
    return out


def check_targets(words, case, want, base=0):
    """The oracle's recount of the finished text against what the case set out to build."""
    text, doc_off = case.batch(base)
    total, nq = profile(words, text, doc_off)
    t0 = case.first_tile(base)
    assert len(text) <= base + (len(case.tiles) + 3) * T
    for k, wnt in enumerate(want):
        tt, q = int(total[t0 + k]), nq[t0 + k]
        n, over = placement(tt, q)
        for key, v in wnt.items():
            if key == "total":
                assert tt == v, (case.label, k, key, tt, v)
            elif key.startswith("nq"):
                assert q[int(key[2:])] == v, (case.label, k, key, q.tolist(), v)
            elif key.startswith("ext"):
                assert n[int(key[3:])] == v, (case.label, k, key, n, v)
            elif key == "mid":                                     # the room ends inside bin `v`: the bins before it are whole
                assert 0 < n[v] < over[v] and all(n[b] == over[b] for b in range(v)) and over[v + 1] > 0 and n[v + 1] == 0, (case.label, k, n, over)
    return text, doc_off
