"""Texts for the 16-byte entries of the queue of 4..8-byte pieces (k_piece_resolve's write-out and lean_window / lean_bin<.., 0>
in jtk_kernels.hip: bytes, position and length in one word): built and checked with the CPU oracle alone.

Hard pieces are no table entries: a blank and rare Han characters, Cyrillic and Greek letters, or an emoji with or without
U+FE0F, kept when the oracle splits them off as one piece and encodes them to two tokens or more.  NOMERGE pieces are eight
bytes none of whose adjacent pairs is a 2-byte token of the rank file: eight single-byte tokens, the one case in which the merge
reads an entry's position before it stores the result (the tokens go to the position-indexed overflow array).

Layouts:
    Shards    every tile a document; the hard pieces stand in the tiles of chosen queue shards (tile % Q_SHARDS), each shard with
              its own number of entries and length pattern, all other tiles one-token fillers (as in test_merge_order_gpu.py)
    Dense     hard pieces back to back in documents of odd lengths: every shard's queue passes the window threshold, and the
              chunks of a job of several chunks start off the tile edges (lead != 0)
    Placed    NOMERGE pieces as a tile's first piece, as its last, and across a tile edge
"""
import base64
import os
import random
import re

import numpy as np

import oracle_lib
import pack_stage_cases as psc

T = psc.T
CSRC = os.path.join(oracle_lib.ROOT, "jtokkit_amd", "csrc")


def _define(header, name):
    with open(os.path.join(CSRC, header)) as f:
        m = re.search(r"^\s*#\s*define\s+%s\s+\(?(\d+)\)?\s" % name, f.read(), re.M)
    assert m, (header, name)
    return int(m.group(1))


Q_SHARDS = _define("jtk_kernels.h", "JTK_Q_SHARDS")
SPAN = _define("jtk_kernels.h", "JTK_M_WGS_PER_SHARD") * _define("jtk_kernels.hip", "JTK_ML_THREADS")   # entries of a pass of one round
RMAX = _define("jtk_merge_order_rules.h", "JTK_MO_RMAX")


def rounds(left, span=None):
    """jtk_mo_rounds restated"""
    span = span or SPAN
    return 4 if left >= 4 * span else 2 if left >= 2 * span else 1


WINDOWS_FROM = 2 * SPAN                             # entries of a shard from which on it is taken in ordered windows
assert rounds(WINDOWS_FROM) == 2 and rounds(WINDOWS_FROM - 1) == 1 and RMAX == 4

_CYR = "абвгдежзийклмнопрстуфхцчшщъыьэюя"
_GRK = "αβγδεζηθικλμνξοπρστυφχψω"
_EMOJI = [chr(c) for c in range(0x1F600, 0x1F650)] + [chr(c) for c in range(0x1F680, 0x1F6C6)] + [chr(c) for c in range(0x1F300, 0x1F321)]
POOL = 61                                           # distinct pieces per length: a result in another entry's place changes the tokens


def two_byte_tokens(name):
    out = set()
    with open(os.path.join(oracle_lib.DATA_DIR, oracle_lib.ENCODINGS[name]["file"]), "rb") as f:
        for line in f:
            if line.strip():
                tok = base64.b64decode(line.split()[0])
                if len(tok) == 2:
                    out.add(tok)
    return out


class Pieces:
    """Per length 4..8 a pool of hard pieces; letters[n]: those that end in a letter (a NOMERGE piece may follow them)."""

    def __init__(self, name):
        self.name = name
        self.w = psc.Words(name)
        self.o = self.w.o
        rnd = random.Random(16)
        han = lambda: chr(rnd.randrange(0x4E00, 0x9FA6))
        let = lambda: rnd.choice(_CYR + _GRK)
        emo = lambda: rnd.choice(_EMOJI)
        make = {4: [lambda: han()],
                5: [lambda: let() + let(), lambda: emo()],
                6: [lambda: let() + han(), lambda: han() + let()],
                7: [lambda: han() + han(), lambda: let() + let() + let()],
                8: [lambda: emo() + "️", lambda: let() + let() + han(), lambda: let() + han() + let()]}
        self.pool, self.letters = {}, {}
        for n, kinds in make.items():
            got, seen = [], set()
            for i in range(20000):
                if len(got) == POOL:
                    break
                p = (" " + kinds[i % len(kinds)]()).encode()
                if p in seen:
                    continue
                seen.add(p)
                assert len(p) == n, (n, p)
                if self.w.count(p) >= 2 and self.o.split(p) == [p]:
                    got.append(p)
            self.pool[n] = got
            self.letters[n] = [p for p in got if p.decode()[-1].isalpha()]
        # the condition of every test built on these: no length of the bin is missing
        for n in range(4, 9):
            assert len(self.pool[n]) == POOL and len(self.letters[n]) >= 8, (name, n, len(self.pool[n]), len(self.letters[n]))
        self.nomerge = self._nomerge()

    def _nomerge(self):
        """eight bytes of symbols, one piece, none of whose adjacent byte pairs is a 2-byte token"""
        two = two_byte_tokens(self.name)
        ok_pair = lambda a, b: bytes([a, b]) not in two
        alphabet = [c.encode() for c in "!\"#$%&'()*+,-./:;<=>?@[\\]^_`{|}~" + "".join(chr(c) for c in range(0xA1, 0xC0) if c != 0xAA and c != 0xAD and c != 0xB5 and c != 0xBA and c not in (0xB2, 0xB3, 0xB9, 0xBC, 0xBD, 0xBE))
                    + "".join(chr(c) for c in (0x2020, 0x2021, 0x2030, 0x203B, 0x20AA, 0x20B9, 0x2116, 0x2190, 0x2192, 0x2200, 0x2206, 0x221A, 0x2248, 0x2260, 0x25A0, 0x25CF, 0x2605, 0x2660, 0x266A, 0x3001, 0x3002, 0x300C))]
        alphabet = [c for c in alphabet if all(ok_pair(c[i], c[i + 1]) for i in range(len(c) - 1))]
        rnd = random.Random(8)
        out, seen = [], set()
        for lead in (b" ", b""):
            for _ in range(200000):
                if len(out) >= 24:
                    break
                p = lead
                while len(p) < 8:
                    cands = [c for c in alphabet if len(p) + len(c) <= 8 and (not p or ok_pair(p[-1], c[0]))]
                    if not cands:
                        break
                    p += rnd.choice(cands)
                if len(p) != 8 or p in seen:
                    continue
                seen.add(p)
                if len(self.o.merge_piece(p)) == 8 and self.o.split(b" ab" + p + b" cd") == [b" ab", p, b" cd"]:
                    out.append(p)
            if out:
                break
        assert len(out) >= 4, "no eight bytes that merge nothing"
        for p in out:
            assert all(ok_pair(p[i], p[i + 1]) for i in range(7)) and self.w.count(p) == 8
        return out


_pieces = {}


def pieces(name):
    if name not in _pieces:
        _pieces[name] = Pieces(name)
    return _pieces[name]


# ---- length patterns along a shard's queue (period 256: a window is some 256 consecutive entries) ----
def length(pattern, i):
    k = i % 256
    if pattern == "mixed":
        return 4 + (i * 7 + i // 5) % 5
    if pattern in ("all4", "all5", "all8"):
        return int(pattern[3:])
    if pattern == "ascending":                       # rounds of 4..5, 5..6, 6..7, 7..8 bytes
        return 4 + k * 5 // 256
    if pattern == "four_five":                       # every round within 5 slots
        return 4 + k % 2
    if pattern == "five_six":                        # every round ends on a 6-byte piece
        return 5 + k % 2
    if pattern == "one_seven":                       # one 7-byte piece among 255 of 4..6: the last round alone needs 8 slots
        return 7 if k == 101 else 4 + k % 3
    if pattern == "short":                           # mostly 4 bytes: dense enough for windows in small chunks
        return 4 if k % 8 else 5 + (k // 8) % 4
    assert pattern == "eights"                       # 8-byte pieces, every other one merging nothing
    return 8


def choose(P, pattern, i, after_letters=True):
    """the i-th piece of a pattern; a NOMERGE piece only where the piece before it ends in a letter"""
    n = length(pattern, i)
    if pattern == "eights" and i % 2 == 1:
        return P.nomerge[(i // 2) % len(P.nomerge)]
    if pattern in ("eights", "placed"):
        return P.letters[n][i % len(P.letters[n])]
    return P.pool[n][i % len(P.pool[n])]


class Shards:
    """spec: shard -> (entries, pattern).  Every tile a document."""

    def __init__(self, name, spec, tiles_per_shard):
        P = self.P = pieces(name)
        w = P.w
        self.name, self.spec = name, spec
        filler = b"".join(psc.tile(w, []))
        done = {s: 0 for s in spec}
        self.plan, parts = {}, []
        for g in range(tiles_per_shard * Q_SHARDS):
            s = g % Q_SHARDS
            if s not in spec or done[s] >= spec[s][0]:
                parts.append(filler)
                continue
            used, mine = 0, []
            while done[s] < spec[s][0]:
                p = choose(P, spec[s][1], done[s])
                if used + len(p) > T or T - used - len(p) == 1:
                    break
                mine.append(p)
                used += len(p)
                done[s] += 1
            rest = T - used
            parts.append(b"".join(mine + w.fillers(rest, (rest + 9) // 10)))
            self.plan[g] = mine
        self.count = done
        for s, (n, _) in spec.items():
            assert done[s] == n, (s, done[s], n)
        self.text = np.frombuffer(b"".join(parts), dtype=np.uint8).copy()
        self.doc_off = np.arange(tiles_per_shard * Q_SHARDS + 1, dtype=np.int64) * T
        assert len(self.text) == self.doc_off[-1]
        # the plan is what the oracle splits: every tile that holds hard pieces
        raw = self.text.tobytes()
        for g, mine in self.plan.items():
            got = P.o.split(raw[g * T:(g + 1) * T])
            assert got[:len(mine)] == mine, (g % Q_SHARDS, g)
            assert all(w.count(p) == 1 for p in got[len(mine):]), (g % Q_SHARDS, g)

    def where(self, d):
        s = d % Q_SHARDS
        return "tile %d, shard %d (%s)" % (d, s, "%d entries, %s" % self.spec[s] if s in self.spec else "fillers")


S2, S4 = 2 * SPAN, 4 * SPAN
MAIN_SPEC = {
    # the loop of 64 consecutive entries per wave alone (shard 0 and all shards not named here: no entry)
    1: (1, "mixed"), 2: (63, "mixed"), 3: (64, "mixed"), 4: (65, "mixed"), 20: (65, "eights"),
    # around the threshold, and what a pass of windows leaves behind: 1 and 63 entries
    5: (S2 - 1, "mixed"), 6: (S2, "mixed"), 7: (S2 + 1, "mixed"), 8: (S2 + 63, "mixed"), 9: (S4 + 1, "short"), 10: (S4 + 63, "short"),
    # rounds of one length, and rounds that end at each length
    11: (S2 + 100, "all4"), 12: (S2 + 100, "all5"), 13: (S2 + 100, "all8"), 14: (S4 + 100, "all4"), 15: (S4 + 100, "four_five"),
    16: (S2 + 100, "ascending"), 17: (S2 + 100, "five_six"), 18: (S2 + 100, "one_seven"), 19: (S4 + 100, "ascending"),
    # pieces that merge nothing inside ordered windows
    21: (S2 + 100, "eights"),
}
OTHER_SPEC = {1: (65, "mixed"), 5: (S2 + 100, "mixed"), 6: (S4 + 1, "ascending")}


def tiles_needed(spec):
    most = 0
    for n, pattern in spec.values():
        tiles, used = 1, 0
        for i in range(n):
            ln = length(pattern, i)
            if used + ln > T or T - used - ln == 1:
                tiles, used = tiles + 1, 0
            used += ln
        most = max(most, tiles)
    return most


class Dense:
    """n_bytes of hard pieces back to back, pattern `pattern`, cut into documents of odd lengths at piece boundaries."""

    def __init__(self, name, n_bytes, pattern="short", nomerge_every=97):
        P = self.P = pieces(name)
        parts, starts, pos, i = [], [], 0, 0
        docs, next_doc = [0], 3001
        while pos < n_bytes:
            p = choose(P, pattern, i)
            if i % nomerge_every == nomerge_every - 1:
                q = P.letters[6][i % len(P.letters[6])]
                parts.append(q); starts.append(pos); pos += len(q)
                p = P.nomerge[(i // nomerge_every) % len(P.nomerge)]
            parts.append(p); starts.append(pos); pos += len(p)
            i += 1
            if pos >= next_doc:
                docs.append(pos)
                next_doc = pos + 2500 + (len(docs) * 389) % 1777
        if docs[-1] != pos:
            docs.append(pos)
        self.parts = parts
        self.starts = np.array(starts, dtype=np.int64)
        self.text = np.frombuffer(b"".join(parts), dtype=np.uint8).copy()
        self.doc_off = np.array(docs, dtype=np.int64)
        raw = self.text.tobytes()
        for d in (0, 1, len(docs) // 2, len(docs) - 2):               # the oracle splits what was laid out
            a, b = docs[d], docs[d + 1]
            k = int(np.searchsorted(self.starts, a))
            got = P.o.split(raw[a:b])
            assert got == parts[k:k + len(got)] and sum(map(len, got)) == b - a, d

    def prefix(self, n_docs):
        out = Dense.__new__(Dense)
        out.P = self.P
        out.doc_off = self.doc_off[:n_docs + 1].copy()
        end = int(out.doc_off[-1])
        out.text = self.text[:end].copy()
        out.starts = self.starts[self.starts < end]
        return out

    def chunks(self, chunk_bytes):
        """the chunk plan (plan_device_chunks, k_plan_chunks of the library): first documents of the chunks"""
        n = len(self.text)
        first = [0]
        if n > chunk_bytes + chunk_bytes // 4 and len(self.doc_off) > 2:
            nc = -(-n // chunk_bytes)
            for c in range(1, nc):
                d = int(np.searchsorted(self.doc_off[:-1], c * chunk_bytes, side="left"))
                if first[-1] < d < len(self.doc_off) - 1:
                    first.append(d)
        return first

    def per_shard(self, chunk_bytes=1 << 40):
        """per chunk: (lead, entries of every shard's queue of 4..8-byte pieces)"""
        first = self.chunks(chunk_bytes) + [len(self.doc_off) - 1]
        out = []
        for c in range(len(first) - 1):
            a, b = int(self.doc_off[first[c]]), int(self.doc_off[first[c + 1]])
            base = a // T * T
            st = self.starts[(self.starts >= a) & (self.starts < b)]
            out.append((a - base, np.bincount(((st - base) // T) % Q_SHARDS, minlength=Q_SHARDS)))
        return out

    def where(self, d):
        return "document %d, bytes %d..%d" % (d, self.doc_off[d], self.doc_off[d + 1])


DENSE_BYTES = 4700000
WINDOW_CHUNK = 9 << 18                              # 2.25 MiB: two chunks of the dense text, both with shards in windows
_dense = {}


def dense(name):
    if name not in _dense:
        _dense[name] = Dense(name, DENSE_BYTES)
    return _dense[name]


def below(d):
    """the longest prefix of whole documents of a dense text that keeps every shard below the window threshold"""
    lo, hi = 1, len(d.doc_off) - 1
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if d.prefix(mid).per_shard()[0][1].max() < WINDOWS_FROM:
            lo = mid
        else:
            hi = mid - 1
    return d.prefix(lo)


class Placed:
    """NOMERGE pieces at chosen offsets: at a tile's byte 0, ending with a tile's last byte, and across tile edges."""

    STARTS = (1 * T, 3 * T - 8, 4 * T - 3, 5 * T - 7, 6 * T - 1, 7 * T + 1000)

    def __init__(self, name):
        P = self.P = pieces(name)
        w = P.w
        parts, pos = [], 0
        for k, at in enumerate(self.STARTS):
            lead = b"" if P.nomerge[0][:1] == b" " else P.letters[5][k]      # (a letter before a piece that has no blank of its own)
            gap = at - pos - len(lead)
            parts += w.fillers(gap, (gap + 7) // 8)
            parts += [lead, P.nomerge[k % len(P.nomerge)]] if lead else [P.nomerge[k % len(P.nomerge)]]
            pos = at + 8
        parts += w.fillers(900, 100)
        pos += 900
        self.text = np.frombuffer(b"".join(parts), dtype=np.uint8).copy()
        assert len(self.text) == pos
        self.doc_off = np.array([0, 700, 3 * T - 8, 5 * T + 1, pos], dtype=np.int64)     # (one document starts on such a piece)
        raw, at = self.text.tobytes(), {}
        for d in range(len(self.doc_off) - 1):
            p0 = int(self.doc_off[d])
            for p in P.o.split(raw[p0:int(self.doc_off[d + 1])]):
                at[p0] = p
                p0 += len(p)
        for k, st in enumerate(self.STARTS):
            assert at.get(st) == P.nomerge[k % len(P.nomerge)] and len(P.o.merge_piece(at[st])) == 8, (k, st)

    def where(self, d):
        return "document %d" % d
