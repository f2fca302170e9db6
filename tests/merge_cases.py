"""Pieces and texts that send irregular pieces through every implementation of bytePairMerge inside k_bpe_merge
(jtokkit_amd/csrc/jtk_kernels.hip), at the first and last lengths of each and at the queue sizes where the dispatch changes:
built with the CPU oracle, merge_ref.py and the host shim alone.  test_merge_cases_cpu.py asserts on the CPU what the set
covers; test_merge_paths_gpu.py runs the texts on the device.

    path            piece bytes   code
    tiny            2..3          tiny_bin
    b0 / b1 / b2    4..8 / 9..12 / 13..16    lean_bin<16,1024,0..2> -> lean_piece16<8/12/16>
    l32 / l64       17..32 / 33..64          lean_bin<32,512,3>, lean_bin<64,256,4>: bytes read from the text
    sm128 / sm256   65..128 / 129..256       merge_bin<128,..,5>, merge_bin<256,..,6>
    mid / long      257..512 / 513..8192     merge_long<512>, merge_long<8192>
    giant           8193..1 MiB              merge_giant

Piece kinds -- each is one pre-token wherever it stands between fillers (one-token words that start with a blank) or at either
end of a document, which check_splits asserts with the oracle's split of the finished documents:
    rare    a blank and letters of a small alphabet of rare letters: many tokens, few merges
    words   a blank and vocabulary words run together: deep merge chains, sensitive to a stale neighbour rank
    multi   a blank and Cyrillic, CJK, Hangul or accented letters, an ASCII letter where the length needs one: high ids
    sym     runs of = - * # / _ . ~ of 1..130 bytes (shorter runs in short pieces): ties everywhere, parts of more than 64 bytes
    defect  a blank and "ab" repeated, one foreign letter far inside: ties whose positions lie on both sides of an edge
    blank   blanks and tabs that end their document

Not covered: giants of more than 20,000 bytes (the CPU oracle is quadratic; merge_giant keeps one chunk minimum per thread up to
262,144 bytes and several beyond), and more than M_CHUNK entries of one shard in bin 6 (sm256 shares merge_bin with sm128, which
crowded() takes past M_CHUNK).
"""
import ctypes as C
import os
import random
import subprocess

import numpy as np

import merge_ref
import oracle_lib
import pack_stage_cases as psc
from pack_stage_cases import Words, bin_of, profile

NAME = "cl100k_base"
T = 2048                                # JTK_TILE
BIN_LAST = (3, 8, 12, 16, 32, 64, 128, 256)   # last length of tiny, bins 0..6 (BIN16 and the clz rule of k_piece_resolve; JTK_BIN_MAXLEN)
MID_CAP = 512                           # JTK_MID_CAP
LONG_CAP = 8192                         # JTK_LONG_CAP
GIANT_CHUNK = 256                       # JTK_GIANT_CHUNK
Q_SHARDS = 64                           # JTK_Q_SHARDS
M_WGS_PER_SHARD = 4                     # JTK_M_WGS_PER_SHARD
ML_THREADS = 1024                       # JTK_ML_THREADS
M_CHUNK = 2048                          # M_CHUNK (merge_bin)
GRID_WGS = Q_SHARDS * M_WGS_PER_SHARD   # workgroups of k_bpe_merge: the stride of the long and giant lists
GRID_WAVES = GRID_WGS * ML_THREADS // 64   # ... and of the mid list
ONE_PASS = {"tiny": ML_THREADS, "b0": ML_THREADS, "b1": ML_THREADS, "b2": ML_THREADS, "l32": ML_THREADS // 2,
            "l64": ML_THREADS // 4, "sm128": M_CHUNK}       # entries of one shard that one workgroup pass takes
GIANT_TOP = 20000

PATHS = (("tiny", 2, 3), ("b0", 4, 8), ("b1", 9, 12), ("b2", 13, 16), ("l32", 17, 32), ("l64", 33, 64), ("sm128", 65, 128),
         ("sm256", 129, 256), ("mid", 257, MID_CAP), ("long", MID_CAP + 1, LONG_CAP), ("giant", LONG_CAP + 1, GIANT_TOP))
PATH_NAMES = tuple(p[0] for p in PATHS)
LEAN = ("b0", "b1", "b2", "l32", "l64")          # result words of 32-bit halves (lean_bin)
STATE = ("sm128", "sm256")                       # result words of 64-bit halves (merge_bin)
TEXT_READERS = PATH_NAMES[4:]                    # paths that read the piece's bytes from the text
KINDS = ("rare", "words", "sym", "multi")
PLACES = ("a0", "a1", "a15", "tile_end", "doc_first")


def path_of(length):
    for name, lo, hi in PATHS:
        if lo <= length <= hi:
            return name
    raise AssertionError(length)


def lengths_of(path):
    """first, first + 1, last - 1 and last; for giant: first, the last cached chunk of exactly 256 positions, that and one more
    position, and about 20,000"""
    name, lo, hi = PATHS[PATH_NAMES.index(path)]
    if name == "giant":
        return (lo, 33 * GIANT_CHUNK, 33 * GIANT_CHUNK + 1, GIANT_TOP)
    return tuple(sorted({lo, lo + 1, hi - 1, hi}))


def kinds_of(path):
    return KINDS if PATH_NAMES.index(path) >= 2 else KINDS[:3]      # multi from b1 up


# ---- the host shim: the lane merge of jtk_merge_core.h and the lean bins' pair lookups, on the CPU -----------------------------

class Sim:
    def __init__(self, name=NAME):
        d = os.path.join(oracle_lib.ROOT, "tests", "hostsim")
        subprocess.check_call(["make", "-C", d, "-s"])
        L = C.CDLL(os.path.join(d, "libjtk_hostsim.so"))
        L.sim_tables_create.restype = C.c_void_p
        L.sim_tables_create.argtypes = [C.c_char_p, C.c_int, C.c_char_p, C.c_size_t, C.POINTER(C.c_int)]
        L.sim_merge_piece.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_void_p]
        L.sim_merge_piece_stats.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_void_p, C.c_void_p]
        cfg = oracle_lib.ENCODINGS[name]
        with open(os.path.join(oracle_lib.DATA_DIR, cfg["file"]), "rb") as f:
            data = f.read()
        st = C.c_int(0)
        self.L, self.h = L, L.sim_tables_create(name.encode(), cfg["kind"], data, len(data), C.byref(st))
        assert self.h and st.value == 0

    def merge(self, piece):
        out = np.empty(64, dtype=np.int32)
        n = self.L.sim_merge_piece(self.h, piece, len(piece), out.ctypes.data)
        assert n >= 1, n
        return out[:n].tolist()

    def stats(self, piece):
        """(tokens, lookups answered from a secondary bucket, lookups that miss in a flagged bucket and in the secondary one)"""
        out, st = np.empty(64, dtype=np.int32), np.zeros(3, dtype=np.int64)
        n = self.L.sim_merge_piece_stats(self.h, piece, len(piece), out.ctypes.data, st.ctypes.data)
        assert n >= 1, n
        return out[:n].tolist(), int(st[0]), int(st[1])


# ---- pieces -----------------------------------------------------------------------------------------------------------------------

RARE = "qxzjvkwy"
SYM = "=-*#/_.~"
_MULTI2 = "абвгдежзиклмнопрстуфхцчшщыэюяéèêëàâäöüßñçõãíóúýřžčěůąęłńśźż"
_MULTI3 = ("的一是不了人我在有他这中大来上国个到说们为子和你地出道也时年得就那要下以生会自着去之过家学对可她里后小么心多天而能好都然"
           "龘靐齉爨灪麤鱻驫饕餮魑魅魍魉"
           "한국어는아름답다가나라마바사자차카타파하긁꿻뷁쉙")


class Entry:
    def __init__(self, label, kind, piece, place=None, then=None):
        self.label, self.kind, self.piece, self.place, self.then = label, kind, piece, place, then
        self.length, self.path = len(piece), path_of(len(piece))

    def __repr__(self):
        return "%s [%s, %s, %d bytes%s]" % (self.label, self.path, self.kind, self.length, ", " + self.place if self.place else "")


class Pieces:
    """The generators and the oracle's verdict on what they make, for one encoding (seeded: the same every run)."""

    def __init__(self, name=NAME):
        self.name = name
        self.w = Words(name)
        self.o = self.w.o
        self.ranks = merge_ref.load_ranks("p50k_base" if name == "p50k_edit" else name)
        self.max_token = max(len(k) for k in self.ranks)
        self.by_len = {}
        for k in sorted(self.ranks):
            if len(k) <= 9 and k.isalpha() and k.islower():
                self.by_len.setdefault(len(k), []).append(k)
        self.lacking = []                # (kind, length) that the vocabulary does not provide as a piece of two or more tokens
        self._sim = None

    @property
    def sim(self):
        if self._sim is None:
            self._sim = Sim(self.name)
        return self._sim

    def count(self, p):
        return self.w.count(p)

    def tokens(self, p):
        return self.o.merge_piece(p)

    def gen(self, kind, length, rnd, blank=None):
        if kind == "rare":
            return b" " + "".join(rnd.choice(RARE) for _ in range(length - 1)).encode()
        if kind == "words":
            out, rest = [b" "], length - 1
            while rest:
                k = rest if rest <= 3 else rnd.randint(3, min(9, rest))
                if rest - k in (1, 2) and k < 7:
                    k = rest                                      # no one- or two-letter tail
                out.append(rnd.choice(self.by_len[k]))
                rest -= k
            return b"".join(out)
        if kind == "multi":
            out, rest = [b" "], length - 1
            while rest:
                if rest == 1:
                    c = rnd.choice(RARE)
                elif rest == 2 or (rest != 3 and rnd.random() < 0.5):
                    c = rnd.choice(_MULTI2)
                else:
                    c = rnd.choice(_MULTI3)
                out.append(c.encode())
                rest -= len(out[-1])
            return b"".join(out)
        if kind == "sym":
            lead = (rnd.random() < 0.5) if blank is None else blank
            top = 130 if length > 64 else max(2, length // 3)
            s = " " if lead else ""
            while len(s) < length:
                s += rnd.choice(SYM) * rnd.randint(1, top)
            return s[:length].encode()
        if kind == "blank":
            return "".join(rnd.choice(" \t") for _ in range(length)).encode()
        raise AssertionError(kind)

    def defect(self, length, at, unit="ab", letter=b"q"):
        body = bytearray((unit.encode() * length)[:length - 1])
        body[at - 1:at] = letter
        return b" " + bytes(body)

    def stands_alone(self, p, last=False):
        """one pre-token after a filler, before a filler and at either end of a document"""
        a, b = self.w.fill[4], self.w.fill[3]
        if last:
            return self.o.split(a + p) == [a, p] and self.o.split(p) == [p]
        return self.o.split(a + p + b) == [a, p, b] and self.o.split(p + b) == [p, b] and self.o.split(a + p) == [a, p]

    def pick(self, kind, length, seed, want=None, tries=4000, blank=None):
        """a piece of that kind and length that merges to two or more tokens (and satisfies `want`), or None"""
        rnd = random.Random("%s/%d/%s" % (kind, length, seed))
        seen = set()
        for _ in range(tries):
            p = self.gen(kind, length, rnd, blank)
            if p in seen:
                continue
            seen.add(p)
            if (length > self.max_token or self.count(p) >= 2) and self.stands_alone(p, kind == "blank") and (want is None or want(p)):
                return p
        return None

    def mutant_changes(self, p, mutant):
        return merge_ref.merge_ref(p, self.ranks, mutant)[0] != merge_ref.merge_ref(p, self.ranks)[0]


def base_entries(P):
    """every (kind, length) of every path: two pieces up to 64 bytes, one beyond"""
    out = []
    for path in PATH_NAMES:
        for length in lengths_of(path):
            for kind in kinds_of(path):
                for rep in range(2 if length <= 64 else 1):
                    p = P.pick(kind, length, "base%d" % rep)
                    if p is None:
                        if rep == 0:
                            P.lacking.append((kind, length))
                        continue
                    out.append(Entry("%s/%s/%d/%d" % (path, kind, length, rep), kind, p))
    return out


def hunted_entries(P, have):
    """Pieces searched for what the plain ones above may lack: a changed result under every mutant on the short paths, token counts
    of <= 6, 7 and 8 on the paths that write a result word, an id >= 65536 at every position of a result word, lookups that go to
    a secondary bucket on the lean paths, far neighbours on the long paths.  A search that finds nothing adds nothing: the CPU
    tier asserts what the whole set holds."""
    out = []
    pool = lambda path: [e for e in have + out if e.path == path]

    def hunt(label, path, want, kinds=KINDS, tries=300, lengths=None):
        name, lo, hi = PATHS[PATH_NAMES.index(path)]
        rnd = random.Random(label)
        for k in range(tries):
            kind = kinds[k % len(kinds)]
            if kind == "multi" and hi < 9:
                continue
            length = rnd.choice(lengths) if lengths else rnd.randint(lo, hi)
            p = P.pick(kind, length, "%s%d" % (label, k), tries=1)
            if p is not None and want(p):
                out.append(Entry("%s/%s/%d/%s" % (path, kind, length, label), kind, p))
                return True
        return False

    # every mutant on every path of up to 512 bytes (the longer ones: the plain pieces, see the CPU tier)
    for path in PATH_NAMES[:9]:
        for mutant in merge_ref.MUTANTS if path != "tiny" else ("rightmost",):
            if any(P.mutant_changes(e.piece, mutant) for e in pool(path)):
                continue
            if path == "tiny":                                     # a tie in three bytes: three of a kind
                for c in SYM + "!?+<>|":
                    p = (c * 3).encode()
                    if P.count(p) >= 2 and P.stands_alone(p) and P.mutant_changes(p, mutant):
                        out.append(Entry("tiny/sym/3/%s" % mutant, "sym", p))
                        break
            else:
                hunt(mutant, path, lambda p: P.mutant_changes(p, mutant), tries=600)
    # token counts in a result word
    for path in LEAN + STATE:
        for label, ok in (("le6", lambda n: n <= 6), ("eq7", lambda n: n == 7), ("eq8", lambda n: n == 8)):
            if not any(ok(P.count(e.piece)) for e in pool(path)):
                hunt(label, path, lambda p: ok(P.count(p)), kinds=("sym", "words", "multi", "rare"), tries=3000)
    # an id of more than 16 bits at every position of a result word
    if max(P.ranks.values()) >= 65536:
        for writer, paths in (("lean", LEAN), ("state", STATE)):
            for at in range(7):
                hit = lambda p: len(P.tokens(p)) <= 7 and len(P.tokens(p)) > at and P.tokens(p)[at] >= 65536
                if any(hit(e.piece) for path in paths for e in pool(path)):
                    continue
                for path in (paths[::-1] if writer == "lean" else paths):
                    if hunt("hi%d" % at, path, hit, kinds=("multi", "sym", "words"), tries=4000):
                        break
    # the second round of the lean bins' lookups
    for path in LEAN:
        for k, label in ((1, "second"), (2, "flagged")):
            if not any(P.sim.stats(e.piece)[k] for e in pool(path)):
                hunt(label, path, lambda p: P.sim.stats(p)[k] > 0, tries=3000)
    # neighbours more than a ballot away (giant pieces are long enough to have them: the CPU tier looks)
    far = lambda p: (lambda tr: tr.ahead.max() > 64 and tr.prev_len.max() > 64)(merge_ref.merge_ref(p, P.ranks)[1])
    for path, lengths in (("mid", None), ("long", range(MID_CAP + 1, 1100))):
        if not any(far(e.piece) for e in pool(path) if e.length <= 1100):
            hunt("far", path, far, kinds=("sym",), tries=200, lengths=lengths)
    return out


DEFECT_UNITS = ("ab", "a", "aab", "aa", "e", "ss", "abb", "s")


def defect_entries(P):
    """A blank and a short unit repeated ties at every repeat; one foreign letter far inside.  "ab" gives ties on both sides of
    every edge, but cl100k_base has no token over "abab", so the order in which its ties are taken does not show; the second unit
    is the first of DEFECT_UNITS for which it does (the last minimum taken first changes the tokens).  Per edge -- slot 63 (the
    lean bins' masks, the ballots' stride), 511 and 8191 (the LDS of merge_long) -- the letter once near the end and once just
    past the edge."""
    shows = [u for u in DEFECT_UNITS if P.mutant_changes(P.defect(100, 91, u), "rightmost")]
    out = []
    for edge, length in ((63, 100), (63, 200), (511, 700), (8191, 8400)):
        for unit in ("ab",) + tuple(shows[:1]):
            for at in (length - 9, edge + 6):
                p = P.defect(length, at, unit)
                assert P.stands_alone(p)
                out.append(Entry("%s/defect/%d/%s-edge%d@%d" % (path_of(length), length, unit, edge, at), "defect", p))
    return out


def placed_entries(P):
    """For the paths that read the text: every edge length again at pos & 15 of 0, 1 and 15, starting in the last 16 bytes of a
    tile and as the first piece of a document (kinds in rotation); two giants back to back in one document (letters, then
    symbols); a giant that is a whole document; blank runs that end their documents."""
    out, k = [], 0
    for path in TEXT_READERS:
        for length in lengths_of(path):
            for place in PLACES:
                kind = KINDS[k % 4]
                k += 1
                p = P.pick(kind, length, "placed" + place)
                out.append(Entry("%s/%s/%d/%s" % (path, kind, length, place), kind, p, place))
    g1, g2 = P.pick("words", 8200, "pair"), P.pick("sym", 9000, "pair", blank=False)
    assert P.o.split(g1 + g2) == [g1, g2]
    out.append(Entry("giant/words/8200/pair", "words", g1, then=Entry("giant/sym/9000/pair", "sym", g2)))
    out.append(Entry("giant/multi/8500/doc_whole", "multi", P.pick("multi", 8500, "whole"), "doc_whole"))
    for length in (5, 12, 20, 40, 100, 200, 300, 600, 8200):
        p = P.pick("blank", length, "blank")
        if p is not None:
            out.append(Entry("%s/blank/%d" % (path_of(length), length), "blank", p, "doc_last"))
    return out


def tail_entries(P):
    """one piece per edge length of the text-reading paths, to stand as the last bytes of a text of its own"""
    out, k = [], 1
    for path in TEXT_READERS:
        for length in lengths_of(path):
            kind = KINDS[k % 4]
            k += 1
            out.append(Entry("%s/%s/%d/text_last" % (path, kind, length), kind, P.pick(kind, length, "tail"), "text_last"))
    return out


# ---- texts ------------------------------------------------------------------------------------------------------------------------

class Text:
    def __init__(self, label, text, doc_off, cases, left_out=(), ballast=0):
        self.label, self.text, self.doc_off, self.cases, self.left_out = label, text, doc_off, cases, list(left_out)
        self.ballast = ballast           # bytes at the front that hold hard pieces which are no cases
        self._starts = np.array([c[0] for c in cases], dtype=np.int64)

    def where(self, pos):
        """what stands at byte `pos` of the text: the case piece there, or the last one before it"""
        k = int(np.searchsorted(self._starts, pos, side="right")) - 1
        if k < 0:
            return "%s: before the first case piece" % self.label
        at, e = self.cases[k]
        inside = "in" if pos < at + e.length else "in the fillers %d bytes after" % (pos - at - e.length)
        return "%s: %s %r at byte %d (pos & 15 = %d, byte %d of tile %d, shard %d)" % (
            self.label, inside, e, at, at & 15, at % T, at // T, at // T % Q_SHARDS)


class _Builder:
    def __init__(self, P, label):
        self.P, self.w, self.label = P, P.w, label
        self.parts, self.docs, self.pos, self.cases, self.left_out, self.ballast = [], [0], 0, [], [], 0
        self.rnd = random.Random(label)

    def raw(self, b):
        self.parts.append(b)
        self.pos += len(b)

    def new_doc(self):
        if self.docs[-1] != self.pos:
            self.docs.append(self.pos)

    def fill(self, n_bytes):
        """one-token fillers of n_bytes bytes together (0, or 2 and more)"""
        if n_bytes:
            for f in self.w.fillers(n_bytes, (n_bytes + 7) // 8):
                self.raw(f)

    def some_fill(self):
        self.fill(self.rnd.randint(8, 40))

    def fill_to(self, mod, rem):
        gap = (rem - self.pos) % mod
        self.fill(gap + mod if gap == 1 else gap)

    def piece(self, e):
        self.cases.append((self.pos, e))
        self.raw(e.piece)

    def add(self, e, one_doc=False):
        if one_doc:
            self.some_fill()
            self.piece(e)
            return
        self.new_doc()
        if e.place == "doc_whole":
            self.piece(e)
            self.new_doc()
            return
        if e.place != "doc_first":
            self.some_fill()
        if e.place in ("a0", "a1", "a15"):
            self.fill_to(16, int(e.place[1:]))
        if e.place == "tile_end":
            self.fill_to(T, T - 16 + self.rnd.randrange(16))
        if e.place == "text_last" and (self.pos + e.length) % 16 == 0:
            self.fill(3)
        self.piece(e)
        if e.then is not None:
            self.piece(e.then)
        if e.place == "doc_last":
            self.new_doc()
        elif e.place != "text_last":
            self.some_fill()

    def finish(self):
        self.new_doc()
        text = np.frombuffer(b"".join(self.parts), dtype=np.uint8).copy()
        assert len(text) == self.pos
        return Text(self.label, text, np.array(self.docs, dtype=np.int64), self.cases, self.left_out, self.ballast)


class Plan:
    """All case pieces of one encoding, made once."""

    def __init__(self, name=NAME):
        self.P = P = Pieces(name)
        self.base = base_entries(P)
        self.hunted = hunted_entries(P, self.base)
        self.defect = defect_entries(P)
        self.placed = placed_entries(P)
        self.tails = tail_entries(P)
        self.entries = self.base + self.hunted + self.defect + self.placed        # what per_piece() lays out
        self.everything = self.entries + [e.then for e in self.entries if e.then] + self.tails

    def per_piece(self, label="per_piece", lead=None):
        """every piece in a document of its own among fillers"""
        b = _Builder(self.P, label)
        if lead is not None:
            lead(b)
        for e in self.entries:
            b.add(e)
        b.new_doc()
        b.fill(50)
        return b.finish()

    def tail_texts(self):
        """texts that end with their piece, their lengths no multiple of 16"""
        out = []
        for e in self.tails:
            b = _Builder(self.P, "tail:" + e.label)
            b.fill(64)
            b.new_doc()
            b.add(e)
            t = b.finish()
            assert len(t.text) % 16 != 0 and t.cases[-1][0] + e.length == len(t.text)
            out.append(t)
        return out

    def one_document(self):
        b = _Builder(self.P, "one_document")
        last = None
        for e in self.entries:
            if e.kind == "blank":
                last = e                                           # a blank run ends its document: one of them, at the end
                continue
            b.add(e, one_doc=True)
            if e.then is not None:
                b.piece(e.then)
        b.some_fill()
        b.piece(last)
        t = b.finish()
        assert len(t.doc_off) == 2
        return t

    def second_chunk(self):
        """per_piece behind one filler document of SECOND_BASE bytes, cut to what two chunks of 64 KiB hold: every plain and
        hunted piece of up to 514 bytes, the defect pieces up to 700, one piece each of 8191, 8192 and 8193 bytes, and the placed
        pieces up to 258 bytes; left_out names the rest."""
        b = _Builder(self.P, "second_chunk")
        base = psc.SECOND_BASE
        b.raw(b.w.fill[4] * (base // 4))
        room = 2 * psc.CHUNK - base - 200
        big = set()
        for e in self.entries:
            fits = e.length <= 258 or (e.place is None and e.length <= 700) or (
                e.place is None and e.kind == "sym" and e.length in (8191, 8192, 8193) and e.length not in big)
            need = e.length + (e.then.length if e.then else 0) + 100 + (T if e.place == "tile_end" else 0)
            if not fits or e.then is not None or need > room:
                b.left_out.append(e.label)
                continue
            if e.length > 700:
                big.add(e.length)
            before = b.pos
            b.add(e)
            room -= b.pos - before
        t = b.finish()
        assert t.doc_off[1] == base and psc.CHUNK * 5 // 4 < len(t.text) <= 2 * psc.CHUNK, len(t.text)
        return t

    def sliced(self):
        """per_piece behind a ballast from byte 0: 192 tiles of 512 four-byte pieces of two tokens, 1536 bin-0 entries in every
        shard -- no shard of the launch fits one pass, so none runs its bins side by side: workgroup k of a shard takes the k-th
        slice of each bin that has one"""
        def lead(b):
            hard = b.w.hard(4, 24, 2, 2)
            for t in range(3 * Q_SHARDS):
                b.new_doc()
                b.raw(b"".join(psc.cycle(hard[t % 24:] + hard[:t % 24], T // 4)))
            b.ballast = b.pos
        return self.per_piece("sliced", lead)


def _distinct(P, kinds, lo, hi, n, label, blank=True):
    """n different pieces of lo..hi bytes, kinds in rotation, each hard and alone after and before its like"""
    rnd = random.Random(label)
    out, seen = [], set()
    k = 0
    while len(out) < n:
        k += 1
        assert k < 40 * n + 1000, (label, len(out))
        kind = kinds[k % len(kinds)]
        length = rnd.randint(lo, hi)
        if kind == "letters":                                      # (three-byte pieces: the rare alphabet has too few)
            p = b" " + "".join(rnd.choice("abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ") for _ in range(length - 1)).encode()
        else:
            p = P.gen(kind, length, rnd, blank)
        if p in seen or (length <= P.max_token and P.count(p) < 2):
            continue
        seen.add(p)
        out.append(Entry("%s/%s/%d/%s%d" % (path_of(length), kind, length, label, len(out)), kind, p))
    return out


def crowded(P):
    """One text in which one shard per bin gets more entries than one pass of a workgroup takes (ONE_PASS): every 64th tile is a
    tile of one bin's pieces, all different, the other tiles are one-token fillers.  tiny .. l64 leave side_by_side and take the
    sliced dispatch in their shard; sm128 goes past M_CHUNK in merge_bin.  sm256 runs the same merge_bin template and is not
    repeated here.  Returns (Text, {path: shard})."""
    spec = (("sm128", 0, ("rare", "words", "sym", "multi"), 65, 66), ("tiny", 5, ("letters",), 3, 3),
            ("b0", 10, ("rare", "words", "sym"), 5, 8), ("b1", 15, KINDS, 9, 12), ("b2", 20, KINDS, 13, 16),
            ("l32", 25, KINDS, 28, 32), ("l64", 30, KINDS, 60, 64))
    b = _Builder(P, "crowded")
    filler = b"".join(psc.tile(P.w, []))
    pools, shards = {}, {}
    for path, shard, kinds, lo, hi in spec:
        pools[shard] = _distinct(P, kinds, lo, hi, ONE_PASS[path] + 60, "crowded-" + path)[::-1]
        shards[path] = shard
    while any(pools.values()):
        for shard in range(Q_SHARDS):
            b.new_doc()
            pool = pools.get(shard)
            if not pool:
                b.raw(filler)
                continue
            end = b.pos + T
            while pool and b.pos + pool[-1].length <= end and end - b.pos - pool[-1].length != 1:
                b.piece(pool.pop())
            b.fill(end - b.pos)
            assert b.pos == end
    return b.finish(), shards


def lists(P, n_giant=GRID_WGS + 1, giant_hi=8500):
    """More mid pieces than the grid has waves and more long pieces and giants than it has workgroups, all different: some wave
    and some workgroup takes a second piece into the LDS (and, for giants, the cache) that it has used for its first."""
    b = _Builder(P, "lists")
    mids = _distinct(P, KINDS, 257, 300, GRID_WAVES + 3, "list-mid", blank=None)
    longs = _distinct(P, KINDS, 513, 640, GRID_WGS + 3, "list-long", blank=None)
    giants = _distinct(P, KINDS, LONG_CAP + 1, giant_hi, n_giant, "list-giant", blank=None)
    every = [e for trio in zip(mids[::16], longs, giants) for e in trio]          # the three lists fill side by side
    used = set(every)
    every += [e for e in mids + longs + giants if e not in used]
    for k, e in enumerate(every):
        if k % 8 == 0:
            b.new_doc()
        b.some_fill()
        b.piece(e)
    b.some_fill()
    return b.finish()


def tile_counts(P, t):
    """Per tile of the text, the pieces of two or more tokens that start in it, per path (PATH_NAMES order): profile() of
    pack_stage_cases carried on past 256 bytes."""
    n = np.zeros(((len(t.text) + T - 1) // T, len(PATHS)), dtype=np.int64)
    raw = t.text.tobytes()
    for d in range(len(t.doc_off) - 1):
        pos = int(t.doc_off[d])
        for p in P.o.split(raw[pos:int(t.doc_off[d + 1])]):
            if len(p) > P.max_token or P.count(p) >= 2:
                n[pos // T, PATH_NAMES.index(path_of(len(p)))] += 1
            pos += len(p)
    return n


def check_splits(P, t):
    """Every document of the text splits into the planned pieces at the planned positions and one-token fillers between them.
    Returns the number of pieces."""
    raw = t.text.tobytes()
    want = {at: e.length for at, e in t.cases}
    found, n = 0, 0
    for d in range(len(t.doc_off) - 1):
        pos = int(t.doc_off[d])
        for p in P.o.split(raw[pos:int(t.doc_off[d + 1])]):
            n += 1
            if pos < t.ballast:
                pass
            elif pos in want:
                assert len(p) == want[pos], (t.where(pos), len(p))
                found += 1
            else:
                assert len(p) <= P.w.max_fill and P.count(p) == 1, (t.where(pos), p[:40])
            pos += len(p)
    assert found == len(want), (t.label, found, len(want))
    return n
