"""Small texts for the two ends of k_piece_resolve around its probe loop (jtokkit_amd/csrc/jtk_kernels.hip): the piece list that
a tile builds from its 32 mask words -- the word counts and their prefix, taken once per tile, and each wave's share of the words
(wave v: the eight consecutive words 8 v .. 8 v + 7) --, and what happens to the pieces that miss the table: their bin, their
slot in the bin and the write-out of the bins that hold any.  Built and counted with the CPU oracle alone, like resolve_cases.py, whose Gen makes the
pieces: test_resolve_list_cases_cpu.py asserts that every text has the counts it is named for, test_resolve_list_gpu.py runs
the texts on the device.

A text is a list of piece lengths.  A piece of two or more bytes is a blank and lowercase letters (every blank starts a piece);
pieces of one byte come as a digit and a letter in turn.  Every adjacent byte pair inside a piece occurs in some table entry,
so pretok_split adds no cut and the device's piece list is the oracle's split.
"""
import random

import numpy as np

import pack_stage_cases as psc
import resolve_cases as rc

NAME = rc.NAME
T = rc.T
TW = T // 64                              # mask words per tile
RES_WAVES = rc.RES_WAVES
CHUNK = psc.CHUNK                         # the smallest JTK_OPT_CHUNK_BYTES
SECOND_BASE = psc.SECOND_BASE             # a first document of that many bytes: the second chunk starts in mid-tile
WORDS_PER_WAVE = TW // RES_WAVES          # wave v of the kernel builds the list entries of words 8 v .. 8 v + 7
ONE_WORD = (4, 9, 18, 27)                 # the word that holds all of a tile's pieces: one of each wave (wd // 8 = 0..3), and one
                                          # of each residue wd % 4 (the share of a kernel that deals the words out in turn)
ALL_WAVES_AT = 64                         # more queued pieces than that: all four waves write the tile's queue entries


class Case:
    def __init__(self, label, parts, docs=None):
        self.label, self.parts = label, parts
        self.text = np.frombuffer(b"".join(parts), dtype=np.uint8).copy()
        self.doc_off = np.array(sorted(set([0, len(self.text)] + list(docs or []))), dtype=np.int64)


def starts(g, case):
    """where the oracle's pieces start (text positions); every piece is checked for its byte pairs"""
    out, raw = [], case.text.tobytes()
    for d in range(len(case.doc_off) - 1):
        pos = int(case.doc_off[d])
        for p in g.o.split(raw[pos:int(case.doc_off[d + 1])]):
            assert g.pairs_ok(p), p[:40]
            out.append(pos)
            pos += len(p)
    return np.array(out, dtype=np.int64)


def word_counts(g, case):
    """piece starts per 64-byte mask word of the text"""
    n = np.zeros((len(case.text) + 63) // 64, dtype=np.int64)
    np.add.at(n, starts(g, case) // 64, 1)
    return n


def misses(g, case):
    """per tile: for each piece that starts in it, in list order, whether it misses the table and is queued (two or more
    tokens, at most BIN_MAXLEN bytes), and its bin (pack_stage_cases.bin_of; -1 for a piece that is not queued)"""
    st = starts(g, case)
    ends = np.append(st[1:], len(case.text))
    for d in case.doc_off[1:-1]:
        assert d in st
    raw = case.text.tobytes()
    out = [[] for _ in range((len(case.text) + T - 1) // T)]
    for s, e in zip(st.tolist(), ends.tolist()):
        p = raw[s:e]
        q = len(p) <= rc.BIN_MAXLEN and g.w.count(p) >= 2
        out[s // T].append(psc.bin_of(len(p)) if q else -1)
    return [np.array(t, dtype=np.int64) for t in out]


def _pieces(g, lengths, rnd):
    """pieces of those lengths: a run of ones is a digit and a letter in turn"""
    out, ones = [], 0
    for n in lengths:
        if n == 1:
            out.append(b"1a"[ones & 1:(ones & 1) + 1])
            ones += 1
        else:
            ones = 0
            out.append(g.w.fill[n] if n in g.w.fill and n <= 8 else g.word(n, rnd))
    return out


# ---- the list build ---------------------------------------------------------------------------------------------------------------

def word_shapes(g):
    """Tile 0: word 0 holds 64 piece starts, word 1 63, word 2 one (at bit 0: a piece of 191 bytes), word 3 none, word 4 one (at
    bit 63); fillers to the tile's end, the last of them starting at bit 63 of the tile's last word.  Tile 1: fillers, then the
    tile's and the text's last piece, which ends 27 bytes short of a multiple of 64."""
    rnd = random.Random("word_shapes")
    lengths = [1] * 64 + [1] * 62 + [2] + [191]
    used = sum(lengths)
    assert used == 4 * 64 + 63
    rest = T - 1 - used                                            # ... up to the tile's last byte, where a piece starts
    lengths += [len(p) for p in g.w.fillers(rest, rest // 6)]
    lengths += [5]                                                 # from bit 63 of word 31 into tile 1
    tail = 1000 - 27 - 4
    lengths += [len(p) for p in g.w.fillers(tail, tail // 7)]
    c = Case("word_shapes", _pieces(g, lengths, rnd))
    assert len(c.text) == T + 1000 - 27 and len(c.text) % 64 != 0
    return c


def one_word_tiles(g):
    """Per word of ONE_WORD (one of each wave's eight: the other three waves hold eight empty words) three tiles: fillers that
    end in a long piece, a tile whose only piece starts -- five short pieces and the start of the next long piece -- lie in that
    word, and the long piece's end among fillers.  Then a tile that lies inside one piece (np == 0)."""
    rnd = random.Random("one_word")
    lengths, tiles = [], {}
    for wd in ONE_WORD:
        base = sum(lengths)
        assert base % T == 0
        head = T - 300
        lengths += [len(p) for p in g.w.fillers(head, head // 8)]
        lengths += [300 + wd * 64 + 3]                              # ends at byte 3 of word wd of the next tile
        lengths += [4, 5, 6, 7, 8]
        tiles[base // T + 1] = wd
        lengths += [(T - wd * 64 - 33) + 200]                       # from byte 33 of the word to byte 200 of the tile after
        rest = T - 200
        lengths += [len(p) for p in g.w.fillers(rest, rest // 8)]
    base = sum(lengths)
    lengths += [len(p) for p in g.w.fillers(T - 40, (T - 40) // 8)] + [40 + T + 60]
    lengths += [len(p) for p in g.w.fillers(T - 60, (T - 60) // 8)]
    c = Case("one_word_tiles", _pieces(g, lengths, rnd))
    c.tiles, c.inside = tiles, base // T + 1
    return c


def second_chunk(g):
    """One filler document of SECOND_BASE bytes (more than a chunk of CHUNK bytes, not a multiple of the tile), then word_shapes
    as the second document: the second chunk's first tile has piece starts of the first document below its lead."""
    c0 = word_shapes(g)
    assert SECOND_BASE % 4 == 0
    c = Case("second_chunk", [g.w.fill[4]] * (SECOND_BASE // 4) + c0.parts, docs=[SECOND_BASE])
    return c


# ---- the pieces that miss ---------------------------------------------------------------------------------------------------------

def miss_tile(g, label, n_pieces, miss_at, hard_len=3):
    """One tile of exactly T bytes and n_pieces pieces: hard pieces of hard_len bytes at the list indices miss_at, one-token
    fillers everywhere else."""
    rnd = random.Random(label)
    miss_at = set(miss_at)
    assert all(0 <= i < n_pieces for i in miss_at)
    pool = [g.hard(hard_len, rnd) for _ in range(16)]
    n_fill = n_pieces - len(miss_at)
    fill = g.w.fillers(T - hard_len * len(miss_at), n_fill)
    rnd.shuffle(fill)
    parts, fi = [], 0
    for i in range(n_pieces):
        if i in miss_at:
            parts.append(pool[i % len(pool)])
        else:
            parts.append(fill[fi])
            fi += 1
    c = Case(label, parts)
    assert len(c.text) == T
    c.n_pieces, c.miss_at, c.hard_len = n_pieces, miss_at, hard_len
    return c


def chunk(c, lanes=range(64)):
    return [64 * c + l for l in lanes]


MISS_TILES = {
    # chunks 0..3 hold 0, 1, 63 and 64 misses (np = 320: wave 0 takes chunks 0 and 4 as a pair, the others a single pass each)
    "per_chunk_0_1_63_64": (320, chunk(1, [17]) + chunk(2, range(1, 64)) + chunk(3), 3),
    # wave 0's pair pass: both chunks all misses
    "pair_all": (330, chunk(0) + chunk(4), 3),
    # lanes 0 and 63 of every chunk, and nothing else
    "lanes_0_63": (330, [i for c in range(5) for i in chunk(c, [0, 63])], 4),
    # np = 600: wave 0 makes a pair pass (chunks 0, 4) and a single pass (chunk 8); only that one has misses
    "single_pass_only": (600, chunk(8), 3),
    # np = 512: wave 3 takes chunks 3 and 7; every other lane of those misses
    "wave3_only": (512, chunk(3, range(0, 64, 2)) + chunk(7, range(1, 64, 2)), 3),
    # 64 queued pieces: wave 0 alone writes the queue entries; 65: all waves do
    "queued_64": (300, list(range(3, 3 + 4 * 64, 4)), 4),
    "queued_65": (300, list(range(3, 3 + 4 * 65, 4)), 4),
    # the most misses a tile can have: 682 pieces of 3 bytes (and one filler of 2), 512 pieces of 4
    "most_of_3": (683, list(range(682)), 3),
    "most_of_4": (512, list(range(512)), 4),
}


def miss_case(g, label):
    n_pieces, at, hard_len = MISS_TILES[label]
    return miss_tile(g, label, n_pieces, at, hard_len)
