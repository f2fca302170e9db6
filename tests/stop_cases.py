"""The cases of the stop-string tests (CPU tier: tests/test_stop_rules_cpu.py; GPU tier: tests/test_stop_strings_gpu.py), and
the edges a case set must reach, computed from the cases and the reference's results, so that neither tier can pass by
missing one.

A case is a matrix of cells.  A cell is the byte string of one token (every single byte is a token of the shipped tables; the
few longer ones used here are listed in TOKENS and the GPU tier checks that the table holds them), PAD (a pad cell, skipped) or
UNK (an id without an entry): the last two contribute no bytes.  Rows are padded with PAD to the case's width.  The decoded
text, byte_off and cell_byte follow from the cells alone."""
import os
import random
import re

import numpy as np

PAD, UNK = "PAD", "UNK"
TOKENS = [b" the", b" world", b"hello"]

_HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "jtokkit_amd", "csrc", "jtk_stop_rules.h")


def _define(name):
    m = re.search(r"^#define\s+%s\s+(\d+)\b" % name, open(_HDR).read(), re.M)
    return int(m.group(1))


LANE = _define("JTK_STOP_LANE")                     # bytes per lane
WAVE = 64 * LANE
TILE = _define("JTK_STOP_LANES") * LANE             # JTK_STOP_TILE
MAX_STRINGS, MAX_BYTES = 16, 64                     # the ABI's limits

S64 = bytes(range(0x30, 0x30 + 64))                 # a 64-byte string of distinct bytes '0'..'o'


def B(b):
    """Single-byte cells."""
    return [bytes([x]) for x in b]


def dots(n):
    return B(b"." * n)


class Case:
    def __init__(self, name, rows, strings, frm=None):
        self.name, self.rows, self.frm = name, rows, frm
        self.strings = [s.encode("utf-8") if isinstance(s, str) else s for s in strings]
        self.width = max([len(r) for r in rows], default=0)
        n = len(rows)
        self.byte_off = np.zeros(n + 1, dtype=np.int64)
        self.cell_byte = np.zeros((n, self.width), dtype=np.int64)
        parts, at = [], 0
        for r, row in enumerate(rows):
            self.byte_off[r] = at
            for c in range(self.width):
                self.cell_byte[r, c] = at
                cell = row[c] if c < len(row) else PAD
                if cell not in (PAD, UNK):
                    parts.append(cell)
                    at += len(cell)
        self.byte_off[n] = at
        self.out = b"".join(parts)

    def cell(self, r, c):
        return self.rows[r][c] if c < len(self.rows[r]) else PAD

    def from_array(self):
        return None if self.frm is None else np.array(self.frm, dtype=np.int64)


def _edge_case():
    """Matches of "ab" across a lane, a wave and a tile edge, a 64-byte string that starts 63 bytes before a tile edge, a tail
    held back across a tile edge: positions are absolute, so every row's length is chosen for where the next one starts."""
    rows, at = [], 0

    def row(length, p, s):                        # a row of `length` bytes with s at absolute position p
        nonlocal at
        k = p - at
        assert 0 <= k and k + len(s) <= length
        rows.append(dots(k) + B(s) + dots(length - k - len(s)))
        at += length

    row(40, LANE - 1, b"ab")
    row(WAVE - 24, WAVE - 1, b"ab")
    row(TILE - at + 44, TILE - 1, b"ab")
    row(2 * TILE - at + 48, 2 * TILE - 63, S64)
    end = 3 * TILE + 5                            # the row ends 5 bytes into the fourth tile with 9 bytes of S64: 4 before the edge
    row(end - at, end - 9, S64[:9])
    row(200, at + 100, b"ab")
    return Case("edges", rows, [S64, b"ab"])


def _fuzz_case(seed, n_rows, alphabet, strings):
    rng = random.Random(seed)
    rows = []
    for _ in range(n_rows):
        n = rng.choice([0, 0, 1, 2, 3, 5, 8, 13, 16, 17, 31, 40, 70])
        cells = []
        for _ in range(n):
            cells.append(bytes([rng.choice(alphabet)]))
            if rng.random() < 0.15:
                cells.append(rng.choice([PAD, UNK]))
        rows.append(cells)
    frm = [rng.choice([0, 0, 0, 1, 2, 5, -3, 100]) for _ in range(n_rows)]
    return Case("fuzz%d" % seed, rows, strings, frm)


def cases():
    sixteen = [b"q%02d" % i for i in range(14)] + [b"Z", S64]
    out = [
        _edge_case(),
        Case("row_straddle", [dots(3) + B(b"ST"), B(b"OP") + dots(2), dots(2) + B(b"STOP") + dots(2), B(b"STO"), B(b"P")], [b"STOP"]),
        Case("first_last", [B(b"ab...."), B(b"....ab"), B(b"ab"), B(b".ab.")], [b"ab"]),
        Case("short_rows", [[], B(b"a"), B(b"ab"), [], [PAD, UNK], B(b"x"), B(b"abc"), B(b"abcd.")], [b"abc", b"abcd"]),
        Case("empty_runs", [dots(TILE - 2) + B(b"ab"), [], [], [], B(b"ab") + dots(5), [], [], dots(TILE - 7 - 2), [], [], B(b"b"), B(b"a")],
             [b"ab"]),
        Case("tie_short_first", [B(b"..abc.."), B(b"abc"), B(b".ab")], [b"ab", b"abc"]),
        Case("tie_long_first", [B(b"..abc.."), B(b"abc"), B(b".ab")], [b"abc", b"ab"]),
        Case("duplicates", [B(b"..ab.."), B(b"a")], [b"ab", b"ab", b"b", b"b"]),
        Case("self_overlap", [B(b"baaaa"), B(b"baa"), B(b"aaaaaaa"), B(b"ba")], [b"aaa", b"aa"]),
        Case("dense", [B(b"a" * (TILE + 100)), B(b"a"), B(b"aa" * 20)], [b"aa", b"a", b"aaa"]),
        Case("from", [B(b"..ab..ab.."), B(b"..ab.."), B(b"ab..ab"), B(b"..ab"), B(b"ab"), [], B(b"abab")], [b"ab"],
             [3, 100, -5, 4, 2, 7, 1]),
        Case("hold_longest", [B(b"..abc"), B(b"..ab"), B(b"c"), B(b"..bcx..abc")], [b"abcd", b"bcx", b"cq"]),
        Case("hold_before_S", [B(b"..ab"), B(b"..ab"), B(b"..ab")], [b"ab", b"bz"], [3, 2, 4]),
        Case("hold_zero_by_match", [B(b"x..ab"), B(b"..ab"), B(b"abx")], [b"abc", b"x"]),
        Case("hold_max", [dots(5) + B(S64[:63]), B(S64[:63]), B(S64[1:]), dots(2) + B(S64)], [S64, b"!"]),
        Case("tokens", [[b".", PAD, b" the", b" world"], [b".", PAD, UNK, b"hello", b"."], B("xé→y".encode()) + [PAD],
                        [b"hello", PAD, b" the", UNK, b" world"], [PAD, PAD, b" the"]],
             [b"e w", b"hel", "é→", b"o t"]),
        Case("n0", [B(b"abc"), [], B(b"Z")], []),
        Case("n1", [B(b"abcZ"), [], B(b"Z"), B(b"abc")], [b"Z"]),
        Case("n16", [B(b"..q07"), B(b"q1"), dots(3) + B(S64) + dots(3), B(b".Z"), B(S64[:10]), B(b"q13q00")], sixteen),
        Case("no_rows", [], [b"ab"]),
        Case("all_empty", [[], [PAD], []], [b"ab"]),
        _fuzz_case(1, 300, b"ab.", [b"ab", b"aab", b"ba.", b"b"]),
        _fuzz_case(2, 300, b"abc", [b"abca", b"cab", b"bb", b"abcabc"]),
    ]
    assert len(set(c.name for c in out)) == len(out)
    return out


ALL_EDGES = {
    "lane_straddle", "wave_straddle", "tile_straddle", "s64_63_before_tile", "row_straddle_no_match", "row_straddle_same_bytes_match",
    "match_first_byte", "match_last_byte", "empty_row", "one_byte_row", "row_shorter_than_every_string", "empty_run_on_tile_edge",
    "tie_short_first", "tie_long_first", "duplicate_wins", "self_overlap", "dense_row", "from_cuts_match", "from_beyond",
    "from_negative", "from_eq_len", "hold_longest_wins", "hold_whole_string_before_S", "hold_zero_by_earlier_match",
    "hold_across_tile", "hold_maxlen_minus_1", "multibyte_string", "match_inside_token_into_later", "col_after_byteless_cells",
    "n0", "n1", "n16", "len1", "len64", "three_tiles",
}


def edges_reached(case, result):
    """The edges of ALL_EDGES that `case` reaches, given the reference's (stop_pos, stop_which, hold, stop_col) for it."""
    pos, which, hold, col = result
    out, strings, off = case.out, case.strings, case.byte_off
    maxlen = max([len(s) for s in strings], default=0)
    got = set()
    n = len(case.rows)
    got.add({0: "n0", 1: "n1", MAX_STRINGS: "n16"}.get(len(strings), "n_other"))
    if len(out) >= 3 * TILE:
        got.add("three_tiles")
    spans, matched = set(), set()                 # strings that lie across the end of a row that has no match | strings that matched
    for q in range(n):
        b, e = int(off[q]), int(off[q + 1])
        f = 0 if case.frm is None else case.frm[q]
        s0 = b + min(max(f, 0), e - b)
        if case.frm is not None:
            if f > e - b:
                got.add("from_beyond")
            if f < 0:
                got.add("from_negative")
            if f == e - b and e > b:
                got.add("from_eq_len")
        if e == b:
            got.add("empty_row")
            if q + 1 < n and off[q + 2] == b and b > 0 and b % TILE == 0:
                got.add("empty_run_on_tile_edge")
        if e - b == 1:
            got.add("one_byte_row")
        if strings and 0 < e - b < min(len(s) for s in strings):
            got.add("row_shorter_than_every_string")
        tails = [p for p in range(max(s0, e - (maxlen - 1)), e) if any(len(s) > e - p and s.startswith(out[p:e]) for s in strings)]
        if which[q] < 0:
            for i, s in enumerate(strings):
                for p in range(s0, e):
                    if p + len(s) > e and out[p:p + len(s)] == s:
                        spans.add(s)
                for p in range(b, s0):
                    if p + len(s) == e and out[p:e] == s:
                        got.add("hold_whole_string_before_S")
            if len(tails) >= 2 and hold[q] == e - tails[0]:
                got.add("hold_longest_wins")
            if hold[q] > 0 and (e - hold[q]) // TILE != (e - 1) // TILE:
                got.add("hold_across_tile")
            if maxlen >= 3 and hold[q] == maxlen - 1:
                got.add("hold_maxlen_minus_1")
            continue
        p, s = int(pos[q]), strings[which[q]]
        last = p + len(s) - 1
        matched.add(s)
        for name, x in (("lane_straddle", LANE), ("wave_straddle", WAVE), ("tile_straddle", TILE)):
            if p // x != last // x:
                got.add(name)
        if len(s) == 64 and maxlen == 64 and (p + 63) % TILE == 0:
            got.add("s64_63_before_tile")
        got.add("len%d" % len(s))
        if p == b:
            got.add("match_first_byte")
        if last == e - 1:
            got.add("match_last_byte")
        if tails:
            got.add("hold_zero_by_earlier_match")
        both = [t for t in strings if out[p:p + len(t)] == t and p + len(t) <= e and t != s and (t.startswith(s) or s.startswith(t))]
        for t in both:
            got.add("tie_short_first" if len(s) < len(t) else "tie_long_first")
        if strings.count(s) > 1:
            got.add("duplicate_wins")
        if any(out[p + d:p + d + len(s)] == s and p + d + len(s) <= e for d in range(1, len(s))):
            got.add("self_overlap")
        if e - b >= TILE and all(any(out[x:x + len(t)] == t for t in strings) for x in range(b, e)):
            got.add("dense_row")
        if any(out[x:x + len(t)] == t and x < s0 < x + len(t) for t in strings for x in range(b, s0)):
            got.add("from_cuts_match")
        if any(x >= 0x80 for x in s):
            got.add("multibyte_string")
        c = int(col[q])
        if case.cell_byte[q, c] < p and last >= case.cell_byte[q, c] + len(case.cell(q, c)):
            got.add("match_inside_token_into_later")
        if c > 0 and case.cell(q, c - 1) in (PAD, UNK) and case.cell_byte[q, c] == p:
            got.add("col_after_byteless_cells")
    if spans:
        got.add("row_straddle_no_match")
    if spans & matched:
        got.add("row_straddle_same_bytes_match")
    return got
