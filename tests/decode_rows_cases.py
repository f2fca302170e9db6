"""Seeded inputs for the decode of id matrices, built for the edges of jtk_decode_rows.hip: shared by
tests/test_decode_rows_rules_cpu.py (rule header == reference, and the coverage conditions on these inputs) and
tests/test_decode_rows_gpu.py (device == reference).

A case is a dict: name, rows int64 [n_rows, width] (the values; `wide` says that some need 64 bits), begin / end (int64 [n_rows] or
None), pad_id, stop (list of ids), skip_pad, keep_stop.  Cells are numbered t = r * width + c; T = cells per tile, 8 per lane,
512 per wave; a tile whose bytes exceed S is written straight to global memory, any other is assembled in LDS.  Ids are picked
by byte length from the table under test (decode_cases.table), never hard-coded.
"""
import numpy as np

import decode_cases as dc
import decode_rows_ref

T = dc.T
S = dc.S
TABLES = dc.TABLES
WIDTHS = (0, 1, 7, 8, 9, 63, 64, 65, 511, 512, 513, 2047, 2048, 2049, 5000)
WIDE_BAD = (2 ** 63 - 1, -2 ** 63)                  # with 2^32 + a valid id: what only a 64-bit cell can hold


def rows_for(width):
    """Rows so that the cells span at least 3 tiles plus a ragged tail."""
    return 5 if width == 0 else -(-(3 * T + 100) // width)


class _Builder:
    def __init__(self, name, seed):
        self.tab = dc.table(name)
        self.h = dc._Builder(self.tab, seed)          # its id pickers: uniform, bad, tile, ids_of_lengths
        self.rng = self.h.rng
        self.n = self.tab.n_ids_table
        self.special = sorted(self.tab.specials)[-1]                      # a special token's id (its literal is its bytes)
        self.no_entry = self.n + 7                                        # an id without an entry, for a stop id
        known = self.h.known
        self.eos, self.pad_valid = int(known[len(known) // 3]), int(known[len(known) // 2])
        self.cases, self.names = [], set()

    def add(self, name, rows, begin=None, end=None, pad_id=0, stop=(), skip_pad=False, keep_stop=False):
        rows = np.asarray(rows, dtype=np.int64)
        assert rows.ndim == 2 and name not in self.names, name
        self.names.add(name)
        nr = rows.shape[0]
        fix = lambda a: None if a is None else np.asarray(a, dtype=np.int64).reshape(nr)
        wide = bool(rows.size) and bool((rows > 2 ** 31 - 1).any() or (rows < -2 ** 31).any())
        self.cases.append(dict(name=name, rows=rows, begin=fix(begin), end=fix(end), pad_id=int(pad_id), stop=[int(s) for s in stop],
                               skip_pad=bool(skip_pad), keep_stop=bool(keep_stop), wide=wide))

    def known(self, nr, width, avoid=()):
        """A matrix of ids that all have an entry, none of them in `avoid`."""
        m = self.h.uniform(nr * width).reshape(nr, width)
        for a in avoid:
            while (m == a).any():
                m[m == a] = self.h.uniform(int((m == a).sum()))
        return m

    def windows(self, nr, width):
        """Random windows: inside, equal, crossed, negative, beyond the row."""
        b = self.rng.integers(0, width + 1, size=nr)
        e = self.rng.integers(0, width + 1, size=nr)
        kind = self.rng.integers(0, 6, size=nr)
        lo, hi = np.minimum(b, e), np.maximum(b, e)
        b, e = np.where(kind == 1, hi, lo), np.where(kind == 1, lo, hi)   # 1: crossed
        e = np.where(kind == 2, b, e)                                     # 2: equal
        b = np.where(kind == 3, -1 - b, b)                                # 3: negative begin
        e = np.where(kind == 4, width + 1 + e, e)                         # 4: end beyond the row
        return b, e

    def generated(self, nr, width):
        """Rows as generate() leaves them: left pad fill, a prompt, a generated part, an EOS, then EOS fill to the row's end."""
        m = self.known(nr, width, avoid=(self.eos, self.pad_valid))
        for r in range(nr):
            lp = int(self.rng.integers(0, width + 1)) if self.rng.random() < 0.5 else 0
            m[r, :lp] = -1
            if self.rng.random() < 0.8 and width:
                m[r, int(self.rng.integers(0, width)):] = self.eos
        return m

    # ---- the case families ----------------------------------------------------------------------------
    def widths(self):
        for width in WIDTHS:
            nr = rows_for(width)
            self.add("plain_w%d" % width, self.known(nr, width))
            if width == 0:
                self.add("w0_with_options", self.known(nr, 0), begin=[0, 1, -1, 0, 5], end=[0, 0, 3, -2, 1], pad_id=-1,
                         stop=[self.eos], skip_pad=True)
                continue
            m = self.generated(nr, width)
            at = self.rng.random(m.shape) < 0.002
            m[at] = self.h.bad(int(at.sum()))
            b, e = self.windows(nr, width)
            self.add("generated_w%d" % width, m, pad_id=-1, stop=[self.eos], skip_pad=True)
            self.add("generated_windows_w%d" % width, m, b, e, pad_id=-1, stop=[self.eos], skip_pad=True, keep_stop=bool(width % 2))
        self.add("no_rows_w7", np.zeros((0, 7)))
        self.add("no_rows_w0", np.zeros((0, 0)), pad_id=-1, stop=[self.eos], skip_pad=True)

    def stage_edge(self):
        """Tiles of exactly x bytes between staged and between direct neighbours (rows of 1024 cells: two per tile)."""
        st, d = 9000, S + 7
        for x in (S - 1, S, S + 1):
            self.add("stage_%d_between_staged" % x, np.concatenate([self.h.tile(st), self.h.tile(x), self.h.tile(st + 1)]).reshape(6, 1024))
            self.add("stage_%d_between_direct" % x, np.concatenate([self.h.tile(d), self.h.tile(x), self.h.tile(d + 2)]).reshape(6, 1024))
        # the same edge with rows that straddle the tiles, and a ragged last tile
        ids = np.concatenate([self.h.tile(S + 1), self.h.tile(S), self.h.tile(st, 2904)])
        self.add("stage_ragged_w1000", ids.reshape(7, 1000))
        # pad cells skipped inside a tile: its bytes come from the other cells alone
        m = np.concatenate([self.h.tile(S + 3), self.h.tile(S - 1)]).reshape(4, 1024)
        wide = np.full((4, 1030), -1, dtype=np.int64)
        wide[:, 3:1027] = m
        self.add("stage_inside_pad_fill", wide, pad_id=-1, skip_pad=True)

    def _at_flat(self, width, nr, residues, mod):
        """Per row r < nr a column c with (r * width + c) % mod == residues[r % len(residues)], 0 < c < width - 1."""
        cols = []
        for r in range(nr):
            want = residues[r % len(residues)]
            c = (want - r * width) % mod
            while c < 1:
                c += mod
            assert c < width - 1
            cols.append(c)
        return np.array(cols, dtype=np.int64)

    def stop_edges(self):
        width, nr = 5000, 12
        res = [(7, 8), (0, 8), (511, 512), (0, 512), (2047, 2048), (0, 2048)]
        cols = np.array([self._at_flat(width, nr, [a], mod)[r] for r, (a, mod) in zip(range(nr), res + res)], dtype=np.int64)
        stops8 = [self.eos] + [int(x) for x in self.known(1, 7, avoid=(self.eos, self.special))[0]]
        base = self.known(nr, width, avoid=stops8 + [self.special])
        for fill in ("single", "dense"):
            m = base.copy()
            for r in range(nr):
                if fill == "dense":
                    m[r, cols[r]:] = self.eos
                else:
                    m[r, cols[r]] = self.eos
            self.add("stop_first_hit_on_edges_%s" % fill, m, stop=[self.eos])
            self.add("stop_first_hit_on_edges_%s_kept" % fill, m, stop=[self.eos], keep_stop=True)
        m = base.copy()
        for r in range(nr):                                               # one of eight stop ids each, others of the eight behind it
            m[r, cols[r]] = stops8[r % 8]
            m[r, cols[r] + 1] = stops8[(r + 3) % 8]
        self.add("stop_eight_ids", m, stop=stops8)
        self.add("stop_eight_ids_kept", m, stop=stops8, keep_stop=True)
        self.add("stop_none_given", m)
        # hit at b, at e - 1, at width - 1, left of b (ignored), right of e (ignored), with dense fill behind
        b = self._at_flat(width, nr, [7, 0, 511, 0, 2047, 0], 2048) + 40
        e = b + np.array([1, 2, 9, 600, 2100, 3000, 1, 2, 9, 600, 2100, 2500])
        e = np.minimum(e, width)
        for what in ("at_b", "at_e_minus_1", "left_of_b", "at_e", "at_last_column"):
            m = base.copy()
            bb, ee = b.copy(), e.copy()
            for r in range(nr):
                if what == "at_last_column":
                    bb[r], ee[r] = (0, width) if r % 2 else (b[r], width + 5)
                c = {"at_b": bb[r], "at_e_minus_1": ee[r] - 1, "left_of_b": bb[r] - 1, "at_e": ee[r], "at_last_column": width - 1}[what]
                if c < width:
                    m[r, c] = self.eos
                if what == "left_of_b" and r % 2:
                    m[r, :bb[r]] = self.eos                                # a dense run that ends right at the window
            self.add("stop_%s" % what, m, bb, ee, stop=[self.eos])
            self.add("stop_%s_kept" % what, m, bb, ee, stop=[self.eos], keep_stop=True)
        # KEEP_STOP: a special token's literal appears; an id without an entry makes the row unknown (only when kept)
        m = base.copy()
        m[:, 100] = self.special
        m[1::2, 100] = self.no_entry
        for keep in (False, True):
            self.add("stop_special_and_no_entry%s" % ("_kept" if keep else ""), m, stop=[self.special, self.no_entry], keep_stop=keep)
        # a row of nothing but stop ids, rows that alternate stop / no stop (every hit opens a run)
        m = base[:4].copy()
        m[0, :] = self.eos
        m[1, ::2] = self.eos
        m[2, 1::2] = self.eos
        self.add("stop_runs", m, [0, 1, 0, 0], None, stop=[self.eos])

    def window_edges(self):
        width, nr = 5000, 12
        m = self.known(nr, width)
        b = self._at_flat(width, nr, [7, 0, 511, 0, 2047, 0], 2048)
        e = np.minimum(self._at_flat(width, nr, [0, 7, 0, 511, 0, 2047], 2048) + 2048, width)
        self.add("window_begin_on_edges", m, b, None)
        self.add("window_end_on_edges", m, None, e)
        self.add("window_both_on_edges", m, b, e)
        self.add("window_equal", m, b, b)
        self.add("window_crossed", m, e, b)
        self.add("window_negative_and_beyond", m, -b - 1, e + width)
        self.add("window_all_outside", m, np.full(nr, width), np.full(nr, -3))
        rb, re = self.windows(nr, width)
        self.add("window_random", m, rb, re)

    def pads(self):
        nr, width = 9, 700
        body = self.known(nr, width, avoid=(self.eos, self.pad_valid))
        lp = self.rng.integers(0, width // 2, size=nr)
        rp = self.rng.integers(width // 2, width + 1, size=nr)
        lp[0], rp[0] = 0, width                                           # a row without pad
        lp[1], rp[1] = width, width                                       # all-pad rows (left fill / right fill)
        lp[2], rp[2] = 0, 0
        for pad, tag in ((-1, "minus_1"), (self.pad_valid, "valid_id")):
            m = body.copy()
            for r in range(nr):
                m[r, :lp[r]] = pad
                m[r, rp[r]:] = pad
            self.add("pad_%s_skipped" % tag, m, pad_id=pad, skip_pad=True)
            self.add("pad_%s_not_skipped" % tag, m, pad_id=pad)            # -1: every padded row is unknown
            self.add("pad_%s_skipped_with_end" % tag, m, None, rp, pad_id=pad, skip_pad=True)
        m = body.copy()                                                    # the pad is a stop id: the first pad ends the row
        for r in range(nr):
            m[r, :lp[r] // 4] = self.eos
            m[r, rp[r]:] = self.eos
        for keep in (False, True):
            self.add("pad_equals_stop%s" % ("_kept" if keep else ""), m, pad_id=self.eos, stop=[self.eos], skip_pad=True, keep_stop=keep)
        self.add("pad_equals_stop_window_behind_left_fill", m, lp // 4, None, pad_id=self.eos, stop=[self.eos], skip_pad=True)

    def unknowns(self):
        pool = self.h.bad_pool
        for width in (1, 3, 9, 600):
            nr = max(len(pool) + 6, rows_for(width) // 3)
            m = self.known(nr, width)
            for k, bad in enumerate(pool):                                 # the last column: the next row shares the lane's 8 cells
                m[(2 * k) % nr, width - 1] = bad
            self.add("unknown_last_column_w%d" % width, m)
            self.add("unknown_last_column_w%d_stop_and_pad" % width, m, pad_id=-1, stop=[self.eos], skip_pad=True)
        nr, width = 16, 40
        m = self.known(nr, width)
        b, e = np.full(nr, 10), np.full(nr, 30)
        for r, c in enumerate([0, 9, 10, 29, 30, 39, 20, 5]):              # inside [10, 30): rows 2, 3, 6
            m[r, c] = self.h.bad(1)[0]
        m[8, 35] = self.h.bad(1)[0]                                        # behind a stop: not decoded, not unknown
        m[8, 25] = self.eos
        m[9, 25] = self.h.bad(1)[0]                                        # before the stop: unknown
        m[9, 26] = self.eos
        self.add("unknown_inside_and_outside_window", m, b, e, stop=[self.eos])
        m = self.known(8, 50)
        valid = int(self.h.uniform(1)[0])
        m[1, 3] = 2 ** 32 + valid                                          # must not alias to `valid`
        m[2, 49] = 2 ** 32
        m[3, 0] = WIDE_BAD[0]
        m[4, 7] = WIDE_BAD[1]
        m[5, 8] = -2 ** 32 + valid
        m[6, 9] = 2 ** 31 + valid
        self.add("unknown_64_bit_values", m)
        self.add("unknown_64_bit_values_as_stop_and_pad", m, pad_id=WIDE_BAD[0], stop=[2 ** 32 + valid, WIDE_BAD[1]], skip_pad=True)

    def build(self):
        self.widths()
        self.stage_edge()
        self.stop_edges()
        self.window_edges()
        self.pads()
        self.unknowns()
        return self.cases


_cases = {}
_expected = {}


def cases(name):
    """The cases of one table (built once; nobody changes them)."""
    if name not in _cases:
        _cases[name] = _Builder(name, seed=7000 + TABLES.index(name)).build()
        for c in _cases[name]:
            for key in ("rows", "begin", "end"):
                if c[key] is not None:
                    c[key].setflags(write=False)
    return _cases[name]


def options(c):
    """The keyword arguments of a case for decode_rows_ref (and, by name, for Batch.decode_rows_host)."""
    return dict(begin=c["begin"], end=c["end"], pad_id=c["pad_id"], stop=c["stop"], skip_pad=c["skip_pad"], keep_stop=c["keep_stop"])


def expected(name):
    """{case name: decode_rows_ref's result} for one table, computed once."""
    if name not in _expected:
        tab = dc.table(name)
        _expected[name] = {c["name"]: decode_rows_ref.decode_rows_ref(tab, c["rows"], **options(c)) for c in cases(name)}
    return _expected[name]


def plain(c):
    """No window, no stop ids, no pad: the case decodes as the flat decode of its rows."""
    return c["begin"] is None and c["end"] is None and not c["stop"] and not c["skip_pad"]
