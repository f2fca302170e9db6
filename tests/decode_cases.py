"""Seeded inputs for batch decode, built for the edges of jtk_decode.hip: shared by tests/test_decode_ref_cpu.py (reference ==
CPU oracle, and the coverage conditions on these inputs) and tests/test_decode_gpu.py (device == reference).

A case is (name, ids int32[], seq_off int64[]).  T = tokens per tile (JTK_DEC_TILE); a tile whose bytes exceed S (DSTAGE) is
written straight to global memory ("direct"), any other is assembled in LDS and stored as aligned words ("staged").  Ids are
picked by byte length from the table under test (decode_ref.DecodeTable), never hard-coded.
"""
import os

import numpy as np

import decode_ref
import oracle_lib

T = 2048
S = 16384
TABLES = ["cl100k_base", "r50k_base", "p50k_base", "p50k_edit", "custom"]
FUZZ_ROUNDS = 20

_CUSTOM_TEXT = (b"the quick brown fox jumps over the lazy dog while seven wizards quietly judge the boxing match and then "
                b"the five dozen liquor jugs are packed into my box with care for the journey over the quiet brown hills ") * 20


def custom_spec():
    """(kind, ranks, specials) of the custom encoding: a tiny trained table; specials far above it, so that real holes lie
    between them, with literals of 1 and of 300 bytes (longer than any table token)."""
    from test_gpu_parity import _train_tiny_bpe
    ranks = _train_tiny_bpe(_CUSTOM_TEXT, 300)
    specials = {"~": len(ranks) + 1000, "<|" + "x" * 296 + "|>": 2 ** 20 + 3}
    return 1, ranks, specials


_tables = {}


def table(name):
    """The reference's table for one of TABLES."""
    if name not in _tables:
        if name == "custom":
            _, ranks, specials = custom_spec()
            _tables[name] = decode_ref.DecodeTable(ranks, specials)
        else:
            cfg = oracle_lib.ENCODINGS[name]
            _tables[name] = decode_ref.DecodeTable.from_tiktoken(os.path.join(oracle_lib.DATA_DIR, cfg["file"]), cfg["specials"])
    return _tables[name]


class _Builder:
    def __init__(self, tab, seed):
        self.tab = tab
        self.rng = np.random.default_rng(seed)
        self.by = tab.ids_by_length()
        self.avail = np.array(sorted(self.by), dtype=np.int64)
        self.lmax = int(self.avail[-1])
        self.known = np.array(sorted(tab.table), dtype=np.int64)
        n = tab.n_ids_table
        holes = tab.holes()
        if len(holes) > 40:
            holes = self.rng.choice(holes, size=40, replace=False)
        self.bad_pool = np.array([-1, -2, -2 ** 31, 2 ** 31 - 1, n, n + 1, n + 12345] + holes.tolist(), dtype=np.int64)
        self.cases = []
        self.names = set()

    # ---- pieces --------------------------------------------------------------------------------------
    def add(self, name, ids, seq_off=None):
        ids = np.asarray(ids, dtype=np.int64)
        if seq_off is None:
            seq_off = [0, len(ids)]
        seq_off = np.asarray(seq_off, dtype=np.int64)
        assert name not in self.names and seq_off[0] == 0 and seq_off[-1] == len(ids) and (np.diff(seq_off) >= 0).all(), name
        self.names.add(name)
        self.cases.append((name, ids.astype(np.int32), seq_off))

    def bad(self, n):
        return self.rng.choice(self.bad_pool, size=n)

    def uniform(self, n):
        """ids drawn uniformly over every id that has an entry."""
        return self.rng.choice(self.known, size=n)

    def ids_of_lengths(self, lens):
        out = np.empty(len(lens), dtype=np.int64)
        for l in np.unique(lens):
            at = np.flatnonzero(lens == l)
            out[at] = self.rng.choice(self.by[int(l)], size=len(at))
        return out

    def _fill(self, n, total):
        """n lengths with the given sum: as many of the longest as fit, the rest 1 byte."""
        lens = np.ones(n, dtype=np.int64)
        extra, i = total - n, 0
        while extra > 0:
            l = int(self.avail[self.avail - 1 <= extra][-1])
            assert i < n and l >= 2, (n, total)
            lens[i] = l
            extra -= l - 1
            i += 1
        return lens

    def lens_with_sum(self, n, total):
        assert n <= total <= n * self.lmax, (n, total)
        m = n // 2
        while True:                                                       # a random half, the other half makes the sum exact
            cand = self.avail[self.avail <= max(2.0 * total / n, 2.0)]
            head = self.rng.choice(cand, size=m) if m else np.zeros(0, dtype=np.int64)
            rest_n, rest = n - m, total - int(head.sum())
            if rest_n <= rest <= rest_n * self.lmax - self.lmax:
                break
            if m == 0:
                rest_n, rest, head = n, total, np.zeros(0, dtype=np.int64)
                break
            m //= 2
        lens = np.concatenate([head, self._fill(rest_n, rest)])
        self.rng.shuffle(lens)
        assert len(lens) == n and lens.sum() == total
        return lens

    def tile(self, total, n=T):
        """n ids that all have an entry, their bytes summing to exactly `total`."""
        return self.ids_of_lengths(self.lens_with_sum(n, total))

    def small_tile(self, k):
        """A full tile of k bytes: one or two real tokens, every other id without an entry."""
        ids = self.bad(T)
        lens = [] if k == 0 else [1] if k == 1 else [1, k - 1]
        at = np.sort(self.rng.choice(T, size=len(lens), replace=False))
        ids[at] = self.ids_of_lengths(np.array(lens, dtype=np.int64))
        return ids

    def seqs(self, n, mean=30):
        """Random sequence offsets over n tokens: about one empty in five, now and then a long one."""
        off = [0]
        while off[-1] < n:
            u = self.rng.random()
            l = 0 if u < 0.2 else int(self.rng.integers(1, 3 * T)) if u < 0.22 else int(self.rng.geometric(1.0 / mean))
            off.append(min(n, off[-1] + l))
        while self.rng.random() < 0.3:
            off.append(n)
        return np.array(off, dtype=np.int64)

    def add_tiles(self, name, tiles):
        ids = np.concatenate(tiles)
        self.add(name, ids, self.seqs(len(ids)))

    # ---- the case families ----------------------------------------------------------------------------
    def token_counts(self):
        for n in (0, 1, 7, 8, 9, 63, 64, 65, T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1, 3 * T + 5):
            ids = self.uniform(n)
            self.add("count_%d_one_seq" % n, ids)
            self.add("count_%d_short_seqs" % n, ids, self.seqs(n, mean=5))

    def stage_edge(self):
        st, d = 9000, S + 7
        totals = [S - 1, S, S + 1, T * self.lmax] + ([T * 128] if self.lmax != 128 else [])
        for x in totals:
            self.add_tiles("stage_%d_first" % x, [self.tile(x), self.tile(st)])
            self.add_tiles("stage_%d_between_staged" % x, [self.tile(st), self.tile(x), self.tile(st + 1)])
            self.add_tiles("stage_%d_between_direct" % x, [self.tile(d), self.tile(x), self.tile(d + 2)])
            if 1500 <= x <= 1500 * self.lmax:
                self.add_tiles("stage_%d_last_partial" % x, [self.tile(st), self.tile(x, 1500)])
        self.add_tiles("stage_direct_then_single_token", [self.tile(d), self.uniform(1)])

    def word_alignment(self):
        """Every pair (obase mod 4, (obase + total) mod 4) of the tile under test, set through the byte sum of the tile
        before it; S, 7000, 8000 and 9000 are multiples of 4."""
        for r0 in range(4):
            for r1 in range(4):
                dlt = (r1 - r0) % 4
                tag = "_%d_%d" % (r0, r1)
                direct = S + 1 + (dlt - 1) % 4                            # S+1 .. S+4, == dlt mod 4
                self.add_tiles("align_plain_staged" + tag, [self.tile(9000 + r0), self.tile(7000 + dlt), self.tile(8000)])
                self.add_tiles("align_direct_between_staged" + tag, [self.tile(9000 + r0), self.tile(direct), self.tile(8000)])
                self.add_tiles("align_direct_last_partial" + tag, [self.tile(9000 + r0), self.tile(direct, 1500)])
                self.add_tiles("align_staged_between_direct" + tag,
                               [self.tile(S + 1 + (r0 - 1) % 4), self.tile(S - 3 + (dlt - 1) % 4), self.tile(S + 5)])
                if r0 == 0:
                    self.add_tiles("align_direct_first" + tag, [self.tile(direct), self.tile(8000)])
        for k in range(6):                                                # its bytes lie inside words the neighbours also write
            for r0 in range(4):
                self.add_tiles("small_tile_%d_bytes_at_%d" % (k, r0), [self.tile(9000 + r0), self.small_tile(k), self.tile(8000)])
            self.add_tiles("small_tile_%d_bytes_between_direct" % k, [self.tile(S + 1 + k), self.small_tile(k), self.tile(S + 9)])
        self.add_tiles("last_tile_single_token", [self.tile(9001), self.tile(8003), self.uniform(1)])

    def with_empty_run(self, off, p, run):
        """Offsets `off` with a start at p followed by `run` empty sequences there."""
        off = sorted(set(off.tolist()) | {p})
        i = off.index(p)
        return np.array(off[:i + 1] + [p] * run + off[i + 1:], dtype=np.int64)

    def sequence_boundaries(self):
        n = 3 * T + 5
        ids = self.uniform(n)
        starts = {0, n}
        for k in (1, 2, 3):
            starts |= {k * T - 1, k * T, k * T + 1}
        for j in range(1, n // 64, 5):
            starts |= {64 * j - 1, 64 * j, 64 * j + 1}
        for j in range(1, n // 8, 7):
            starts |= {8 * j - 1, 8 * j, 8 * j + 1}
        self.add("starts_at_tile_word_lane_edges", ids, sorted(s for s in starts if 0 <= s <= n))
        self.add("starts_at_every_lane_edge", ids, sorted({0, n} | {8 * j + d for j in range(1, n // 8) for d in (-1, 0, 1)}))
        n = T + 100
        ids = self.uniform(n)
        places = (("token_0", 0), ("tile_edge", T), ("mask_word_edge", 64 * 5), ("mid_lane", 8 * 3 + 3), ("n_tok", n))
        for run in (1, 2, 65):
            for what, p in places:
                self.add("empty_run_%d_at_%s" % (run, what), ids, self.with_empty_run(self.seqs(n), p, run))
            off = self.seqs(n)
            for _, p in places:
                off = self.with_empty_run(off, p, run)
            self.add("empty_run_%d_everywhere" % run, ids, off)
        self.add("no_ids_no_seqs", [], [0])
        self.add("no_ids_1_seq", [], [0, 0])
        self.add("no_ids_300_seqs", [], [0] * 301)
        for ns in (255, 256, 257):
            cuts = np.sort(self.rng.integers(0, 301, size=ns - 1))
            self.add("n_seqs_%d" % ns, self.uniform(300), np.concatenate([[0], cuts, [300]]))
        self.add("one_seq_per_token", self.uniform(T + 10), np.arange(T + 11))

    def id_classes(self):
        tab = self.tab
        n = tab.n_ids_table
        classes = [0, tab.n_table - 1] + sorted(tab.specials) + [n, n + 1, 2 ** 31 - 1, -1, -2 ** 31] + tab.holes()[:3].tolist()
        seqs = []
        for c in classes:
            k = self.uniform(4).tolist()
            seqs += [[c], [k[0], c, k[1]], [c, k[2]], [k[3], c]]
        b = self.bad(8).tolist()
        k = self.uniform(8).tolist()
        seqs += [[b[0], k[0], k[1]], [k[2], b[1], k[3]], [k[4], k[5], b[2]], [b[3], b[4], b[5]], [], [b[6]], [k[6]]]
        off = np.concatenate([[0], np.cumsum([len(s) for s in seqs])])
        self.add("id_classes", [i for s in seqs for i in s], off)
        for with_start in (False, True):                                  # across a tile edge; a start on the edge moves the blame
            for a, b2 in ((True, False), (False, True), (True, True)):
                ids = self.uniform(2 * T)
                if a:
                    ids[T - 1] = self.bad(1)[0]
                if b2:
                    ids[T] = self.bad(1)[0]
                off = sorted(set(self.seqs(2 * T).tolist()) - {T - 1, T, T + 1} | ({T} if with_start else set()))
                self.add("unknown_at_tile_edge_%d%d_%s" % (a, b2, "start" if with_start else "inside"), ids, off)
        n = T + 100
        for run in (1, 2, 65):                                            # beside a run of empties on the same token index
            for what, p in (("mid_lane", 8 * 3 + 3), ("tile_edge", T), ("mask_word_edge", 64 * 5)):
                for side in ("before", "after", "both"):
                    ids = self.uniform(n)
                    if side != "after":
                        ids[p - 1] = self.bad(1)[0]
                    if side != "before":
                        ids[p] = self.bad(1)[0]
                    off = set(self.seqs(n).tolist()) - {p - 1, p + 1}     # (the neighbours hold more than the one id)
                    off = self.with_empty_run(np.array(sorted(off)), p, run)
                    self.add("unknown_%s_empty_run_%d_at_%s" % (side, run, what), ids, off)
        self.add_tiles("tile_of_unknown_ids", [self.tile(9002), self.bad(T), self.tile(8001)])
        self.add("only_unknown_ids", self.bad(T + 3), self.seqs(T + 3, mean=5))

    def fuzz(self):
        n = self.tab.n_ids_table
        for r in range(FUZZ_ROUNDS):
            cnt = int(self.rng.integers(1, 3 * T + 1))
            ids = self.rng.integers(-2, n + 2, size=cnt)
            if r % 2:                                                     # (4 ids in 100,000 have no entry: make them common)
                at = self.rng.random(cnt) < 0.01
                ids[at] = self.rng.choice([-2, -1, n, n + 1], size=int(at.sum()))
            self.add("fuzz_%d" % r, ids, self.seqs(cnt))

    def build(self):
        self.token_counts()
        self.stage_edge()
        self.word_alignment()
        self.sequence_boundaries()
        self.id_classes()
        self.fuzz()
        return self.cases


_cases = {}
_expected = {}


def cases(name):
    """The cases of one table (built once; nobody changes them)."""
    if name not in _cases:
        _cases[name] = _Builder(table(name), seed=1000 + TABLES.index(name)).build()
        for _, ids, seq_off in _cases[name]:
            ids.setflags(write=False)
            seq_off.setflags(write=False)
    return _cases[name]


def expected(name):
    """{case name: decode_ref's (out bytes, byte_off, status)} for one table, computed once."""
    if name not in _expected:
        tab = table(name)
        _expected[name] = {c[0]: tab.decode_ref(c[1], c[2]) for c in cases(name)}
    return _expected[name]


def is_fuzz(case_name):
    return case_name.startswith("fuzz_")
