"""Cases of the repeated-n-gram pass (jtk_batch_ngram_repeats) for the CPU tier (tests/test_repeat_rules_cpu.py: the shim of the
rule header against tests/repeat_ref.py) and the GPU tier (tests/test_repeat_gpu.py).  Documents are built from words that are
one cl100k_base token each behind a space (minhash_cases.pool), so a document of l words has l tokens and positions are running
sums; the tiers check that from the oracle's own tokens (edges_reached works on the oracle's ids and the reference's results,
never on the plan).  No case has more than about 4,500 tokens.

A case: name, n, seed, base (doc_index_base), docs (bytes), route (how the batch is encoded).  Every case is run in both modes.
"A later occurrence in a tile that is walked first" needs no case of its own: the CPU tier walks every case with the tiles
descending, which puts the later occurrence of every cross-tile repeat first."""
import collections

import numpy as np

import minhash_cases as mc
import repeat_ref as rr

Case = collections.namedtuple("Case", "name n seed base docs route")
_Enc = collections.namedtuple("_Enc", "name docs route")

TILE = 512                    # JTK_NG_TILE (the CPU tier checks these against the header)
LANE = 8                      # JTK_NG_LANE
WG = 2048                     # JTK_NG_TILE * JTK_NG_BLOCK_TILES
T = TILE
MAX_SEED = (1 << 64) - 1
WRAP_BASE = (1 << 64) - 3     # base + d wraps for d >= 3
NGRAMS = (1, 2, 13, 32)
MIN_BUDGET = 64 * 20          # JTK_RP_MIN_TABLE_BYTES
LIT = b"<|endoftext|>"

doc = mc.doc
batch = mc.batch


def oracle():
    return mc.oracle()


def words(idx):
    """The pool's words of these indices, joined."""
    return b"".join(mc.pool()[i % 200] for i in idx)


def ids_of(docs, route, keep_refused=False):
    """(ids per document, status per document) by the CPU oracle, as the encode of `route` leaves them.  keep_refused: a
    refused document keeps the tokens its text has as ordinary text -- the rule must not look at them."""
    ids, status = mc.expected_ids(_Enc("x", docs, route))
    if keep_refused:
        ids = [oracle().encode_ordinary(d.replace(b"\xff", b"").replace(LIT, b"")) if st < 0 else x for d, x, st in zip(docs, ids, status)]
    return [list(x) for x in ids], list(status)


def planted(length, salt, plants):
    """A document of `length` words of filler with phrases (bytes of whole words, 3 bytes each) put at the given positions."""
    w = [mc.word(salt, i) for i in range(length)]
    for at, phrase in plants:
        ph = [phrase[k:k + 3] for k in range(0, len(phrase), 3)]
        assert at >= 0 and at + len(ph) <= length
        w[at:at + len(ph)] = ph
    return b"".join(w)


_POOL_IDS = []


def _slot_words(seed, base, slot, capacity=64):
    """The pool's words whose 1-gram k, in document 0, has home slot `slot` in a table of `capacity`."""
    if not _POOL_IDS:
        _POOL_IDS.extend(oracle().encode_ordinary(w) for w in mc.pool())
    kd = rr.doc_key(rr.key_of(seed, 1), base, 0)
    return [w for w, ids in zip(mc.pool(), _POOL_IDS) if rr.k_of(ids, kd) & (capacity - 1) == slot]


def wrap_seed(base):
    """The first seed under which three words of the pool share home slot 63 of 64 in document 0."""
    for seed in range(1, 4000):
        if len(_slot_words(seed, base, 63)) >= 3:
            return seed
    raise AssertionError("no seed gives the wrap-around words")


def _placement(n):
    """Documents at tokens 0 .. 1899, 1900 .. 4299 and 4300 .. 4319; the middle one crosses the workgroup edges 2048 and 4096."""
    ph = [words(range(20 + 33 * k, 20 + 33 * k + n)) for k in range(6)]
    at = lambda a: a - 1900
    plants = [(at(1950), ph[0]), (at(1966), ph[0]), (at(4200), ph[0]),          # first in an earlier lane, in an earlier workgroup
              (at(2100), ph[1]), (at(2700), ph[1]),                              # first in an earlier tile of the same workgroup
              (at(2300), ph[2]), (at(2559), ph[2]),                              # a start on a tile's last token
              (at(2330), ph[3]), (at(3072 - (n - 1)), ph[3]),                    # a start n - 1 before a tile
              (at(3200), ph[4]), (at(3200 + n), ph[4]),                          # n apart
              (at(3300), ph[5]), (at(3300 + n + 1), ph[5])]                      # n + 1 apart
    return [doc(1900, 60 + n), planted(2400, 61 + n, plants), doc(20, 62 + n)]


def cases():
    out = []
    bases = {1: 0, 2: 5, 13: WRAP_BASE, 32: 0}
    for n in NGRAMS:
        docs = batch([0, 1, n - 1, n, n + 1, 0, 2 * n + 3, 1, n, 0], n)
        out.append(Case("lengths_n%d" % n, n, 0 if n in (1, 13) else MAX_SEED, bases[n], docs, "ordinary"))
    for n in NGRAMS:
        w = mc.pool()[3]
        out.append(Case("all_equal_n%d" % n, n, n, bases[n], [w * (n + 1), doc(5, 1), w * 40, w * (n + 64), doc(3, 2)], "ordinary"))
    a, b, c = mc.pool()[5], mc.pool()[6], mc.pool()[7]
    for n in (2, 3, 13):
        out.append(Case("periods_n%d" % n, n, MAX_SEED if n == 3 else 7, 5, [(a + b) * 3, (a + b) * 20, (a + b + c) * 15, (a + b + c) * 2, (a + b) * 66],
                        "ordinary"))
    A, X = words(range(10, 15)), words(range(20, 23))
    out.append(Case("same_across_docs_n2", 2, 3, 0, [A, A, X, X, words([30, 31, 32, 33]) + A[:6], A[:6] + words([34, 35, 36])], "ordinary"))
    A = words(range(10, 26))
    out.append(Case("same_across_docs_n13", 13, 3, WRAP_BASE, [A, A, doc(7, 53) + A[:39], A[:39] + doc(2, 54)], "ordinary"))
    out.append(Case("straddle_n2", 2, 4, 0, [words([40, 41, 42, 43, 44, 40]), words([41, 45, 46]), words([47, 48])], "ordinary"))
    B = words(range(50, 63))
    out.append(Case("straddle_n13", 13, 4, 5, [B + words(range(70, 75)) + B[:18], B[18:] + words(range(80, 84)), doc(3, 55)], "ordinary"))
    for n in (2, 13):
        out.append(Case("placement_n%d" % n, n, MAX_SEED if n == 2 else 0, 5 if n == 2 else 0, _placement(n), "ordinary"))
    for n in (2, 13):
        P, Q = words(range(50, 50 + n)), words(range(90, 90 + n))
        d1 = words([100, 101, 102]) + P + words([103, 104]) + P + words([105, 106, 107])
        l1 = 8 + 2 * n
        d2 = Q + words([108]) + Q + words([109, 110]) + Q + words([111])
        out.append(Case("top_edges_n%d" % n, n, 6, 0, [doc(T - 4, 70), d1, doc(2 * T - (T - 4) - l1, 71), d2], "ordinary"))
    P = words(range(120, 125))
    for r in (1, 2, 65):
        docs = [b""] * r + [doc(T - 10, 72 + r) + P + P] + [b""] * r + [P + doc(20, 73 + r) + P] + [b""] * r
        out.append(Case("empty_runs_%d" % r, 5, r, r, docs, "ordinary"))
    A = words(range(130, 136))
    out.append(Case("refused_special", 2, 9, 0, [A + A, A + LIT + A, A + doc(3, 91) + A, doc(9, 94)], "encode"))
    out.append(Case("refused_utf8", 2, 9, 5, [A + A, A + b"\xff" + A, A + doc(3, 96) + A, doc(9, 99)], "validate"))
    docs = [doc(10, 100) + LIT + doc(6, 101) + LIT + doc(10, 100), LIT + LIT + LIT, doc(4, 102), b"<|fim_prefix|>" + doc(20, 103) + doc(20, 103)]
    out.append(Case("allow_special", 2, 10, 0, docs, "allow_special"))
    docs = [doc(l // 2, 140 + d) * 2 + doc(l % 2, 150 + d) for d, l in enumerate([30, 8, 1, 0, 50] * 2)]
    out.append(Case("fim", 2, 11, 0, docs, "fim"))
    # ---- the table, through 1-grams chosen by their home slot in document 0
    seed = wrap_seed(5)
    w63 = _slot_words(seed, 5, 63)
    rest = [w for w in mc.pool() if w not in w63]
    out.append(Case("table_wrap", 1, seed, 5, [b"".join(w63[:3] + rest[:4] + w63[:2] + rest[2:6] + w63[2:3])], "ordinary"))
    out.append(Case("table_cap_exact", 1, 0, 0, [words(list(range(16)) * 2)], "ordinary"))                       # m = 32: 2 m = 64
    out.append(Case("table_cap_plus2", 1, 0, 0, [words(list(range(16)) * 2 + [3])], "ordinary"))                 # m = 33: 2 m = 66
    # ---- the groups under the smallest budget (at most 32 n-grams share a table): boundaries at tokens 14, 120, ...
    lens = [5, 9, 0, 100, 0, 0, 100, 7, 3, 40, 0, 12, 6, 6, 6, 300, 11, 0]
    docs = [doc(l // 2, 160 + d) * 2 + doc(l % 2, 180 + d) for d, l in enumerate(lens)]
    out.append(Case("grouping_n2", 2, 12, WRAP_BASE, docs, "ordinary"))
    out.append(Case("grouping_n13", 13, 12, 0, docs, "ordinary"))
    return out


def all_edges():
    e = {("len", n, l) for n in NGRAMS for l in (0, 1, n - 1, n, n + 1, 2 * n + 3)}
    e |= {("all_equal", "n+1"), ("all_equal", 40), "lane_run_merge", "period2", "period3"}
    e |= {"same_gram_adjacent_docs", "same_gram_docs_in_one_lane", "end_of_d_is_start_of_d1", "straddle_equals_in_doc"}
    e |= {"first_in_earlier_lane", "first_in_earlier_tile", "first_in_earlier_workgroup", "doc_crosses_two_workgroup_edges"}
    e |= {"start_on_tile_last", "start_n_minus_1_before_tile", "cover_crosses_tile", "cover_crosses_lane", "apart_n", "apart_n_plus_1"}
    e |= {("count", 2), ("count", 3), ("count", 65), "top_tie", "top_first_on_tile_first", "top_first_on_tile_last"}
    e |= {(where, r) for where in ("empty_run_tile_first", "empty_run_start", "empty_run_end") for r in (1, 2, 65)}
    e |= {("refused", "encode"), ("refused", "validate"), ("route", "allow_special"), ("route", "fim")}
    e |= {("seed", 0), ("seed", MAX_SEED), ("base", 0), ("base", 5), ("base", WRAP_BASE)}
    e |= {"chain_wraps", "key_not_at_home", "cap_exact", "cap_plus2"}
    e |= {"group_boundary_in_tile", "group_boundary_in_lane", "group_single_over_budget", "group_only_empty"}
    return e


def edges_reached(case, ids, status, later, marked):
    """The edges a case reaches: from the oracle's ids (a refused document with the tokens it would have as ordinary text) and the
    reference's results in the two modes (`later`: only later occurrences start; `marked`: JTK_REPEAT_MARK_FIRST)."""
    got = {("seed", case.seed), ("base", case.base), ("route", case.route)}
    n = case.n
    lens = [len(x) for x in ids]
    off = later.tok_off.tolist()
    total, nd = off[-1], len(ids)
    flat = [t for x in ids for t in x]
    ok = [status[d] >= 0 for d in range(nd)]
    grams = [[tuple(x[i:i + n]) for i in range(len(x) - n + 1)] if ok[d] else [] for d, x in enumerate(ids)]
    hit = [int(p) for p in np.flatnonzero(later.flags & rr.START)]
    mhits = set(int(p) for p in np.flatnonzero(marked.flags & rr.START))
    doc_of = np.repeat(np.arange(nd), lens).tolist()
    for d, l in enumerate(lens):
        s, e = off[d], off[d + 1]
        x = ids[d]
        if ok[d] and l in (0, 1, n - 1, n, n + 1, 2 * n + 3):
            got.add(("len", n, l))
        if not ok[d] and 0 < d < nd - 1 and ok[d - 1] and ok[d + 1] and len(set(grams_of(x, n))) < len(grams_of(x, n)) \
                and set(grams_of(x, n)) & set(grams[d - 1]):
            got.add(("refused", case.route))
        if l == 0 or not ok[d]:
            continue
        if len(set(x)) == 1 and l == n + 1:
            got.add(("all_equal", "n+1"))
        if len(set(x)) == 1 and l == 40:
            got.add(("all_equal", 40))
        for period in (2, 3):
            if l >= 2 * period and len(set(x[:period])) == period and all(x[i] == x[i + period] for i in range(l - period)):
                got.add("period%d" % period)
        if s // WG + 2 <= (e - 1) // WG:
            got.add("doc_crosses_two_workgroup_edges")
        for i in range(len(grams[d]) - 1):
            if grams[d][i] == grams[d][i + 1] and (s + i) // LANE == (s + i + 1) // LANE:
                got.add("lane_run_merge")
        counts = {int(c) for c in later.count[s:e]}
        got |= {("count", c) for c in (2, 3, 65) if c in counts}
        if later.top_count[d] >= 2:
            firsts = {int(later.first[s + i]) for i in range(len(grams[d])) if later.count[s + i] == later.top_count[d]}
            if len(firsts) >= 2:
                got.add("top_tie")
            at = s + int(later.top_first[d])
            if at % T == 0 and at > 0:
                got.add("top_first_on_tile_first")
            if at % T == T - 1:
                got.add("top_first_on_tile_last")
        if d + 1 < nd and lens[d + 1] and ok[d + 1]:
            once = lambda g, q: grams[q].count(g) == 1
            for g in set(grams[d]) & set(grams[d + 1]):
                if once(g, d) and once(g, d + 1):
                    p, q = s + grams[d].index(g), e + grams[d + 1].index(g)
                    if p not in mhits and q not in mhits:
                        got.add("same_gram_adjacent_docs")
                        if p // LANE == q // LANE:
                            got.add("same_gram_docs_in_one_lane")
            if l >= n and lens[d + 1] >= n and tuple(x[-n:]) == tuple(ids[d + 1][:n]) and e - n not in mhits and e not in mhits:
                got.add("end_of_d_is_start_of_d1")
            for i in range(max(s, e - n + 1), e):
                if i + n <= off[d + 2] and (tuple(flat[i:i + n]) in grams[d] or tuple(flat[i:i + n]) in grams[d + 1]):
                    got.add("straddle_equals_in_doc")
    hits = set(hit)
    for g in hit:
        d = doc_of[g]
        f = off[d] + int(later.first[g])
        if f // T == g // T and f // LANE != g // LANE:
            got.add("first_in_earlier_lane")
        if f // WG == g // WG and f // T != g // T:
            got.add("first_in_earlier_tile")
        if f // WG != g // WG:
            got.add("first_in_earlier_workgroup")
        if n > 1:
            if g // T != (g + n - 1) // T:
                got.add("cover_crosses_tile")
            if g // LANE != (g + n - 1) // LANE:
                got.add("cover_crosses_lane")
            if g % T == T - 1:
                got.add("start_on_tile_last")
            if g % T == T - n + 1:
                got.add("start_n_minus_1_before_tile")
    for g in mhits:
        if g + n in mhits and not any(g + j in mhits for j in range(1, n)):
            got.add("apart_n")
        if g + n + 1 in mhits and not any(g + j in mhits for j in range(1, n + 1)) and not marked.flags[g + n] & rr.COVERED:
            got.add("apart_n_plus_1")
    d = 0
    while d < nd:
        if lens[d]:
            d += 1
            continue
        first = d
        while d < nd and lens[d] == 0:
            d += 1
        r, p = d - first, off[first]
        if first == 0:
            got.add(("empty_run_start", r))
        elif d == nd:
            got.add(("empty_run_end", r))
        elif p % T == 0 and 0 < p < total:
            got.add(("empty_run_tile_first", r))
    # the table of the whole batch as one group
    ks = [k for here in rr.doc_ks(ids, status, n, case.seed, case.base) for _, k in here]
    m, cap = len(ks), rr.capacity(len(ks))
    homes = collections.Counter(k & (cap - 1) for k in set(ks))
    if homes[cap - 1] >= 2:
        got.add("chain_wraps")
    if any(c >= 2 for c in homes.values()):
        got.add("key_not_at_home")
    if m >= 32 and 2 * m == cap:
        got.add("cap_exact")
    if cap > 64 and 2 * m == cap // 2 + 2:
        got.add("cap_plus2")
    # the groups under the smallest budget
    for d0, d1, gm in rr.groups(lens, status, n, MIN_BUDGET):
        p = off[d1]
        if 0 < p < total and off[d0] < p:
            if p % T:
                got.add("group_boundary_in_tile")
            if p % LANE:
                got.add("group_boundary_in_lane")
        if d1 - d0 == 1 and rr.capacity(gm) * rr.SLOT_BYTES > MIN_BUDGET:
            got.add("group_single_over_budget")
        if off[d1] == off[d0]:
            got.add("group_only_empty")
    return got


def grams_of(x, n):
    return [tuple(x[i:i + n]) for i in range(len(x) - n + 1)]
