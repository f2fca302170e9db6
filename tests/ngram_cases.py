"""Cases of the n-gram set and overlap pass (jtk_ngram_set_*, jtk_batch_ngram_overlap) for the CPU tier
(tests/test_ngram_rules_cpu.py: the shim of the rule header against tests/ngram_ref.py) and the GPU tier
(tests/test_ngram_gpu.py).  Documents are built from words that are one cl100k_base token each behind a space
(minhash_cases.pool), so a document of l words has l tokens and positions are running sums; the tiers check that from the
oracle's own tokens (edges_reached works on the oracle's ids and the reference's result, never on the plan).

A case: name, n, seed, steps (how the set is built, in order), docs (the corpus, bytes), route (how the corpus is encoded).
A step is ("texts", docs, route) -- encoded and added as a batch -- or ("keys", ngrams) -- each entry a text of exactly n tokens
whose k goes in through add_keys, duplicates and all."""
import collections

import numpy as np

import minhash_cases as mc
import ngram_ref as nr

Case = collections.namedtuple("Case", "name n seed steps docs route")
_Enc = collections.namedtuple("_Enc", "name docs route")

TILE = 512                    # JTK_NG_TILE (the CPU tier checks both against the header)
LANE = 8                      # JTK_NG_LANE
T = TILE
MAX_SEED = (1 << 64) - 1
NGRAMS = (1, 2, 13, 32)
LIT = b"<|endoftext|>"

doc = mc.doc
batch = mc.batch


def oracle():
    return mc.oracle()


def ids_of(docs, route, keep_refused=False):
    """(ids per document, status per document) by the CPU oracle, as the encode of `route` leaves them.  keep_refused: a
    refused document keeps the tokens its text has as ordinary text -- the rule must not look at them."""
    ids, status = mc.expected_ids(_Enc("x", docs, route))
    if keep_refused:
        ids = [oracle().encode_ordinary(d.replace(b"\xff", b"")) if st < 0 else x for d, x, st in zip(docs, ids, status)]
    return [list(x) for x in ids], list(status)


_POOL_IDS = []


def _slot_words(seed, slot, capacity=64):
    """The pool's words whose 1-gram k has home slot `slot` in a table of `capacity`."""
    if not _POOL_IDS:
        _POOL_IDS.extend(oracle().encode_ordinary(w) for w in mc.pool())
    key = nr.key_of(seed, 1)
    return [w for w, ids in zip(mc.pool(), _POOL_IDS) if nr.k_of(ids, key) & (capacity - 1) == slot]


def wrap_seed():
    """The first seed under which four words of the pool share home slot 63 of 64 and two more share another."""
    for seed in range(1, 4000):
        if len(_slot_words(seed, 63)) >= 4 and len(_slot_words(seed, 20)) >= 2 and not _slot_words(seed, 21):
            return seed
    raise AssertionError("no seed gives the wrap-around words")


def cases():
    out = []
    # every length around n, the set built from the same documents
    for n in NGRAMS:
        docs = batch([0, 1, n - 1, n, n + 1, 0, 2 * n + 3, 1, n, 0], n)
        out.append(Case("lengths_n%d" % n, n, 0 if n in (1, 13) else MAX_SEED, [("texts", docs, "ordinary")], docs, "ordinary"))
    # the second document starts n + 2 tokens before the first tile edge and runs 2 n + 3 past it; all its n-grams are in the set
    for n in (2, 13, 32):
        docs = batch([T - n - 2, 3 * n + 5, 7], 40 + n)
        out.append(Case("straddle_n%d" % n, n, n, [("texts", docs[1:2], "ordinary")], docs, "ordinary"))
    for n in (2, 13):
        A, B, R = doc(n, 300 + n), doc(n, 310 + n), doc(2 * n + 2, 320 + n)
        f = lambda l, s: doc(l, 330 + n + s)
        docs = [f(T - 5, 0) + A + f(3, 1) + B + f(10, 2),              # A starts 5 tokens before the tile edge
                f(7, 3) + A + B + f(4, 4) + A + f(1, 5) + B + f(6, 6),  # hits n apart, then n + 1 apart
                f(9, 7) + R + f(9, 8),                                  # n + 3 starts in a row
                f(T - 40, 9), f(2 * n, 10) + A]                          # ... and A ends on a tile's last token region
        out.append(Case("patterns_n%d" % n, n, MAX_SEED, [("texts", [A, B], "ordinary"), ("texts", [R], "ordinary")], docs, "ordinary"))
    # document ends: halves of a set n-gram on either side of a tile edge that is a document end; whole ones at an end and a start
    n = 13
    A = doc(n, 400)
    A1, A2 = b"".join(mc.word(400, i) for i in range(6)), b"".join(mc.word(400, i) for i in range(6, n))
    docs = [doc(T - 6, 401) + A1, A2 + doc(20, 402) + A, A + doc(5, 403), doc(T - 2 * n - 50, 404), doc(4, 405) + A, A]
    out.append(Case("doc_ends", n, 5, [("texts", [A], "ordinary")], docs, "ordinary"))
    for r in (1, 2, 65):
        docs = batch([0] * r + [T] + [0] * r + [30] + [0] * r, 5)
        out.append(Case("empty_runs_%d" % r, 5, r, [("texts", [docs[2 * r + 1], docs[r][:60]], "ordinary")], docs, "ordinary"))
    # tokens 8 .. 1043 are one document: the middle tile is wholly inside it
    docs = batch([5, 3, 2 * T + 12, 4, 6], 6)
    out.append(Case("three_tiles_n13", 13, 0, [("texts", [docs[2], docs[0]], "ordinary")], docs, "ordinary"))
    out.append(Case("three_tiles_n1", 1, MAX_SEED, [("texts", [doc(40, 61)], "ordinary")], docs, "ordinary"))
    docs = batch([1, 2, 1, 0, 1, 1, 2, 0, 1, 1] * 60, 8)
    out.append(Case("many_short", 2, 8, [("texts", docs[:50], "ordinary")], docs, "ordinary"))
    docs = [doc(20, 90), doc(3, 91) + LIT + doc(2, 92), doc(7, 93), doc(3, 91) + doc(2, 92), doc(9, 94)]
    out.append(Case("refused_special", 2, 9, [("texts", docs, "encode")], docs, "encode"))
    docs = [doc(20, 95), doc(3, 96) + b"\xff" + doc(2, 97), doc(7, 98), doc(3, 96) + doc(2, 97), doc(9, 99)]
    out.append(Case("refused_utf8", 2, 9, [("texts", docs, "validate")], docs, "validate"))
    docs = [doc(10, 100) + LIT + doc(6, 101), LIT, doc(4, 102), b"<|fim_prefix|>" + doc(40, 103)]
    out.append(Case("allow_special", 2, 10, [("texts", [doc(3, 104) + LIT + doc(6, 101), docs[3]], "allow_special")], docs, "allow_special"))
    docs = batch([30, 8, 1, 0, 50] * 2, 11)
    out.append(Case("fim", 2, 11, [("texts", docs[:5], "fim")], docs, "fim"))
    # ---- the set's own edges, through add_keys with 1-grams chosen by their home slot
    seed = wrap_seed()
    w63, w20 = _slot_words(seed, 63), _slot_words(seed, 20)
    rest = [w for w in mc.pool() if w not in w63 and w not in w20]
    probe = b"".join(w63[:4] + w20[:2] + rest[:10])          # present and absent words of both chains, and unrelated ones
    # three keys with home slot 63 lie in 63, 0, 1; the fourth word of that slot is absent and walks 63, 0, 1 to the empty 2
    out.append(Case("set_wrap", 1, seed, [("keys", w63[:3])], [probe, doc(30, 500)], "ordinary"))
    # one key at slot 20; the absent second word of that slot passes it and ends at the empty 21
    out.append(Case("set_chain", 1, seed, [("keys", w20[:1] + rest[:3])], [probe], "ordinary"))
    out.append(Case("set_dups", 1, seed, [("keys", [w63[0], w63[0], rest[0]]), ("keys", [rest[0], rest[1], w63[0]])], [probe], "ordinary"))
    words = mc.pool()
    out.append(Case("set_grow_exact", 1, 0, [("keys", words[:32])], [doc(100, 501)], "ordinary"))               # 2 (0 + 32) = 64
    out.append(Case("set_grow_plus2", 1, 0, [("keys", words[:33])], [doc(100, 501)], "ordinary"))               # 2 (0 + 33) = 66
    out.append(Case("set_grow_second", 1, MAX_SEED, [("keys", words[:16]), ("keys", words[8:24]), ("keys", words[20:29])],
                    [doc(100, 502)], "ordinary"))                                 # 2 (16 + 16) = 64, then 2 (24 + 9) = 66
    out.append(Case("set_grow_batch", 2, 0, [("texts", [doc(17, 503)], "ordinary"), ("texts", [doc(18, 504)], "ordinary")],
                    [doc(17, 503) + doc(18, 504)], "ordinary"))                   # 16 n-grams, then 2 (16 + 17) = 66
    out.append(Case("set_empty", 13, 0, [], batch([0, 40, 3, T + 9], 505), "ordinary"))
    return out


def build_set(case, wrong=None):
    """The reference set of a case, and per step what goes in: ("batch", ids, status) or ("keys", list of k)."""
    s = nr.Set(case.seed, case.n)
    fed = []
    key = nr.key_of(case.seed, case.n)
    for kind, what, *route in case.steps:
        if kind == "texts":
            ids, status = ids_of(what, route[0], keep_refused=True)
            s.add_docs(ids, status, wrong)
            fed.append(("batch", ids, status))
        else:
            grams = [oracle().encode_ordinary(g) for g in what]
            assert all(len(g) == case.n for g in grams)
            ks = [nr.k_of(g, key, 0 if wrong == "id_not_plus_1" else 1) for g in grams]
            s.add_keys(ks)
            fed.append(("keys", ks))
    return s, fed


def all_edges():
    e = {("len", n, l) for n in NGRAMS for l in (0, 1, n - 1, n, n + 1)}
    e |= {("straddle", n, s) for n in (2, 13, 32) for s in range(1, n)}
    e |= {"cover_crosses_tile", "cover_crosses_lane", "start_on_tile_last", "start_n_minus_1_before_tile", "ends_on_tile_last",
          "starts_on_tile_first", "halves_no_hit", "whole_at_end_and_start", "three_tiles", "run_n_plus_3", "apart_n", "apart_n_plus_1"}
    e |= {(where, r) for where in ("empty_run_tile_first", "empty_run_start", "empty_run_end") for r in (1, 2, 65)}
    e |= {("refused", route, side) for route in ("encode", "validate") for side in ("source", "corpus")}
    e |= {("route", r) for r in ("allow_special", "fim")} | {("seed", 0), ("seed", MAX_SEED)}
    e |= {"wrap3", "absent_walks_wrapped_chain", "absent_passes_occupied", "present_not_at_home", "dups_within", "dups_across",
          "grow_exact", "grow_plus2", "grow_on_second_insert", "grow_by_batch", "empty_set"}
    return e


def _between(status, d):
    return 0 < d < len(status) - 1 and status[d] < 0 and status[d - 1] >= 0 and status[d + 1] >= 0


def edges_reached(case, ids, status, ngset, fed, res):
    """The edges a case reaches: from the oracle's ids of the corpus, the reference set and what fed it, and the reference's
    result `res` of the overlap."""
    got = {("seed", case.seed), ("route", case.route)}
    n = case.n
    lens = [len(x) for x in ids]
    off = res.tok_off.tolist()
    total, nd = off[-1], len(ids)
    flat = [t for x in ids for t in x]
    key = nr.key_of(case.seed, n)
    hit = [int(p) for p in np.flatnonzero(res.flags & nr.START)]
    hits = set(hit)
    for d, l in enumerate(lens):
        s, e = off[d], off[d + 1]
        if status[d] >= 0 and l in (0, 1, n - 1, n, n + 1):
            got.add(("len", n, l))
        if l == 0:
            continue
        if e % T == 0 and e < total:
            got.add("ends_on_tile_last")
        if s % T == 0 and s > 0:
            got.add("starts_on_tile_first")
        if (e - 1) // T - s // T >= 2 and s % T and e % T and e < total and res.n_hit[d] > 0:
            got.add("three_tiles")
        if d + 1 < nd and lens[d + 1] and status[d] >= 0 and status[d + 1] >= 0:
            for i in range(max(s, e - n + 1), e):
                if i + n <= off[d + 2] and nr.k_of(flat[i:i + n], key) in ngset.keys and i not in hits:
                    got.add("halves_no_hit")
            if l >= n and lens[d + 1] >= n and e - n in hits and e in hits:
                got.add("whole_at_end_and_start")
    for g in hit:
        if g // T != (g + n - 1) // T:
            got |= {"cover_crosses_tile", ("straddle", n, T - g % T)}
        if g // LANE != (g + n - 1) // LANE:
            got.add("cover_crosses_lane")
        if g % T == T - 1 and n > 1:
            got.add("start_on_tile_last")
        if g % T == T - n + 1 and n > 1:
            got.add("start_n_minus_1_before_tile")
        if all(g + j in hits for j in range(n + 3)):
            got.add("run_n_plus_3")
        if g + n in hits and not any(g + j in hits for j in range(1, n)):
            got.add("apart_n")
        if g + n + 1 in hits and not any(g + j in hits for j in range(1, n + 1)) and not res.flags[g + n] & nr.COVERED:
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
    for d in range(nd):
        if _between(status, d):
            got.add(("refused", case.route, "corpus"))
    for (kind, what, *route), f in zip(case.steps, fed):
        if f[0] == "batch" and any(_between(f[2], d) for d in range(len(f[2]))):
            got.add(("refused", route[0], "source"))
    # the set
    C = ngset.capacity
    table = ngset.table()
    if not ngset.keys:
        got.add("empty_set")
    if sum(1 for k in ngset.keys if k & (C - 1) == C - 1) >= 3:
        got.add("wrap3")
    for k in {nr.k_of(flat[i:i + n], key) for d in range(nd) if status[d] >= 0 for i in range(off[d], off[d + 1] - n + 1)}:
        home = k & (C - 1)
        if k in ngset.keys:
            if table[home] != k:
                got.add("present_not_at_home")
        elif table[home]:
            got.add("absent_passes_occupied")
            walk = home
            while table[walk]:
                walk = (walk + 1) & (C - 1)
            if walk < home:
                got.add("absent_walks_wrapped_chain")
    c, cap, seen = 0, nr.MIN_CAPACITY, set()
    for i, f in enumerate(fed):
        ks = f[1] if f[0] == "keys" else nr.doc_keys(f[1], f[2], case.seed, n)
        if f[0] == "keys":
            if len(set(ks)) < len(ks):
                got.add("dups_within")
            if seen & set(ks):
                got.add("dups_across")
        need = 2 * (c + len(ks))
        if need == cap:
            got.add("grow_exact")
        if need == cap + 2:
            got |= {"grow_plus2"} | ({"grow_on_second_insert"} if i else set()) | ({"grow_by_batch"} if f[0] == "batch" else set())
        cap = max(cap, nr.capacity(c, len(ks)))
        seen |= set(ks)
        c = len(seen)
    assert cap == ngset.capacity and c == len(ngset.keys)
    return got
