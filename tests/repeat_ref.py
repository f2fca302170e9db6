"""Repeated token n-grams inside a document (jtk_batch_ngram_repeats), written out from the rule's text alone -- nothing here is
shared with jtokkit_amd/csrc/jtk_repeat_rules.h.  Python integers and one Python dict per document; flags and per-document
results by their definitions, never by the kernels' tile walk or their table.  Documents are lists of token ids (the CPU
oracle's) with a status each; a refused document (status < 0) has no n-grams whatever tokens it is given.

wrong=: a deliberately wrong rule, for the CPU tier's check that the case set tells the right rule from wrong ones."""
import numpy as np

M64 = (1 << 64) - 1
G = 0x9E3779B97F4A7C15
START, COVERED = 1, 2
MARK_FIRST = 1
MIN_CAPACITY = 64
SLOT_BYTES = 20
WRONG_RULES = ("no_doc_salt", "first_is_last", "mark_first_swapped", "cross_doc_end", "refused_hashed", "covers_n_minus_1", "halo_dropped",
               "top_tie_takes_last", "count_minus_one", "base_ignored")


def mix(x):
    """The splitmix64 finaliser, on a Python integer."""
    x &= M64
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & M64
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & M64
    x ^= x >> 31
    return x


def key_of(seed, n):
    return mix(seed + G * (n + 97))


def doc_key(key, base, d):
    return mix(key + G * (((base + d) & M64) + 1))


def k_of(ids, kd):
    """k of one n-gram (all of ids) under its document's key."""
    h = 0
    for t in ids:
        h = (h * G + (t & 0xFFFFFFFF) + 1) & M64
    return mix(h ^ kd) or G


def n_ngrams(length, n):
    return max(length - n + 1, 0)


def capacity(m):
    """The smallest power of two >= max(64, 2 m)."""
    cap = MIN_CAPACITY
    while cap < 2 * m:
        cap *= 2
    return cap


def groups(lens, status, n, budget):
    """The groups of whole consecutive documents that share a table: a list of (d0, d1, m).  A group takes its first document
    and then documents while the table of its n-grams stays within `budget` bytes."""
    out, d0 = [], 0
    while d0 < len(lens):
        m, d = 0, d0
        while d < len(lens):
            md = n_ngrams(lens[d], n) if status[d] >= 0 else 0
            if d > d0 and capacity(m + md) * SLOT_BYTES > budget:
                break
            m += md
            d += 1
        out.append((d0, d, m))
        d0 = d
    return out


def starts(docs, status, n, wrong=None):
    """Per document the list of (document-relative start, the ids of the n-gram there)."""
    flat = [t for ids in docs for t in ids]
    out, pos = [], 0
    for ids, st in zip(docs, status):
        here = []
        if st >= 0 or wrong == "refused_hashed":
            if wrong == "cross_doc_end":
                here = [(i, flat[pos + i:pos + i + n]) for i in range(len(ids)) if pos + i + n <= len(flat)]
            else:
                here = [(i, ids[i:i + n]) for i in range(len(ids) - n + 1)]
        out.append(here)
        pos += len(ids)
    return out


def doc_ks(docs, status, n, seed, base, wrong=None):
    """Per document the list of (document-relative start, k)."""
    key = key_of(seed, n)
    out = []
    for d, here in enumerate(starts(docs, status, n, wrong)):
        kd = key if wrong == "no_doc_salt" else doc_key(key, 0 if wrong == "base_ignored" else base, d)
        out.append([(i, k_of(g, kd)) for i, g in here])
    return out


class Result:
    pass


def repeats(docs, status, n, seed=0, base=0, mark_first=False, wrong=None, tile=None):
    """.flags uint8 [total tokens]; .n_repeat, .n_covered, .top_count int32 and .top_first int64 [n_docs]; .tok_off int64
    [n_docs + 1]; and per token .first (document-relative, -1 where no n-gram starts) and .count (0 there)."""
    r = Result()
    nd = len(docs)
    r.tok_off = np.zeros(nd + 1, dtype=np.int64)
    if docs:
        np.cumsum([len(x) for x in docs], out=r.tok_off[1:])
    total = int(r.tok_off[-1])
    r.flags = np.zeros(total, dtype=np.uint8)
    r.first = np.full(total, -1, dtype=np.int64)
    r.count = np.zeros(total, dtype=np.int64)
    r.n_repeat = np.zeros(nd, dtype=np.int32)
    r.n_covered = np.zeros(nd, dtype=np.int32)
    r.top_count = np.zeros(nd, dtype=np.int32)
    r.top_first = np.full(nd, -1, dtype=np.int64)
    if wrong == "mark_first_swapped":
        mark_first = not mark_first
    reach = n - 1 if wrong == "covers_n_minus_1" else n
    ks = doc_ks(docs, status, n, seed, base, wrong)
    shared = {}
    if wrong == "no_doc_salt":                      # (the wrong rule: one dict for the whole batch, positions in batch order)
        for d, here in enumerate(ks):
            for i, k in here:
                shared.setdefault(k, []).append(int(r.tok_off[d]) + i)
    for d, here in enumerate(ks):
        base_pos, length = int(r.tok_off[d]), len(docs[d])
        where = {}
        for i, k in here:
            where.setdefault(k, []).append(i)
        if wrong == "no_doc_salt":
            where = {k: [p - base_pos for p in shared[k]] for k in where}
        hits = []
        for i, k in here:
            at = where[k]
            first = max(at) if wrong == "first_is_last" else min(at)
            count = len(at) - (1 if wrong == "count_minus_one" else 0)
            r.first[base_pos + i], r.count[base_pos + i] = first, count
            if (count >= 2) if mark_first else (first < i):
                hits.append(i)
        for i in hits:
            r.flags[base_pos + i] |= START
        for p in range(length):
            if any(p - reach < i <= p for i in hits
                   if not (wrong == "halo_dropped" and (base_pos + i) // tile != (base_pos + p) // tile)):
                r.flags[base_pos + p] |= COVERED
        r.n_repeat[d] = len(hits)
        r.n_covered[d] = int(((r.flags[base_pos:base_pos + length] & COVERED) != 0).sum())
        if here:
            top = max(int(r.count[base_pos + i]) for i, _ in here)
            firsts = [int(r.first[base_pos + i]) for i, _ in here if r.count[base_pos + i] == top]
            r.top_count[d] = top
            r.top_first[d] = max(firsts) if wrong == "top_tie_takes_last" else min(firsts)
    return r
