"""Token n-gram sets and overlap (jtk_ngram_set_*, jtk_batch_ngram_overlap), written out from the rule's text alone -- nothing
here is shared with jtokkit_amd/csrc/jtk_ngram_rules.h.  Python integers and a Python set of k; flags and per-document results
by their definitions, never by the kernels' tile walk.  Documents are lists of token ids (the CPU oracle's) with a status each;
a refused document (status < 0) has no n-grams whatever tokens it is given.

wrong=: a deliberately wrong rule, for the CPU tier's check that the case set tells the right rule from wrong ones."""
import numpy as np

M64 = (1 << 64) - 1
G = 0x9E3779B97F4A7C15
START, COVERED = 1, 2
MIN_CAPACITY = 64
WRONG_RULES = ("cross_doc_end", "short_doc_rule", "halo_dropped", "covers_n_minus_1", "id_not_plus_1", "probe_no_wrap",
               "probe_stops_at_mismatch", "refused_hashed")


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
    return mix(seed + G * (n + 33))


def k_of(ids, key, plus=1):
    """k of one n-gram (all of ids)."""
    h = 0
    for t in ids:
        h = (h * G + (t & 0xFFFFFFFF) + plus) & M64
    return mix(h ^ key) or G


def n_ngrams(length, n):
    return max(length - n + 1, 0)


def capacity(c, m):
    """The smallest power of two >= max(64, 2 (c + m))."""
    cap = MIN_CAPACITY
    while cap < 2 * (c + m):
        cap *= 2
    return cap


def starts(docs, status, n, wrong=None):
    """Per document the list of (document-relative start, the ids of the n-gram there)."""
    flat = [t for ids in docs for t in ids]
    out, pos = [], 0
    for ids, st in zip(docs, status):
        here = []
        if st >= 0 or wrong == "refused_hashed":
            if wrong == "cross_doc_end":
                here = [(i, flat[pos + i:pos + i + n]) for i in range(len(ids)) if pos + i + n <= len(flat)]
            elif wrong == "short_doc_rule" and 0 < len(ids) < n:
                here = [(0, list(ids))]
            else:
                here = [(i, ids[i:i + n]) for i in range(len(ids) - n + 1)]
        out.append(here)
        pos += len(ids)
    return out


def doc_keys(docs, status, seed, n, wrong=None):
    """k of every n-gram of the documents, in order (duplicates and all)."""
    key = key_of(seed, n)
    plus = 0 if wrong == "id_not_plus_1" else 1
    return [k_of(g, key, plus) for here in starts(docs, status, n, wrong) for _, g in here]


class Set:
    """The distinct k inserted so far, the capacity by the rule, and -- for the two wrong probes -- a table filled in insertion
    order as the rule describes it."""

    def __init__(self, seed, n):
        self.seed, self.n = seed, n
        self.keys = set()
        self.order = []                         # distinct keys in insertion order
        self.capacity = MIN_CAPACITY

    def add_keys(self, keys):
        keys = [int(k) for k in keys]
        assert 0 not in keys
        self.capacity = max(self.capacity, capacity(len(self.keys), len(keys)))
        for k in keys:
            if k not in self.keys:
                self.keys.add(k)
                self.order.append(k)

    def add_docs(self, docs, status, wrong=None):
        self.add_keys(doc_keys(docs, status, self.seed, self.n, wrong))

    def table(self):
        t = [0] * self.capacity
        for k in self.order:
            s = k & (self.capacity - 1)
            while t[s]:
                s = (s + 1) & (self.capacity - 1)
            t[s] = k
        return t

    def contains(self, k, wrong=None, table=None):
        if wrong not in ("probe_no_wrap", "probe_stops_at_mismatch"):
            return k in self.keys
        s = k & (self.capacity - 1)
        while True:
            if table[s] == k:
                return True
            if table[s] == 0 or wrong == "probe_stops_at_mismatch":
                return False
            s += 1
            if s == self.capacity:
                return False                    # (the wrong rule: no wrap-around)


class Result:
    pass


def overlap(docs, status, ngset, wrong=None, tile=None):
    """.flags uint8 [total tokens], .n_hit int32, .n_covered int32, .first_hit int64 [n_docs], .tok_off int64 [n_docs + 1]."""
    n = ngset.n
    key = key_of(ngset.seed, n)
    plus = 0 if wrong == "id_not_plus_1" else 1
    table = ngset.table() if wrong in ("probe_no_wrap", "probe_stops_at_mismatch") else None
    r = Result()
    r.tok_off = np.zeros(len(docs) + 1, dtype=np.int64)
    if docs:
        np.cumsum([len(x) for x in docs], out=r.tok_off[1:])
    r.flags = np.zeros(int(r.tok_off[-1]), dtype=np.uint8)
    r.n_hit = np.zeros(len(docs), dtype=np.int32)
    r.n_covered = np.zeros(len(docs), dtype=np.int32)
    r.first_hit = np.full(len(docs), -1, dtype=np.int64)
    reach = n - 1 if wrong == "covers_n_minus_1" else n
    for d, here in enumerate(starts(docs, status, n, wrong)):
        base, length = int(r.tok_off[d]), len(docs[d])
        hits = [i for i, g in here if ngset.contains(k_of(g, key, plus), wrong, table)]
        for i in hits:
            r.flags[base + i] |= START
        for p in range(length):
            if any(p - reach < i <= p for i in hits
                   if not (wrong == "halo_dropped" and (base + i) // tile != (base + p) // tile)):
                r.flags[base + p] |= COVERED
        r.n_hit[d] = len(hits)
        r.n_covered[d] = int(((r.flags[base:base + length] & COVERED) != 0).sum())
        if hits:
            r.first_hit[d] = hits[0]
    return r
