"""MinHash signatures, LSH band keys, agreement and near-duplicate clusters over token n-grams (jtk_batch_minhash,
jtk_batch_minhash_agree, HipEncoding.near_duplicates), written out from the rule's text alone -- nothing here is shared with
jtokkit_amd/csrc/jtk_minhash_rules.h.  Documents are lists of token ids (the CPU oracle's); a refused document (status < 0) is
passed as no tokens.  The arithmetic is modulo 2^64: numpy uint64 arrays wrap, and `plain_signature` is the same rule in
Python integers for documents small enough to check by hand.

wrong=: a deliberately wrong rule, for the CPU tier's check that the case set tells the right rule from wrong ones."""
import math

import numpy as np

M64 = (1 << 64) - 1
G = 0x9E3779B97F4A7C15
EMPTY = 0xFFFFFFFF
WRONG_RULES = ("halo_dropped", "no_short_rule", "a_not_odd", "id_not_plus_1", "cross_doc_end", "last_writer_wins", "band_ignores_j")


def mix(x):
    """The splitmix64 finaliser, on a Python integer."""
    x &= M64
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & M64
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & M64
    x ^= x >> 31
    return x


def mix_array(x):
    x = x.astype(np.uint64)
    x = x ^ (x >> np.uint64(30))
    x = x * np.uint64(0xBF58476D1CE4E5B9)
    x = x ^ (x >> np.uint64(27))
    x = x * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def key_of(seed, n):
    return mix(seed + G * (n + 1))


def draw(key, j):
    return mix(key + j)


def coefficients(key, K, wrong=None):
    a = [draw(key, 2 * k + 1) | (0 if wrong == "a_not_odd" else 1) for k in range(K)]
    b = [draw(key, 2 * k + 2) for k in range(K)]
    return a, b


def n_shingles(length, n):
    return 0 if length == 0 else length - min(n, length) + 1


def shingle_sets(ids, n):
    """The shingles as a set of tuples (for the true Jaccard similarity)."""
    m = min(n, len(ids))
    return {tuple(ids[i:i + m]) for i in range(len(ids) - m + 1)} if ids else set()


def jaccard(a, b, n):
    sa, sb = shingle_sets(a, n), shingle_sets(b, n)
    return len(sa & sb) / len(sa | sb) if sa | sb else 1.0


def plain_signature(ids, seed, n, K):
    """One document, Python integers only."""
    key = key_of(seed, n)
    if not ids:
        return [EMPTY] * K
    m = min(n, len(ids))
    xs = []
    for i in range(len(ids) - m + 1):
        h = 0
        for t in ids[i:i + m]:
            h = (h * G + (t & 0xFFFFFFFF) + 1) & M64
        xs.append(mix(h ^ key) & 0xFFFFFFFF)
    return [min(((((draw(key, 2 * k + 1) | 1) * x + draw(key, 2 * k + 2)) & M64) >> 32) for x in xs) for k in range(K)]


def shingle_x(ids, key, m, plus=1):
    """x of every shingle of m tokens of one token array (uint32 array)."""
    t = (np.asarray(ids, dtype=np.int64) & 0xFFFFFFFF).astype(np.uint64) + np.uint64(plus)
    count = len(t) - m + 1
    h = np.zeros(count, dtype=np.uint64)
    for j in range(m):
        h = h * np.uint64(G) + t[j:j + count]
    return mix_array(h ^ np.uint64(key)) & np.uint64(0xFFFFFFFF)


def min_values(x, a, b):
    """min over the shingles of ((a_k x + b_k) mod 2^64) >> 32, for every k."""
    a = np.array(a, dtype=np.uint64)[:, None]
    b = np.array(b, dtype=np.uint64)[:, None]
    out = np.full(a.shape[0], EMPTY, dtype=np.uint64)
    for lo in range(0, len(x), 4096):
        v = (a * x[None, lo:lo + 4096] + b) >> np.uint64(32)
        out = np.minimum(out, v.min(axis=1))
    return out.astype(np.uint32)


class Result:
    pass


def minhash(docs, seed, n, K, bands=0, wrong=None, tile=None):
    """docs: a list of id lists (empty for a refused document).  Returns .sig uint32 [n_docs, K], .n_shingles int32 [n_docs],
    .band_keys uint64 [n_docs, bands] or None.  tile: the kernels' tile, needed by the two wrong rules that are about tiles
    (a document's tokens are then at the positions its predecessors' lengths give)."""
    key = key_of(seed, n)
    a, b = coefficients(key, K, wrong)
    r = Result()
    r.sig = np.full((len(docs), K), EMPTY, dtype=np.uint32)
    r.n_shingles = np.zeros(len(docs), dtype=np.int32)
    pos = 0
    flat = [t for ids in docs for t in ids]
    for d, ids in enumerate(docs):
        start, pos = pos, pos + len(ids)
        if not ids:
            continue
        m = min(n, len(ids))
        r.n_shingles[d] = len(ids) - m + 1
        plus = 0 if wrong == "id_not_plus_1" else 1
        if wrong == "no_short_rule" and len(ids) < n:
            r.n_shingles[d] = 0
            continue
        if wrong == "cross_doc_end":
            # every token starts a shingle of n ids that runs on into the next documents (cut at the batch's end)
            src = flat[start:start + len(ids) + n - 1]
            x = shingle_x(src, key, n, plus) if len(src) >= n else shingle_x(src, key, len(src), plus)
        else:
            x = shingle_x(ids, key, m, plus)
        if wrong in ("halo_dropped", "last_writer_wins"):
            at = start + np.arange(len(x))                      # the shingles' first tokens in the batch
            if wrong == "halo_dropped":
                x = x[(at + m - 1) // tile == at // tile]
            else:
                x = x[at // tile == at[-1] // tile]
            if not len(x):
                continue
        r.sig[d] = min_values(x, a, b)
    r.band_keys = None
    if bands:
        rows = K // bands
        r.band_keys = np.zeros((len(docs), bands), dtype=np.uint64)
        for j in range(bands):
            h = np.full(len(docs), draw(key, (1 << 32) + (0 if wrong == "band_ignores_j" else j)), dtype=np.uint64)
            for i in range(rows):
                h = mix_array(h ^ r.sig[:, j * rows + i].astype(np.uint64))
            r.band_keys[:, j] = h
    return r


def agree(sig, pair_a, pair_b):
    """Per pair the number of equal columns; -1 where an index is outside [0, n_sig)."""
    n = len(sig)
    return np.array([int((sig[a] == sig[b]).sum()) if 0 <= a < n and 0 <= b < n else -1 for a, b in zip(pair_a, pair_b)], dtype=np.int32)


def candidate_pairs(n_shingles_, band_keys):
    """Per band the documents that have shingles, stable-sorted by key; every two consecutive ones with equal keys."""
    live = [d for d in range(len(n_shingles_)) if n_shingles_[d] > 0]
    pairs = set()
    for j in range(band_keys.shape[1]):
        order = sorted(live, key=lambda d: int(band_keys[d, j]))      # (sorted() is stable)
        for p, q in zip(order, order[1:]):
            if band_keys[p, j] == band_keys[q, j]:
                pairs.add((p, q))
    return sorted(pairs)


def near_duplicates(docs, threshold, seed, n, K, bands):
    """Labels: the smallest document index of each document's cluster."""
    r = minhash(docs, seed, n, K, bands)
    pairs = candidate_pairs(r.n_shingles, r.band_keys)
    need = int(math.ceil(threshold * K))
    got = agree(r.sig, [p for p, _ in pairs], [q for _, q in pairs])
    parent = list(range(len(docs)))

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x

    for (p, q), c in zip(pairs, got):
        if c >= need:
            rp, rq = find(p), find(q)
            if rp != rq:
                parent[max(rp, rq)] = min(rp, rq)
    return np.array([find(d) for d in range(len(docs))], dtype=np.int64)
