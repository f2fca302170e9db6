"""Cases of the MinHash pass (jtk_batch_minhash, jtk_batch_minhash_agree) for the CPU tier (tests/test_minhash_rules_cpu.py: the
shim of the rule header against tests/minhash_ref.py) and the GPU tier (tests/test_minhash_gpu.py).  Where placement matters a
document is built from tokens, not text: words that are one cl100k_base token each behind a space, found through the oracle,
so a document of l words has l tokens and the batch's token positions are the running sum of the lengths.  The tiers check
that from the oracle's own tokens (edges_reached works on the token counts it is given, never on the plan).

A case: name, docs (bytes), route (how it is encoded), params (a list of (ngram, num_hashes, bands, seed))."""
import collections
import re

import numpy as np

import fim_ref
import oracle_lib

Case = collections.namedtuple("Case", "name docs route params")

TILE = 512                    # JTK_MH_TILE (the CPU tier checks it against the header)
T = TILE
MAX_SEED = (1 << 64) - 1
NGRAMS = (1, 2, 5, 32)
HASH_COUNTS = (1, 63, 64, 65, 100, 128, 256)
FIM = dict(seed=11, base=0, fim_rate=1 << 31, spm_rate=1 << 31)      # the route "fim"
FIM_IDS = (100258, 100259, 100260)
CHUNK_BYTES = 1 << 16                                                 # the route "chunked"

_POOL = []


def oracle():
    return oracle_lib.get("cl100k_base")


def pool():
    """200 words of two lowercase letters that are one token behind a space."""
    if not _POOL:
        o = oracle()
        for a in "abcdefghijklmnopqrstuvwxyz":
            for b in "aeioubcdfghlmnprst":
                w = (" " + a + b).encode()
                if len(o.encode_ordinary(w)) == 1:
                    _POOL.append(w)
                if len(_POOL) == 200:
                    return _POOL
        raise AssertionError("fewer than 200 single-token words")
    return _POOL


def word(salt, i, lo=0, hi=200):
    return pool()[lo + (salt * 1000003 + i * 7919 + (i * i) % 101) % (hi - lo)]


def doc(length, salt, lo=0, hi=200):
    """A document of `length` tokens."""
    return b"".join(word(salt, i, lo, hi) for i in range(length))


def batch(lens, salt=0):
    return [doc(l, salt * 131 + d) for d, l in enumerate(lens)]


# num_hashes 1, 63, 64, 65, 100, 128, 256; bands 0, 1, K and a proper divisor; seeds 0 and 2^64 - 1
K_SWEEP = [(5, 1, 1, 0), (5, 63, 0, 0), (5, 63, 9, MAX_SEED), (5, 64, 64, 0), (5, 65, 5, 0), (5, 100, 0, MAX_SEED), (5, 100, 20, 0),
           (5, 128, 1, 0), (5, 256, 32, MAX_SEED)]


def cases():
    out = []
    for n in NGRAMS:
        out.append(Case("lengths_n%d" % n, batch([0, 1, n - 1, n, n + 1, 0, 2 * n + 3, 1, n, 0], n), "ordinary", [(n, 128, 16, 0)]))
    for n in (2, 5, 32):
        # the second document starts n + 2 tokens before the first tile edge and runs 2 n + 3 past it
        out.append(Case("straddle_n%d" % n, batch([T - n - 2, 3 * n + 5, 7], 40 + n), "ordinary", [(n, 64, 8, 1)]))
    # a document ends on a tile's last token (511), the next starts on a tile's first (512); one starts on a tile's last (1023)
    out.append(Case("doc_edges", batch([300, 212, 511, 20, 9], 3), "ordinary", [(5, 128, 0, 3), (1, 64, 0, 3)]))
    # 3 tokens at 511..513 (shorter than 5) and 20 tokens at 1014..1033 (shorter than 32) straddle tile edges
    out.append(Case("short_straddles", batch([T - 1, 3, 10, T - 22, 20, 5], 4), "ordinary", [(5, 64, 0, 4), (32, 64, 4, 4)]))
    for r in (1, 2, 65):
        out.append(Case("empty_runs_%d" % r, batch([0] * r + [T] + [0] * r + [30] + [0] * r, 5), "ordinary", [(5, 64, 8, 5)]))
    # tokens 8 .. 1043: the middle tile is wholly inside, two short documents before and two after in the outer tiles
    out.append(Case("three_tiles", batch([5, 3, 2 * T + 12, 4, 6], 6), "ordinary", K_SWEEP + [(32, 128, 16, 6), (1, 256, 0, 6)]))
    out.append(Case("one_doc_one_tile", batch([200], 7), "ordinary", [(5, 128, 16, 7), (32, 100, 10, 7)]))
    out.append(Case("many_short", batch([1, 2, 1, 0, 1, 1, 2, 0, 1, 1] * 60, 8), "ordinary", [(2, 65, 13, 8), (1, 64, 0, 8)]))
    out.append(Case("refused_special", [doc(20, 90), doc(3, 91) + b"<|endoftext|>" + doc(2, 92), doc(7, 93), doc(9, 94)], "encode", [(5, 64, 8, 9)]))
    out.append(Case("refused_utf8", [doc(20, 95), doc(3, 96) + b"\xff" + doc(2, 97), doc(7, 98), doc(9, 99)], "validate", [(5, 64, 8, 9)]))
    out.append(Case("allow_special", [doc(10, 100) + b"<|endoftext|>" + doc(6, 101), b"<|endoftext|>", doc(4, 102),
                                      b"<|fim_prefix|>" + doc(40, 103)], "allow_special", [(2, 64, 8, 10)]))
    out.append(Case("fim", batch([30, 8, 1, 0, 50] * 2, 11), "fim", [(5, 64, 8, 11)]))
    # three chunks of 64 KiB of device-resident text
    out.append(Case("chunked", batch([1500, 900, 0, 2100, 1, 640] * 12, 12), "chunked", [(5, 64, 8, 12)]))
    return out


_SPECIAL_RE = None


def expected_ids(case):
    """(ids per document, status per document) by the CPU oracle: what the encode of this case's route leaves on the device.  A
    refused document (status < 0) is given no tokens here: the rule gives it no shingles whatever the encode left it."""
    global _SPECIAL_RE
    o = oracle()
    ids, status = [], []
    if case.route == "fim":
        r = fim_ref.encode_batch(o.encode_ordinary, case.docs, FIM["seed"], FIM["base"], FIM["fim_rate"], FIM["spm_rate"], FIM_IDS)
        return [list(x) for x in r.docs], r.status.tolist()
    specials = oracle_lib.ENCODINGS["cl100k_base"]["specials"]
    if _SPECIAL_RE is None:
        _SPECIAL_RE = re.compile(b"(" + b"|".join(re.escape(k.encode()) for k in specials) + b")")
    for d in case.docs:
        st, t = 0, []
        if case.route == "encode":
            try:
                t = o.encode(d)
            except oracle_lib.OracleError as e:
                st = e.code
        elif case.route == "validate" and not fim_ref.well_formed(d):
            st = -6                                                    # JTK_ERR_BAD_UTF8
        elif case.route == "allow_special":
            for part in _SPECIAL_RE.split(d):
                t += [specials[part.decode()]] if part.decode() in specials else o.encode_ordinary(part)
        else:
            t = o.encode_ordinary(d)
        ids.append(list(t))
        status.append(st)
    return ids, status


def agree_pairs(n_sig):
    """a == b, both orders of a pair, and indices of -1 and n_sig on either side."""
    last = n_sig - 1
    return [(0, 0), (last, last), (0, last), (last, 0), (1 % n_sig, 2 % n_sig), (2 % n_sig, 1 % n_sig), (-1, 0), (0, -1), (n_sig, 0),
            (0, n_sig), (n_sig + 5, -3)]


def band_label(K, bands):
    return {x for x, hit in (("0", bands == 0), ("1", bands == 1), ("K", bands == K), ("proper", 1 < bands < K)) if hit}


def all_edges():
    e = {("len", n, l) for n in NGRAMS for l in (0, 1, n - 1, n, n + 1)}
    e |= {("straddle", n, s) for n in (2, 5, 32) for s in range(1, n)}
    e |= {"ends_on_tile_last", "starts_on_tile_last", "starts_on_tile_first", "short_straddles", "three_tiles", "one_doc_one_tile",
          "tile_over_256_docs"}
    e |= {(where, r) for where in ("empty_run_tile_first", "empty_run_start", "empty_run_end") for r in (1, 2, 65)}
    e |= {("K", k) for k in HASH_COUNTS} | {("bands", b) for b in ("0", "1", "K", "proper")} | {("seed", 0), ("seed", MAX_SEED)}
    e |= {("refused", "encode"), ("refused", "validate")} | {("route", r) for r in ("allow_special", "fim", "chunked")}
    return e


def edges_reached(case, lens, status):
    """The edges a case reaches, from the token counts per document (those of the oracle's encode) and the statuses."""
    got = set()
    lens = [int(x) for x in lens]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64).tolist()
    total, nd = off[-1], len(lens)
    got.add(("route", case.route))
    for n, K, bands, seed in case.params:
        got.add(("K", K))
        got |= {("bands", b) for b in band_label(K, bands)}
        got.add(("seed", seed))
        for d, l in enumerate(lens):
            s, e = off[d], off[d + 1]
            if l in (0, 1, n - 1, n, n + 1):
                got.add(("len", n, l))
            if l == 0:
                continue
            if e % T == 0 and e < total:
                got.add("ends_on_tile_last")
            if s % T == T - 1:
                got.add("starts_on_tile_last")
            if s % T == 0 and s > 0:
                got.add("starts_on_tile_first")
            if l < n and s // T != (e - 1) // T:
                got.add("short_straddles")
            if l >= n:
                for edge in range((s // T + 1) * T, e, T):
                    got |= {("straddle", n, sp) for sp in range(1, n) if edge - sp >= s and edge - sp + n <= e}
            if (e - 1) // T - s // T >= 2 and s % T != 0 and e % T != 0 and e < total:
                before = [x for x in range(d) if lens[x]]
                after = [x for x in range(d + 1, nd) if lens[x]]
                if before and after and lens[before[-1]] < T and lens[after[0]] < T:
                    got.add("three_tiles")
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
    if nd == 1 and 0 < total <= T:
        got.add("one_doc_one_tile")
    for t0 in range(0, total, T):
        if sum(1 for x in range(nd) if lens[x] and off[x] < t0 + T and off[x + 1] > t0) > 256:
            got.add("tile_over_256_docs")
    for d in range(1, nd - 1):
        if status[d] < 0 and status[d - 1] == 0 and status[d + 1] == 0 and lens[d - 1] and lens[d + 1]:
            got.add(("refused", case.route))
    return got


# ---- the estimator: 54 fixed pairs of 400-token documents that share a suffix
EST_FRACTIONS = (0.0, 0.1, 0.3, 0.5, 0.8, 1.0)
EST_NGRAMS = (1, 2, 5)
EST_SEEDS = (0, 1, 12345)
EST_K = 256
EST_LEN = 400


def estimator_pairs():
    """Per fraction two documents (bytes) of 400 tokens whose last round(f * 400) tokens are the same; the prefixes draw their
    words from disjoint halves of the pool and the suffix from the whole pool, so f = 0 is Jaccard 0 for every n."""
    out = []
    for k, f in enumerate(EST_FRACTIONS):
        s = int(round(f * EST_LEN))
        suffix = doc(s, 700 + k)
        out.append((f, doc(EST_LEN - s, 710 + k, 0, 100) + suffix, doc(EST_LEN - s, 720 + k, 100, 200) + suffix))
    return out


# ---- near duplicates: 40 documents
NEAR = dict(threshold=0.6, ngram=2, num_hashes=128, bands=32, seed=7)
NEAR_LEN = 200


def _replaced(text_words, salt):
    """5 % of the words (10 of 200, evenly spread) replaced by other words."""
    w = list(text_words)
    for j in range(10):
        at = 7 + 20 * j
        k = 0
        while word(salt, at + 1000 * k) == w[at]:
            k += 1
        w[at] = word(salt, at + 1000 * k)
    return w


def near_dup_batch():
    """(docs as bytes, the expected labels).  With n = 2 a replaced word changes 2 of a document's 199 shingles: a copy with 10
    words replaced shares at least 179 shingles with its original, Jaccard >= 179 / 219 = 0.82, against the threshold 0.6;
    unrelated documents share a few of the pool's 40 000 word pairs by chance."""
    base = [[word(500 + g, i) for i in range(NEAR_LEN)] for g in range(27)]
    plan = []                                   # (words, group)
    for g in range(6):
        plan.append((base[g], g))
    plan += [(base[0], 0), (base[0], 0), (base[1], 1)]                                           # exact copies
    plan += [(_replaced(base[2], 601), 2), (_replaced(base[2], 602), 2), (_replaced(base[2], 603), 2), (_replaced(base[3], 604), 3),
             (_replaced(base[3], 605), 3), (_replaced(base[0], 606), 0)]                         # 5 % replaced
    plan += [(base[g], g) for g in range(6, 27)]                                                 # unrelated
    plan += [([], 100), ([], 101), ([], 102), ([word(9, 0), word(9, 1)], 103)]                   # three empty, one of 2 tokens
    order = [(7 * i + 3) % 40 for i in range(40)]                                                # (7 and 40 are coprime: a permutation)
    assert len(plan) == 40 and sorted(order) == list(range(40))
    docs = [None] * 40
    group = [None] * 40
    for src, at in enumerate(order):
        docs[at] = b"".join(plan[src][0])
        group[at] = plan[src][1]
    labels = [min(i for i in range(40) if group[i] == group[d]) for d in range(40)]
    return docs, np.array(labels, dtype=np.int64)
