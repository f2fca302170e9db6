"""A plain model of jtk_batch_encode_device_max_tokens (jtk_abi.cpp drives the rounds, jtokkit_amd/csrc/jtk_maxtok.hip decides):
pure Python, with the CPU oracle for splits and merges and no call into product code.  For a batch it replays the rounds --
which documents are open, the prefix each one gets, where that prefix lies in the round's gather buffer and in its chunk's piece
mask -- and decides every document the way the rules say, the last safe piece start found by a loop over the piece starts of
oracle.split(prefix), byte position by byte position, without any word arithmetic.  What it returns per document is what the
case set (tests/maxtok_cases.py) names its edges by and what the tests compare with the oracle on the whole document.

`mutant=` switches on one of the mistakes a kernel could make (MUTANTS); the case set must tell each from the right rule."""
import collections

import numpy as np

MARGIN = 16                   # JTK_MAXTOK_MARGIN
TILE = 2048                   # JTK_TILE: a chunk's mask origin is the chunk's first byte rounded down to it
HOST_CHUNK = 32 << 20         # jtk_batch.host_chunk_bytes
DEVICE_CHUNK = 1 << 30        # jtk_batch.chunk_bytes
UNSUPPORTED_SPECIAL = -2

MUTANTS = ("M_unsafe",        # ignores jtk_maxtok_safe_start
           "M_margin",        # accepts starts up to p (the bit of the neighbour's first byte included) instead of p - 16
           "M_top1",          # accepts p - 15
           "M_sum64",         # sums the byte lengths of the first 64 tokens only
           "M_min")           # p == len: keeps n instead of min(n, max_tokens)


# ---- the rules, restated (jtk_maxtok_rules.h)
def first_prefix(max_tokens):
    return 1 << 44 if max_tokens > (1 << 40) else 8 * max_tokens + 64


def next_prefix(P):
    return P if P > (1 << 40) else 4 * P


def prefix_bytes(length, P, cb):
    p = min(length, P)
    return length if p > cb else p


def maybe_space(c):
    return 0x09 <= c <= 0x0D or c in (0x20, 0xC2, 0xE1, 0xE2, 0xE3)


def safe_start(c0, c1):
    return not maybe_space(c0) or (c0 < 0x80 and not maybe_space(c1))


def backoff(tx, keep, nb, tok_len):
    """GptBytePairEncoding.java:90-100 -> (kept, from, units, ok)."""
    n = len(tx)
    while True:
        if nb == n or (tx[nb] & 0xC0) != 0x80:
            return keep, nb, 0, True
        c = nb
        while c > 0 and (tx[c] & 0xC0) == 0x80:
            c -= 1
        if tx[c:c + 3] == b"\xef\xbf\xbd":
            return keep, c, 1, True
        if keep == 0:
            return 0, 0, 0, False
        nb -= tok_len[keep - 1]
        keep -= 1


def more_units_than(tx, start, k):
    u = 0
    for c in tx[start:start + 64]:
        if (c & 0xC0) != 0x80:
            u += 2 if c >= 0xF0 else 1
            if u > k:
                return True
    return False


class Oracle:
    """The oracle's answers, each asked once: token lists and piece starts per byte string, byte length per id."""

    def __init__(self, o):
        self.o, self._enc, self._starts, self._len, self._whole = o, {}, {}, {}, {}

    def tokens(self, b):
        if b not in self._enc:
            self._enc[b] = self.o.encode_ordinary(b)
        return self._enc[b]

    def starts(self, b):
        if b not in self._starts:
            pos, out = 0, []
            for piece in self.o.split(b):
                out.append(pos)
                pos += len(piece)
            self._starts[b] = out
        return self._starts[b]

    def tok_len(self, ids):
        for t in ids:
            if t not in self._len:
                self._len[t] = len(self.o.decode_bytes([t]))
        return [self._len[t] for t in ids]

    def whole(self, doc, max_tokens):
        """encode_ordinary(doc, max_tokens) of the whole document: (ids, truncated)."""
        if (doc, max_tokens) not in self._whole:
            self._whole[(doc, max_tokens)] = self.o.encode_ordinary(doc, max_tokens)
        return self._whole[(doc, max_tokens)]


def special_docs(docs, literals):
    """text.contains(literal), per document."""
    return [any(lit in d for lit in literals) for d in docs]


def device_chunk_starts(goff, cb):
    """plan_device_chunks / k_plan_chunks: the first document at or after c * cb, for a job of more than one and a quarter chunks."""
    n_bytes, n = int(goff[-1]), len(goff) - 1
    starts = [0]
    if n_bytes > cb + cb // 4 and n > 1:
        for c in range(1, (n_bytes + cb - 1) // cb):
            d = int(np.searchsorted(goff[:n], c * cb, side="left"))
            if d > starts[-1] and d < n:
                starts.append(d)
    return starts


Scan = collections.namedtuple("Scan", "round p g0 chunk n_chunks base top q word step lane steps n_tokens cum cum64")
Result = collections.namedtuple("Result", "round p g0 src16 dst16 scans gathers ids kept truncated status nb")
Round = collections.namedtuple("Round", "n_in open_items n_act gbytes chunk_first")


def run(oracle, docs, max_tokens, ordinary=True, chunk_bytes=None, tensor_offset=0, literals=(), mutant=None):
    """-> (results [n_docs], rounds).  A Result holds the deciding round, its p and g0, the alignments of that round's gather, every
    scan the document went through (base and top as k_mt_decide sees them; the mask word, scan step and lane that find q), every
    gather as (round, source address % 16, g0 % 16, p), and the final (ids, kept, truncated, status)."""
    assert mutant is None or mutant in MUTANTS
    mx = max_tokens
    chunk = DEVICE_CHUNK if chunk_bytes is None else chunk_bytes
    cb = min(HOST_CHUNK, chunk)
    doc_off = np.concatenate([[0], np.cumsum([len(d) for d in docs])]).astype(np.int64)
    special = special_docs(docs, literals) if not ordinary else [False] * len(docs)
    out = [None] * len(docs)
    scans = [[] for _ in docs]
    gathers = [[] for _ in docs]
    src16 = [int(tensor_offset + doc_off[d]) % 16 for d in range(len(docs))]
    items = []                                                               # round 1: every document is an item
    for d, doc in enumerate(docs):
        if special[d]:
            out[d] = Result(0, 0, 0, src16[d], 0, (), (), [], 0, False, UNSUPPORTED_SPECIAL, 0)
        elif not doc or mx == 0:
            _, start, units, ok = backoff(doc, 0, 0, [])
            out[d] = Result(0, 0, 0, src16[d], 0, (), (), [], 0, bool(ok and more_units_than(doc, start, units)), 0, 0)
        items.append((d, out[d] is None))
    rounds = []
    P, rnd = first_prefix(mx), 1
    while True:
        act = [d for d, is_open in items if is_open]
        if not act:
            rounds.append(Round(len(items), [], 0, 0, []))
            break
        ps = [prefix_bytes(len(docs[d]), P, cb) for d in act]
        goff = np.concatenate([[0], np.cumsum(ps)]).astype(np.int64)
        first = device_chunk_starts(goff, chunk)
        rounds.append(Round(len(items), [j for j, (_, is_open) in enumerate(items) if is_open], len(act), int(goff[-1]), first))
        nxt = []
        for slot, d in enumerate(act):
            doc, p, g0 = docs[d], ps[slot], int(goff[slot])
            c = int(np.searchsorted(first, slot, side="right")) - 1
            gathers[d].append((rnd, src16[d], g0 % 16, p))
            pre = doc[:p]
            toks = oracle.tokens(pre)
            tl = oracle.tok_len(toks)
            n = len(toks)
            k, nb = -1, 0
            if p == len(doc):
                k = n if mutant == "M_min" else min(n, mx)
                nb = sum(tl[:min(k, 64)] if mutant == "M_sum64" and mx > 64 else tl[:k])
            else:
                base = g0 - (int(goff[first[c]]) & ~(TILE - 1))
                top = base + p - MARGIN
                hi = p if mutant == "M_margin" else p - MARGIN + 1 if mutant == "M_top1" else p - MARGIN
                st = set(oracle.starts(pre))
                if mutant == "M_margin":
                    st.add(p)                                                # (the neighbour's first byte, or the end of the text)
                q = 0
                for pos in range(hi, 0, -1):                                 # byte by byte, from the margin down
                    if pos in st and (mutant == "M_unsafe" or safe_start(doc[pos], doc[pos + 1] if pos + 1 < len(doc) else 0)):
                        q = pos
                        break
                tw, wl = top >> 6, (base + 1) >> 6
                steps = (tw - wl) // 64 + 1 if top > base and tw >= wl else 0
                word = step = lane = -1
                if q > 0 and q <= p - MARGIN:
                    word = (base + q) >> 6
                    step, lane = (tw - word) // 64, (tw - word) % 64
                    steps = step + 1
                cum = sum(tl[:mx])
                cum64 = sum(tl[:64])
                scans[d].append(Scan(rnd, p, g0, c, len(first), base, top, q, word, step, lane, steps, n, cum, cum64))
                if q > 0 and n >= mx:
                    s = cum64 if mutant == "M_sum64" and mx > 64 else cum
                    if s <= q:
                        k, nb = mx, s
            if k < 0:
                nxt.append((d, True))
                continue
            nxt.append((d, False))
            keep, start, units, ok = backoff(doc, k, nb, tl)
            tr = bool(ok and more_units_than(doc, start, units))
            out[d] = Result(rnd, p, g0, src16[d], g0 % 16, tuple(scans[d]), tuple(gathers[d]), toks[:keep], keep, tr, 0, nb)
        items = nxt
        P, rnd = next_prefix(P), rnd + 1
    return out, rounds


def expected(oracle, docs, max_tokens, ordinary, literals=()):
    """What the call must return per document: the oracle on the whole document, or the special-token reference."""
    sp = special_docs(docs, literals) if not ordinary else [False] * len(docs)
    out = []
    for d, doc in enumerate(docs):
        if sp[d]:
            out.append(([], 0, False, UNSUPPORTED_SPECIAL))
        else:
            ids, tr = oracle.whole(doc, max_tokens)
            out.append((ids, len(ids), tr, 0))
    return out
