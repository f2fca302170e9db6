"""The case set of the allow-special edge tests (CPU and GPU tier): batches for JTK_ENCODE_ALLOW_SPECIAL built on the partition of
its kernels (jtokkit_amd/csrc/jtk_special.hip) -- k_sp_find's 16-byte lanes, 1024-byte waves and 4096-byte workgroups, the two
bounds of its scans (batch end, document's end) and its document lookup; the 256-lane launch blocks of k_sp_resolve / k_sp_walk
and the look-back window of the certain test; the empty slots of k_sp_subs; k_sp_gather's 4096 tokens a workgroup, its
grid-stride rounds and its keep-j shortcut.  model() walks a batch as the kernels do (tests/special_sim, the shared rule header
and plain loops) and says where every literal, sub-document and output token lands; reach() names the edges a batch reaches
from the model's answer, and the tests assert on it.  Built on the CPU, seeded.

Filler between literals is ASCII words (none holds `a`, `b` or `@`: the chain and stitch literals) with decoys that fire the
first-byte bitmap without a match: `<`, `<|`, `<|endoftext|` without its `>`, and the first bytes of every longer literal."""
import collections
import ctypes as C
import functools
import os
import random

import numpy as np

import oracle_lib
import special_ref

# ---- the partition of the kernels (tests/test_special_cases_cpu.py reads them from the sources)
LANE = 16                     # bytes per k_sp_find lane
WAVE = 64 * LANE              # bytes per wave of k_sp_find
BLOCK = 4096                  # JTK_SPECIAL_BLOCK: bytes per k_sp_find workgroup (FT = 256 lanes)
FT = 256
GT, GPER = 256, 16            # k_sp_gather: lanes per workgroup, output tokens per lane
GATHER_WG = GT * GPER         # 4096 output tokens per gather workgroup and round
GATHER_BYTES = 4 * GATHER_WG  # the gather's grid: n_bytes // GATHER_BYTES + 1 workgroups
LAUNCH = 256                  # lanes per workgroup of resolve, walk, docs, subs, count
MIN_CHUNK = 65536             # the smallest JTK_OPT_CHUNK_BYTES / JTK_OPT_HOST_CHUNK_BYTES
LIMIT = 128 << 10             # every batch is smaller

EOT = b"<|endoftext|>"
PRE = b"<|e"
L1, L2 = b"@", b"#$"
L17 = b"{" + b"s" * 15 + b"}"
L300 = b"[" + b"q" * 298 + b"]"
L4100 = b"(" + b"w" * 4098 + b")"
SWEEP_LITS = (EOT, L1, L2, L17, L300)
LONG_A = b"a" * 302
LONG_STARTS = (4 * 4096 - 6, 6 * 4096 - 2)     # where find_dense holds the 4100-byte literal

CL100K = "cl100k_base"
# custom encodings: the cl100k rank file with a special set of their own (name -> ordered {literal: id})
CUSTOM = {
    "sp_find": collections.OrderedDict([(EOT, 100257), (L1, 100300), (L2, 100301), (L17, 100302), (L300, 100303), (L4100, 100304)]),
    "sp_prefix": collections.OrderedDict([(EOT, 100257), (PRE, 100300)]),
    "sp_chain_a": collections.OrderedDict([(b"a", 100300), (b"aa", 100301), (b"aaa", 100302)]),
    "sp_chain_abab": collections.OrderedDict([(b"abab", 100300), (b"bab", 100301), (b"ba", 100302)]),
    "sp_chain_aba": collections.OrderedDict([(b"aba", 100300), (b"a", 100301)]),
    "sp_stitch": collections.OrderedDict([(L1, 100300), (LONG_A, 100301), (b"a", 100302), (EOT, 100257)]),
}
STITCH_TOTALS = (4095, 4096, 4097, 8191, 8192, 8193)
EMPTY_RUNS = (1, 2, 300)
DOC_COUNTS = (255, 256, 257)

MUTANTS = dict(M_batch_end=1, M_no_tail_mask=2, M_doc_ge=3, M_first_match=4, M_window=5, M_chain_docs=6, M_empty_at_self=7,
               M_keep_j=8, M_pad_end=9)

Case = collections.namedtuple("Case", "name kind enc docs allowed modes validate pad invalid")
#   enc: cl100k_base or a key of CUSTOM; docs: [bytes]; allowed: the allowed sets to run, each None (every literal) or a tuple of
#   literals; modes: the values of `ordinary`; validate: run with JTK_ENCODE_VALIDATE_UTF8; pad: the bytes behind the batch that
#   would complete its cut literal (find/batch-end); invalid: the documents declared malformed UTF-8 (stitch, -6)


def specials(enc):
    """Ordered {literal bytes: id}."""
    if enc in CUSTOM:
        return CUSTOM[enc]
    return collections.OrderedDict((k.encode(), v) for k, v in oracle_lib.ENCODINGS[enc]["specials"].items())


def amap(enc, allowed):
    sp = specials(enc)
    return collections.OrderedDict((k, v) for k, v in sp.items() if allowed is None or k in allowed)


def oracle():
    return oracle_lib.get(CL100K)          # (every encoding here has cl100k's ranks and pattern: encodeOrdinary is the same)


# ---- filler
WORDS = [b"the", b"of", b"token", b"edge", b"code", b"row", b"unit", b"71", b"will", b"seen", b"in", b"it", b"model", b"365"]
DECOYS = {
    "sp_find": [b"<", b"<|", b"<|endoftext|", b"#", b"{s", b"[q", b"("],
    "sp_prefix": [b"<", b"<|"],
    CL100K: [b"<", b"<|", b"<|endoftext|", b"<|fim_", b"<|endofprompt"],
    "sp_stitch": [b"<", b"<|", b"<|endoftext|"],
}


def filler(rng, n, enc, decoys=True):
    """Exactly n bytes of words and decoys; holds no literal of `enc`."""
    out, size = [], 0
    dec = DECOYS.get(enc, []) if decoys else []
    while size < n + 1:
        w = rng.choice(dec) if dec and rng.random() < 0.2 else rng.choice(WORDS)
        out.append(w)
        size += len(w) + 1
    text = b" ".join(out)[:n]
    assert len(text) == n and not any(lit in text for lit in specials(enc)), enc
    return text


def _round_up(x, m):
    return (x + m - 1) // m * m


def _pack(docs):
    doc_off = np.zeros(len(docs) + 1, dtype=np.int64)
    np.cumsum([len(d) for d in docs], out=doc_off[1:])
    return b"".join(docs), doc_off


def _case(name, kind, enc, docs, allowed=(None,), modes=(False, True), validate=False, pad=b"", invalid=()):
    assert sum(len(d) for d in docs) < LIMIT, name
    return Case(name, kind, enc, tuple(docs), tuple(allowed), tuple(modes), validate, pad, tuple(invalid))


# ---- find: a literal at every offset from E - len - 1 to E + 1 of an edge
def _sweep(seed, name, kind, lits, edge, is_anchor, first_anchor, cap=LIMIT - 512):
    """A literal of `lits` at anchor + delta for every delta in [-len - 1, 1], each at an anchor of its own (a multiple of `edge`
    that is_anchor accepts); documents end between the placements.  -> cases of up to `cap` bytes."""
    rng = random.Random(seed)
    out, places, cur = [], [], 0

    def flush():
        n = cur + rng.randint(3, 40)
        buf = bytearray(filler(rng, n, "sp_find"))
        cuts = [0]
        for i, (s, lit) in enumerate(places):
            buf[s:s + len(lit)] = lit
            if i and (i % 3 == 0 or edge >= BLOCK):
                prev_end = places[i - 1][0] + len(places[i - 1][1])
                cuts.append((prev_end + s + 1) // 2)
        cuts.append(n)
        docs = [bytes(buf[a:b]) for a, b in zip(cuts, cuts[1:])]
        out.append(_case("%s_%d" % (name, len(out)), kind, "sp_find", docs, allowed=(None, (EOT,))))

    for lit in lits:
        for delta in range(-len(lit) - 1, 2):
            while True:
                a = max(_round_up(cur + len(lit) + 2, edge), first_anchor)
                while not is_anchor(a):
                    a += edge
                if a + delta + len(lit) + 2 <= cap:
                    break
                flush()
                places, cur = [], 0
            places.append((a + delta, lit))
            cur = a + delta + len(lit) + 1
    flush()
    return out


def _find_cases():
    out = _sweep(11, "find_lane", "find/lane", SWEEP_LITS, LANE, lambda a: a % WAVE != 0, LANE)
    out += _sweep(12, "find_wave", "find/wave", SWEEP_LITS, WAVE, lambda a: a % BLOCK != 0, WAVE)
    out += _sweep(13, "find_block", "find/block", SWEEP_LITS, 2 * BLOCK, lambda a: True, 2 * BLOCK)
    # a lane of 16 candidates, a whole block of them, a wave without a candidate between two that hold some, and the 4100-byte
    # literal from 6 bytes before a block edge (it ends two bytes short of the block after the next) and from 2 bytes before one
    # (2 + 4096 + 2: three find blocks)
    rng = random.Random(14)
    buf = bytearray(filler(rng, 7 * BLOCK + 200, "sp_find"))
    buf[64:80] = L1 * 16
    buf[BLOCK:2 * BLOCK] = L1 * BLOCK
    w = 2 * BLOCK
    buf[w:w + 3 * WAVE] = filler(rng, 3 * WAVE, "sp_find", decoys=False)
    for p in (w + 5, w + 500, w + WAVE - 13, w + 2 * WAVE, w + 2 * WAVE + 700):
        buf[p:p + len(EOT)] = EOT
    for p in LONG_STARTS:
        buf[p:p + len(L4100)] = L4100
    cuts = [0, 70, BLOCK + 1000, 2 * BLOCK + WAVE + 100, len(buf)]
    out.append(_case("find_dense", "find/block", "sp_find", [bytes(buf[a:b]) for a, b in zip(cuts, cuts[1:])], allowed=(None, (L1, L4100))))
    return out


def _doc_boundary_case():
    """A document boundary at every position 1..12 inside `<|endoftext|>`; `<|e` ends inside the first document from 3 on."""
    rng = random.Random(21)
    docs = []
    for k in range(1, len(EOT)):
        docs.append(filler(rng, rng.randint(5, 60), "sp_prefix") + EOT[:k])
        docs.append(EOT[k:] + filler(rng, rng.randint(5, 60), "sp_prefix"))
    docs.append(filler(rng, 30, "sp_prefix") + EOT + b" " + PRE + filler(rng, 9, "sp_prefix"))
    docs.append(filler(rng, 40, "sp_prefix"))
    return _case("find_doc_boundary", "find/doc-boundary", "sp_prefix", docs, allowed=(None, (EOT,), (PRE,)))


def short_by(m):
    """The bytes a batch of n_bytes = m mod 16 stops short of its literal's end: 1 to 3, and inside the last granule."""
    return min(1 + m % 3, 16 - m) if m else 1


def _batch_end_cases():
    rng = random.Random(31)
    out = []
    for m in range(16):
        for short in (0, short_by(m)):
            n = 64 + m
            lit = EOT[:len(EOT) - short]
            d0 = filler(rng, 21, CL100K)
            d1 = filler(rng, n - 21 - len(lit), CL100K) + lit
            out.append(_case("batch_end_%s_%d" % ("short" if short else "exact", m), "find/batch-end", CL100K, [d0, d1],
                             pad=EOT[len(EOT) - short:]))
    return out


def _docs_cases():
    rng = random.Random(41)
    out = []
    f = lambda n: filler(rng, n, CL100K)
    for r in EMPTY_RUNS:
        docs = [b""] * r + [f(40) + EOT] + [b""] * r + [EOT + f(33)] + [b""] * r + [EOT] + [b""] * r + [f(20) + EOT + f(3), EOT] + [b""] * r
        out.append(_case("docs_empties_%d" % r, "docs/empties", CL100K, docs))
    for n in DOC_COUNTS:
        docs = []
        for d in range(n):
            k = d % 5
            docs.append([b"", EOT, f(7), EOT + f(5) + EOT, f(11) + EOT][k])
        out.append(_case("docs_count_%d" % n, "docs/empties", CL100K, docs))
    # doc_off on 16-, 1024- and 4096-byte edges, a literal at each side of every boundary
    docs, at = [], 0
    for end in (16, 32, 48, 1024, 1040, 2048, 4096, 4112, 8192, 8192, 8208):
        n = end - at
        docs.append(b"" if n == 0 else EOT + f(n - 13) if n < 26 else EOT + f(n - 26) + EOT)
        at = end
    docs.append(EOT)
    out.append(_case("docs_aligned", "docs/empties", CL100K, docs))
    # more than 1.25 chunks of the smallest size: a literal lies across byte MIN_CHUNK at a document's end, 300 empty documents
    # follow -- the chunk plan of the sub-documents cuts behind the literal's slot, at the head of the empty ones
    docs = [f(20000), f(MIN_CHUNK - 6 - 20000) + EOT] + [b""] * 300 + [EOT + f(20000), b"", b"", f(5000) + EOT]
    out.append(_case("docs_two_chunks", "docs/empties", CL100K, docs))
    return out


# ---- chains
def n_candidates(text, lits):
    return sum(any(text.startswith(x, p) for x in lits) for p in range(len(text)))


def _chain_case(enc, unit, run, exact, h):
    """Isolated `unit`s (one certain candidate each) lead a `run` (one chain) across candidate indices 255|256 and 511|512 and
    byte 4096 of the text; `exact` units (the look-back at its limit) follow; documents 2 and 3 cut a run in two at h."""
    rng = random.Random(len(enc))
    lits = list(specials(enc))
    assert n_candidates(unit, lits) == 1 and n_candidates(run, lits) >= 12
    parts, n_cand, size = [], 0, 0

    def add(x):
        nonlocal n_cand, size
        parts.append(x)
        n_cand += n_candidates(x, lits)
        size += len(x)

    for edge in (256, 512):
        while n_cand < edge - 6:
            add(b" " + rng.choice(WORDS) + b" " + unit)
        add(b" " + run)
    add(b" ")
    add(filler(rng, BLOCK - 6 - size, enc))
    add(run)
    for _ in range(20):
        add(b" " + rng.choice(WORDS) + b" " + exact + rng.choice([b"", b" "]) + rng.choice(WORDS))
    main = b"".join(parts)
    docs = [main, b"", filler(rng, 30, enc) + b" " + run[:h], run[h:] + b" " + filler(rng, 30, enc), run, unit]
    first = lits[0]
    return _case("chains_" + enc[9:], "chains", enc, docs, allowed=(None, (first,), tuple(lits[1:])))


def _chain_two_chunks():
    """More than 1.25 chunks of the smallest size, a run of `a` from 7 bytes before byte MIN_CHUNK: the kept `aaa` at MIN_CHUNK - 1
    lies across the chunk edge, its segment slot and the empty slots of the dropped candidates behind it start the next chunk."""
    rng = random.Random(77)
    enc = "sp_chain_a"
    main = filler(rng, MIN_CHUNK - 7, enc) + b"a" * 19 + b" " + filler(rng, 21000, enc) + b" aaaa"
    return _case("chains_two_chunks", "chains", enc, [main, b"aa", filler(rng, 3000, enc) + b"a"], allowed=(None, (b"aa", b"aaa")))


def _chain_cases():
    return [_chain_two_chunks(),
            _chain_case("sp_chain_a", b"a", b"a" * 19, b"aaa", 10),
            _chain_case("sp_chain_abab", b"ba", b"ab" * 10, b"ababa", 11),
            _chain_case("sp_chain_aba", b"a", b"ab" * 12 + b"a", b"aba", 2)]


# ---- stitch
def _stitch_cases():
    rng = random.Random(61)
    out = []
    f = lambda n: filler(rng, n, "sp_stitch")
    for total in STITCH_TOTALS:
        # 1-byte literals and two-byte ` x` tokens: a token per literal, a token per ` x`
        k = total // 2
        docs = [L1 * 700 + b" x" * 300 + L1 * (k - 1000), b"", b" x" * 5, L1 * 7 + b" x" * (total - k - 12)]
        out.append(_case("stitch_total_%d" % total, "stitch", "sp_stitch", docs))
    # 301 unkept candidates (602 empty slots) between the long literal's token and the next segment's
    docs = [f(50) + b" " + LONG_A + b" " + f(700), L1 * 300 + b" x" * 40, LONG_A, f(20) + b" " + LONG_A[:200] + b" " + f(9)]
    out.append(_case("stitch_empty_run", "stitch", "sp_stitch", docs, allowed=(None, (L1, LONG_A))))
    # a refused document that holds candidates, between accepted ones: by a literal outside the allowed set, by a malformed byte
    docs = [f(60) + L1 * 3, L1 * 25 + b" " + f(30) + b" " + EOT + L1 * 4 + f(12), L1 + f(50) + L1, b"", L1 * 2]
    out.append(_case("stitch_refused_special", "stitch", "sp_stitch", docs, allowed=((L1, LONG_A, b"a"), None)))
    docs = [f(60) + L1 * 3, L1 * 25 + b" " + f(30) + b" " + L1 + b"\xff" + L1 * 4 + f(12), L1 + f(50) + L1, b"", L1 * 2]
    out.append(_case("stitch_refused_utf8", "stitch", "sp_stitch", docs, validate=True, invalid=(1,)))
    # the same without a candidate in the whole batch: a refused document has no tokens then either
    docs = [f(60), f(30) + b" " + EOT + f(12), b"", f(50)]
    out.append(_case("stitch_refused_special_no_candidate", "stitch", "sp_stitch", docs, allowed=((L1,),)))
    docs = [f(60), f(30) + b"\xff" + f(12), b"", f(50)]
    out.append(_case("stitch_refused_utf8_no_candidate", "stitch", "sp_stitch", docs, validate=True, invalid=(1,)))
    return out


@functools.lru_cache(maxsize=None)
def cases():
    out = _find_cases() + [_doc_boundary_case()] + _batch_end_cases() + _docs_cases() + _chain_cases() + _stitch_cases()
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


def by_name():
    return {c.name: c for c in cases()}


def combos(c):
    """(allowed, ordinary) of every run of the case."""
    return [(a, o) for a in c.allowed for o in c.modes]


# ---- the restatement's answer
_tok_cache = {}


def encode_ordinary(seg):
    if seg not in _tok_cache:
        _tok_cache[seg] = oracle().encode_ordinary(seg) if seg else []
    return _tok_cache[seg]


class _Cached:
    encode_ordinary = staticmethod(encode_ordinary)


def valid_utf8(doc):
    try:
        doc.decode("utf-8")
        return True
    except UnicodeDecodeError:
        return False


@functools.lru_cache(maxsize=None)
def _expected(name, allowed, ordinary):
    c = by_name()[name]
    lits = list(specials(c.enc))
    out = []
    for doc in c.docs:
        if c.validate and not valid_utf8(doc):
            out.append((-6, []))
            continue
        toks = special_ref.encode(_Cached, doc, amap(c.enc, allowed), lits, ordinary)
        out.append((-2, []) if toks is None else (0, toks))
    return tuple(out)


def expected(c, allowed, ordinary):
    """special_ref.encode of every document -> [(status, tokens)]: -2 where it refuses, -6 (validate) for malformed UTF-8."""
    return _expected(c.name, allowed, ordinary)


# ---- the model: the batch walked as the kernels walk it
def load_sim(path):
    L = C.CDLL(path)
    L.sim_special_batch.restype = C.c_int64
    L.sim_special_batch.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_char_p, C.c_void_p, C.c_int,
                                    C.c_int] + [C.c_void_p] * 5 + [C.c_int64] + [C.c_void_p] * 5
    L.sim_special_stitch.restype = C.c_int64
    L.sim_special_stitch.argtypes = [C.c_int64, C.c_int64] + [C.c_void_p] * 5 + [C.c_int64, C.c_int, C.c_int, C.c_int] + \
        [C.c_void_p] * 4 + [C.c_int64]
    return L


Model = collections.namedtuple("Model", "docs status cand_pos cand_len cand_lit cand_doc keep sub_off sub_lit sub_doc cnt tok_off total")
#   docs: the token list of every document (-1: a token whose source lies outside its sub-document)


def padded(c):
    """The batch's bytes as device text holds them: the pad of the case behind them, zeros to the next multiple of 16 plus 16."""
    text, doc_off = _pack(c.docs)
    n = len(text)
    return text + (c.pad + bytes(32))[:_round_up(n, 16) + 16 - n], doc_off, n


def model(sim, c, allowed, ordinary, mutant=0):
    buf, doc_off, n = padded(c)
    sp = specials(c.enc)
    lits = list(sp)
    ids = np.array(list(sp.values()), dtype=np.int32)
    off = np.zeros(len(lits) + 1, dtype=np.uint32)
    off[1:] = np.cumsum([len(x) for x in lits])
    al = np.array([1 if allowed is None or x in allowed else 0 for x in lits] + [0], dtype=np.uint8)
    nd, cap = len(c.docs), n + 16
    text = np.frombuffer(buf, dtype=np.uint8).copy()
    cpos, cdoc = np.zeros(cap, dtype=np.int64), np.zeros(cap, dtype=np.int64)
    clen, clit = np.zeros(cap, dtype=np.int32), np.zeros(cap, dtype=np.int32)
    keep = np.zeros(cap, dtype=np.uint8)
    ns_cap = nd + 2 * cap + 1
    first = np.zeros(max(nd, 1), dtype=np.int64)
    soff, sdoc = np.zeros(ns_cap, dtype=np.int64), np.zeros(ns_cap, dtype=np.int64)
    slit = np.full(ns_cap, -2, dtype=np.int32)
    status = np.zeros(max(nd, 1), dtype=np.int32)
    nc = sim.sim_special_batch(text.ctypes.data, n, doc_off.ctypes.data, nd, len(lits), off.ctypes.data, b"".join(lits), al.ctypes.data,
                               0 if ordinary else 1, mutant, cpos.ctypes.data, clen.ctypes.data, clit.ctypes.data, cdoc.ctypes.data,
                               keep.ctypes.data, cap, first.ctypes.data, soff.ctypes.data, slit.ctypes.data, sdoc.ctypes.data,
                               status.ctypes.data)
    assert nc >= 0
    n_sub = nd + 2 * nc
    raw = bytes(buf)
    if c.validate:
        for d, doc in enumerate(c.docs):
            if not valid_utf8(doc):
                status[d] = min(status[d], -6)
    seg_tok, seg_count = [], np.zeros(n_sub + 1, dtype=np.int64)
    for j in range(n_sub):
        toks = []
        if slit[j] == -1 and status[sdoc[j]] >= 0 and soff[j] < soff[j + 1] <= n:
            try:
                toks = encode_ordinary(raw[soff[j]:soff[j + 1]])
            except oracle_lib.OracleError:
                if mutant == 0:                # (only a wrong rule may cut a segment where the oracle refuses it)
                    raise
                toks = [-1]
        seg_tok.append(toks)
        seg_count[j] = len(toks)
    cnt = np.zeros(n_sub + 1, dtype=np.int64)
    tok_off = np.zeros(nd + 1, dtype=np.int64)
    tcap = int(seg_count.sum() + n_sub + 1)
    src_sub, src_idx = np.zeros(tcap, dtype=np.int64), np.zeros(tcap, dtype=np.int64)
    total = sim.sim_special_stitch(n_sub, nd, slit.ctypes.data, sdoc.ctypes.data, status.ctypes.data, seg_count.ctypes.data,
                                   first.ctypes.data, n, GT, GPER, mutant, cnt.ctypes.data, tok_off.ctypes.data, src_sub.ctypes.data,
                                   src_idx.ctypes.data, tcap)
    assert 0 <= total <= tcap
    seg_base = np.zeros(n_sub + 1, dtype=np.int64)
    np.cumsum(seg_count[:n_sub], out=seg_base[1:])
    flat = np.array([t for toks in seg_tok for t in toks] + [-1], dtype=np.int64)
    j, i = src_sub[:total], src_idx[:total]
    lit = slit[j]
    inside = (lit == -1) & (i >= 0) & (i < seg_count[j])
    tokens = np.where(lit >= 0, ids[np.maximum(lit, 0)], np.where(inside, flat[np.where(inside, seg_base[j] + i, len(flat) - 1)], -1))
    docs = [tokens[tok_off[d]:tok_off[d + 1]].tolist() if tok_off[d] <= tok_off[d + 1] else [-1] for d in range(nd)]
    return Model(docs, status[:nd].tolist(), cpos[:nc], clen[:nc], clit[:nc], cdoc[:nc], keep[:nc], soff[:n_sub + 1], slit[:n_sub],
                 sdoc[:n_sub], cnt, tok_off, int(total))


def wrong(sim, c, allowed, ordinary, mutant=0):
    """The documents on which the model (with a mutant) and the restatement disagree."""
    m = model(sim, c, allowed, ordinary, mutant)
    exp = expected(c, allowed, ordinary)
    return [d for d in range(len(c.docs)) if (m.status[d], m.docs[d]) != (exp[d][0], list(exp[d][1]))]


# ---- what a batch reaches, from the model's answer
def sweep_required(lit):
    return set(range(-len(lit) - 1, 2))


def sweep_reached(m, lits):
    """{(edge kind, literal): deltas}: candidate starts at edge + delta for lane (16), wave (1024 inside a block), block (4096)
    and the 8192 edges."""
    got = collections.defaultdict(set)
    for p, li in zip(m.cand_pos.tolist(), m.cand_lit.tolist()):
        lit = lits[li]
        for delta in range(-len(lit) - 1, 2):
            a = p - delta
            if a <= 0:
                continue
            if a % LANE == 0:
                got[(LANE, lit)].add(delta)
            if a % WAVE == 0 and a % BLOCK != 0:
                got[(WAVE, lit)].add(delta)
            if a % BLOCK == 0:
                got[(BLOCK, lit)].add(delta)
            if a % (2 * BLOCK) == 0:
                got[(2 * BLOCK, lit)].add(delta)
    return got


def chains(m):
    """The chains as (first, last) candidate index: a certain candidate and the uncertain ones behind it."""
    out, i, n = [], 0, len(m.keep)
    while i < n:
        j = i + 1
        while j < n and m.keep[j] != 1:
            j += 1
        if j - i > 1:
            out.append((i, j - 1))
        i = j
    return out


def longest_flat_run(m):
    """The longest run of equal cnt values (sub-documents without a token) with a token before and behind it."""
    cnt = m.cnt[:len(m.sub_lit) + 1]
    best, j = 0, 0
    while j < len(cnt):
        k = j
        while k + 1 < len(cnt) and cnt[k + 1] == cnt[j]:
            k += 1
        if cnt[j] > 0 and cnt[j] < m.total:
            best = max(best, k - j)               # k - j sub-documents hold no token
        j = k + 1
    return best
