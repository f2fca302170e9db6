"""Cases of the fill-in-the-middle rule (JTK_ENCODE_FIM) for the CPU tier (tests/test_fim_rules_cpu.py: the shim of the rule
header against tests/fim_ref.py) and the GPU tier (tests/test_fim_gpu.py).  Documents are bytes; rates are in units of 2^-32.
Seeds that force a cut to 0, to len or both cuts to one place are found by search with the restatement, which is cheap."""
import collections

import fim_ref as fr

Case = collections.namedtuple("Case", "name docs seed base fim_rate spm_rate")

ALWAYS = fr.ALWAYS
HALF = 1 << 31

PIZZA = "\U0001F355".encode()                # one 4-byte character
MIXED = [s.encode() for s in (
    "def f(x):\n    return x + 1\n", "hello world", "日本語のテキストです。", "naïve café — déjà vu", "a", "",
    "\U0001F355\U0001F600 pizza \U0001F355", "for (int i = 0; i < n; i++) { a[i] = b[i] * 2; }", "xéy", "١٢٣ ٤٥٦", "  \n\n\t  ",
    "it's we're they'll", "The quick brown fox jumps over the lazy dog.", "𝔘𝔫𝔦𝔠𝔬𝔡𝔢", "á̂̃b", "1234567890" * 3)]
CONT_ONLY = [b"\x80" * k for k in range(1, 9)] + [b"\xbf" * 5, b"a" + b"\x80" * 6, b"\x80" * 6 + b"z"]
LONE_LEADS = [b"abc\xe6", b"ab\xf0\x9f", b"\xc3", b"\xe6\x97", b"ok\xf0", b"\xf0\x9f\x8d", b"caf\xc3"]


def find_seed(doc, g, pred, start=0):
    """The first seed >= start for which pred(raw cut 0, raw cut 1, a, b) holds for `doc` at global index g."""
    for seed in range(start, start + 200000):
        p0, p1 = fr.raw_cut(seed, g, 0, len(doc)), fr.raw_cut(seed, g, 1, len(doc))
        a, b = fr.cuts_of(doc, seed, g)
        if pred(p0, p1, a, b):
            return seed
    raise AssertionError("no seed found")


def cases():
    out = []
    hello = b"hello world"
    n = len(hello)
    out.append(Case("mixed_psm", MIXED, 1, 0, ALWAYS, 0))
    out.append(Case("mixed_spm", MIXED, 2, 0, ALWAYS, ALWAYS))
    out.append(Case("mixed_half", MIXED * 3, 3, 0, HALF, HALF))
    out.append(Case("empty_documents", [b"", b"", b"x", b"", b""], 4, 0, ALWAYS, HALF))
    out.append(Case("no_documents", [], 4, 0, ALWAYS, HALF))
    out.append(Case("one_byte_documents", [bytes([c]) for c in b"abcdefgh \n"] * 4, 5, 0, ALWAYS, HALF))
    out.append(Case("one_four_byte_character", [PIZZA] * 64, 6, 0, ALWAYS, HALF))
    out.append(Case("continuation_bytes_only", CONT_ONLY * 6, 7, 0, ALWAYS, HALF))
    out.append(Case("lone_lead_bytes_at_the_end", LONE_LEADS * 6, 8, 0, ALWAYS, HALF))
    out.append(Case("cut_forced_to_0", [hello], find_seed(hello, 0, lambda p0, p1, a, b: a == 0 and b not in (0, n)), 0, ALWAYS, 0))
    out.append(Case("cut_forced_to_len", [hello], find_seed(hello, 0, lambda p0, p1, a, b: b == n and a not in (0, n)), 0, ALWAYS, ALWAYS))
    out.append(Case("both_cuts_at_0", [hello], find_seed(hello, 0, lambda p0, p1, a, b: a == 0 and b == 0), 0, ALWAYS, 0))
    out.append(Case("both_cuts_at_len", [hello], find_seed(hello, 0, lambda p0, p1, a, b: a == n and b == n), 0, ALWAYS, ALWAYS))
    out.append(Case("cuts_0_and_len", [hello], find_seed(hello, 0, lambda p0, p1, a, b: a == 0 and b == n), 0, ALWAYS, HALF))
    out.append(Case("cuts_equal_inside", [hello], find_seed(hello, 0, lambda p0, p1, a, b: a == b and 0 < a < n), 0, ALWAYS, 0))
    out.append(Case("cuts_equal_by_snapping", [b"ab" + PIZZA + b"cd"],
                    find_seed(b"ab" + PIZZA + b"cd", 0, lambda p0, p1, a, b: p0 != p1 and a == b == 2), 0, ALWAYS, ALWAYS))
    for fname, f in (("0", 0), ("1", 1), ("always", ALWAYS)):
        for sname, s in (("0", 0), ("1", 1), ("always", ALWAYS)):
            out.append(Case("rates_%s_%s" % (fname, sname), MIXED, 9, 0, f, s))
    out.append(Case("doc_index_base", MIXED, 10, 12345678901, HALF, HALF))
    out.append(Case("doc_index_base_top_bit", MIXED, 11, (1 << 62) + 5, ALWAYS, HALF))
    out.append(Case("large_seed", MIXED, (1 << 64) - 3, 7, ALWAYS, HALF))
    return out


TILE = 1024                                  # cells per gather tile (JTK_FIM_TILE; the CPU tier checks it against the header)


def gather_edge_case(count, sentinel, cell, spm):
    """One long document whose stitched stream crosses a gather-tile boundary, after one-byte documents that shift it so that
    its `sentinel` ("suf" or "mid") lies in cell `cell` (1023: the last of a tile, 1024: the first of the next) of the
    result.  count(bytes) -> tokens of encodeOrdinary, from the oracle.  The long document keeps its global index (and so its
    cuts) whatever the number of fillers: doc_index_base moves instead."""
    G = 5000
    doc = (" a b c" * 400).encode()
    spm_rate = ALWAYS if spm else 0
    for seed in range(100, 400):
        kind, a, b = fr.transform(doc, seed, G, HALF, spm_rate)
        if kind == fr.NONE or not 0 < a < b < len(doc):
            continue
        c0, c1, c2 = count(doc[:a]), count(doc[a:b]), count(doc[b:])
        # the sentinel's offset in the document's stream
        at = {("suf", False): 1 + c0, ("mid", False): 2 + c0 + c2, ("suf", True): 1, ("mid", True): 2 + c2}[(sentinel, spm)]
        total, k = 0, 0
        while total + at < cell and k < 2000:                  # fillers G - 1, G - 2, ...: 1 token untouched, 4 cut
            k += 1
            total += 1 + (3 if fr.kind_of(seed, G - k, 1, HALF, spm_rate) else 0)
        if total + at == cell and total + 3 + c0 + c1 + c2 > TILE:
            return Case("gather_%s_%d_%s" % (sentinel, cell, "spm" if spm else "psm"), [b"a"] * k + [doc, b"tail"], seed, G - k, HALF, spm_rate)
    raise AssertionError("no seed found")


def gather_edge_cases(count):
    return [gather_edge_case(count, s, c, spm) for s in ("suf", "mid") for c in (TILE - 1, TILE) for spm in (False, True)]


def tiny_documents(n=3000):
    """n documents of one to three bytes: many documents per gather tile, empty parts everywhere."""
    alphabet = [b"a", b"b ", b" c", b"\xc3\xa9", b"xyz", b"\xe6\x97\xa5", b"1", b"\n\n", b"it", b"\xe2\x82"]
    return Case("tiny_documents", [alphabet[(d * 7 + d // 10) % len(alphabet)] for d in range(n)], 21, 0, ALWAYS, HALF)


def sentinel_cells(ref, ids):
    """Which cells of a reference result hold a sentinel."""
    import numpy as np
    return np.isin(ref.tokens, np.array(ids, dtype=np.int32))


def zero_token_parts_at_tile_starts():
    """One-byte documents, half of them cut: two of a cut document's three parts are empty, so sentinels follow each other.  The
    seed is searched so that at two tile starts at least the cell and the one before it are both sentinels: an empty part lies
    exactly on the tile boundary.  (One byte is one token in every shipped table, which the search relies on and the tiers
    check against the oracle.)"""
    docs = [b"a"] * 1500
    ids = (-1, -2, -3)
    for seed in range(300):
        ref = fr.encode_batch(lambda b: [0] * len(b), docs, seed, 0, HALF, HALF, ids)
        sent = sentinel_cells(ref, ids)
        starts = [t for t in range(TILE, len(sent), TILE) if sent[t] and sent[t - 1]]
        if len(starts) >= 2:
            return Case("zero_token_parts_at_tile_starts", docs, seed, 0, HALF, HALF)
    raise AssertionError("no seed found")


ALL_EDGES = {"kind0", "psm", "spm", "cut0", "cutlen", "equal", "snap1", "snap2", "snap3", "limit", "lands_on_continuation",
             "empty_prefix", "empty_middle", "empty_suffix", "empty_doc"}


def edges_reached(case):
    got = set()
    for d, doc in enumerate(case.docs):
        g = case.base + d
        kind, a, b = fr.transform(doc, case.seed, g, case.fim_rate, case.spm_rate)
        got.add(("kind0", "psm", "spm")[kind])
        if not doc:
            got.add("empty_doc")
        if kind == fr.NONE:
            continue
        n = len(doc)
        got |= {e for e, hit in (("cut0", a == 0), ("cutlen", b == n), ("equal", a == b), ("empty_prefix", a == 0),
                                 ("empty_middle", a == b), ("empty_suffix", b == n)) if hit}
        for k in (0, 1):
            p = fr.raw_cut(case.seed, g, k, n)
            q = fr.snap(doc, p)
            if p - q:
                got.add("snap%d" % (p - q))
            if p - q == 3 and 0 < q < n and 0x80 <= doc[q] <= 0xBF:
                got |= {"limit", "lands_on_continuation"}
    return got
