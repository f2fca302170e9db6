"""The rule of jtk_batch_phrase_hits (include/jtokkit_amd.h) in plain Python -- bytes.startswith at every position, unicodedata for
the boundary, a dict for the distinct phrases; it shares no code with the product -- and the cases both tiers of its tests run,
each on an edge of the rule or of the kernel's partition (a granule of 16 start positions, a wave's 1024, a tile of 4096)."""
import collections
import random
import unicodedata

import numpy as np

OUTS = (("group_mask", np.uint32), ("n_hits", np.int32), ("first_hit", np.int64), ("first_which", np.int32), ("n_hit_units", np.int32),
        ("unit_mask", np.uint32))
G, WAVE, TILE, MAXLEN = 16, 1024, 4096, 64


def fold(b):
    return bytes(c + 32 if 65 <= c <= 90 else c for c in b)


def is_word(b):
    """Is the UTF-8 of one character a word character ('_', L* or N*); what does not decode to one character is not."""
    try:
        ch = b.decode("utf-8")
    except UnicodeDecodeError:
        return False
    return len(ch) == 1 and (ch == "_" or unicodedata.category(ch)[0] in "LN")


def bounded(x, p, n):
    """No word character ends at p - 1 (found over at most three continuation bytes, inside the document) or starts at p + n."""
    j = p - 1
    while p - j <= 3 and j > 0 and x[j] & 0xC0 == 0x80:
        j -= 1
    q = p + n
    return not (p > 0 and is_word(x[j:p])) and (q >= len(x) or not is_word(x[q:q + (1 if x[q] < 0xC0 else 2 if x[q] < 0xE0 else 3 if x[q] < 0xF0 else 4)]))


def hits(docs, status, phrases, fold_ascii=False, word_bounds=False, units=None):
    """docs: bytes each; phrases: (bytes, group) pairs, equal ones (after folding) one phrase with the OR of their groups and the
    smallest index; units: (unit_off [n + 1], begin, end) in batch positions, or None.  A dict of arrays by the names of OUTS."""
    by_first = {}
    for i, (ph, g) in enumerate(phrases):
        e = by_first.setdefault(ph[0] | (32 if fold_ascii and 65 <= ph[0] <= 90 else 0), {}).setdefault(fold(ph) if fold_ascii else ph, [0, i])
        e[0] |= 1 << g
    unit_off, begin, end = units if units is not None else (np.zeros(len(docs) + 1, np.int64), [], [])
    out = {name: np.full(len(begin) if name == "unit_mask" else len(docs), -1 if name.startswith("first") else 0, dtype=dt) for name, dt in OUTS}
    base = 0
    for d, doc in enumerate(docs):
        x = fold(doc) if fold_ascii else doc
        count = 0
        for p in range(len(x) if status[d] >= 0 else 0):
            for ph, (mask, idx) in by_first.get(x[p], {}).items():
                if not x.startswith(ph, p) or (word_bounds and not bounded(x, p, len(ph))):
                    continue
                count += 1
                out["group_mask"][d] |= mask
                if out["first_hit"][d] < 0 or (out["first_hit"][d] == p and idx < out["first_which"][d]):
                    out["first_hit"][d], out["first_which"][d] = p, idx
                for u in range(unit_off[d], unit_off[d + 1]):
                    if begin[u] <= base + p and base + p + len(ph) <= end[u]:
                        out["unit_mask"][u] |= mask
        out["n_hits"][d] = min(count, 2 ** 31 - 1)
        out["n_hit_units"][d] = np.count_nonzero(out["unit_mask"][unit_off[d]:unit_off[d + 1]])
        base += len(doc)
    return out


def pack(docs):
    doc_off = np.zeros(len(docs) + 1, dtype=np.int64)
    np.cumsum([len(x) for x in docs], out=doc_off[1:])
    return np.frombuffer(b"".join(docs) + b"\0", dtype=np.uint8)[:-1], doc_off


# ---- the cases: documents, (phrase, group) pairs, the statuses the encode leaves and its route
Case = collections.namedtuple("Case", "name docs phrases status route")
LONG = bytes(range(0x30, 0x30 + MAXLEN - 2)) + b"pq"            # 64 bytes: '0' .. 'm', then "pq"
NEIGHBOURS = ("x", "7", "_", " ", "é", "中", "\U0001D400", "“", "\U0001F600")   # letter, digit, '_', blank, L of 2 / 3 / 4 bytes, Pi, So


def plant(size, items):
    """`size` bytes of ". " with every (position, bytes) item at its byte position."""
    out = bytearray((b". " * size)[:size])
    for pos, s in items:
        out[pos:pos + len(s)] = s
    assert len(out) == size
    return bytes(out)


def case(name, docs, phrases, status=None, route="ordinary"):
    enc = lambda s: s.encode() if isinstance(s, str) else s
    return Case(name, [enc(d) for d in docs], [(enc(p), g) for p, g in phrases], status or [0] * len(docs), route)


def cases():
    rng = random.Random(7)
    six = [("needle", 0), ("hay stack", 1), ("pin", 2), ("a", 3), ("zz top", 4), ("thread", 5)]
    far = [("".join(rng.choice("ABCDEFGHIJKLMNOPQRSTUVWXYZ") for _ in range(8)), 31) for _ in range(5000)]      # (none occurs in the text)
    placed = plant(3 * TILE, [(100, b"needle"), (TILE - 3, b"hay stack"), (TILE + 500, b"pin"), (2 * TILE - 1, b"zz top"), (3 * TILE - 6, b"thread")])
    # the character before "cat": 2 bytes across byte 4096 of the batch, 4 bytes across 8192, 3 bytes that end a tile ("cat" on the next one's first byte)
    before = plant(3 * TILE + 3, [(TILE - 1, "écat".encode()), (2 * TILE - 2, "\U0001D400cat".encode()), (3 * TILE - 3, "中cat".encode())])
    assert [before.find(b"cat", k * TILE) for k in (1, 2, 3)] == [TILE + 1, 2 * TILE + 2, 3 * TILE] and before[TILE - 1] == 0xC3 and before[2 * TILE - 2] == 0xF0
    lines = ("see our terms of use here\n  javascript:void(0)  \nline one \t\nlorem\nipsum\n\n para two   \nuse\ncookies\n\n\n{x}", "", "no hit\n", "cookie policy")
    return [
        # hits that start on a tile's last byte and the next one's first; 64 bytes that end one byte into the next tile, on the last staged byte, on the text's last
        case("tile_edges", [plant(3 * TILE, [(TILE - 63, LONG + b"r"), (2 * TILE - 1, LONG), (3 * TILE - MAXLEN, LONG)])], [(LONG, 0), ("pq", 1), ("qr", 2)]),
        case("character_before_across_tile_edge", [before], [("cat", 0), ("at", 1)]),
        case("document_edges", ["..needle", "nee", "dle..", "", "n", "needle", "e", "needleneedle", "x <|endoftext|> needle", "needl"],
             [("needle", 0), ("n", 1), ("dle..", 2)], [0] * 8 + [-1, 0], "encode"),
        case("granule_and_wave_edges", [plant(2 * WAVE, [(p, b"needle") for p in (G - 1, G, WAVE - 1, WAVE)])], [("needle", 5)]),
        case("phrase_shapes", ["abcd ab abc abx dup # ## tea ten team te t", "teamabcd#dup"],
             [("ab", 0), ("abc", 1), ("abcd", 2), ("dup", 3), ("dup", 7), ("#", 8), ("tea", 9), ("ten", 10), ("team", 31), ("dup", 3)]),
        case("empty_set", ["abcd ab", ""], []),
        case("fold", ["A Z @ [ É a z ` { é AZ@[É az`{é"], [(c, i) for i, c in enumerate("AZ@[Éaz`{é")] + [("Az", 20), ("aZ@", 21)]),
        case("neighbours", ["cat"] + [a + "cat" + b for a in NEIGHBOURS for b in (" ", a)] + [" cat" + b for b in NEIGHBOURS], [("cat", 0), ("at", 1)]),
        case("dense_one_document", ["a" * 10000], [("a", 0), ("aa", 1)]),
        case("dense_100_documents", ["a" * 100] * 100, [("a", 0), ("aa", 1)]),
        case("table_in_lds", [placed], six),
        case("table_in_global", [placed], six + far),
        case("units", lines, [("terms of use", 0), ("cookie policy", 0), ("use\ncookies", 0), ("javascript", 1), ("lorem\nipsum", 2), ("{", 3), (" \t", 4), ("  ", 5)]),
    ]


CASES = {c.name: c for c in cases()}
