"""The case set of the character-position tests (CPU and GPU tier): lists of documents (bytes) laid out so that the edges of the
index of jtk_charpos_rules.h -- 64-byte blocks, 4096-byte superblocks, the 16-byte granule of the last load -- fall where they
can go wrong.  edges_reached() names what a list of documents reaches; the tests assert on it."""
import random

BLOCK, SUPER = 64, 4096

_POOLS = {1: "abcdefghij klmnop,.\n", 2: "éñöüßжиΩλ", 3: "日本語のテキスト書€‍", 4: "\U0001F600\U0001F355\U0001D11E\U00020000\U0001F469"}


def fill(rng, n_bytes, widths=(1, 1, 2, 3, 4)):
    """Exactly n_bytes of well-formed text that mixes characters of the given byte widths."""
    out, left = [], n_bytes
    while left > 0:
        w = rng.choice([x for x in widths if x <= left] or [1])
        out.append(rng.choice(_POOLS[w]))
        left -= w
    b = "".join(out).encode("utf-8")
    assert len(b) == n_bytes
    return b


def edge_docs():
    """Well-formed documents whose ends and 4-byte characters sit on block and superblock edges (when the list starts at a
    superblock edge of the batch): 17,455 bytes, more than four superblocks and a ragged tail."""
    rng = random.Random(5)
    g = "\U0001F600".encode("utf-8")
    docs = [fill(rng, 62) + g + fill(rng, 62)]                                  # [0, 128): a 4-byte character across byte 64
    docs.append(fill(rng, 128))                                                 # [128, 256): block edge to block edge
    docs.append(fill(rng, SUPER - 256))                                         # [256, 4096): block edge to superblock edge
    docs.append(fill(rng, SUPER - 2) + g + fill(rng, 3 * BLOCK - 2))            # [4096, 8384): ... across byte 8192
    docs.append(fill(rng, 3 * SUPER - 8384, widths=(3,)))                       # [8384, 12288): 3-byte characters only
    docs.append(fill(rng, SUPER - 8, widths=(4,)) + fill(rng, 8, widths=(2,)))  # [12288, 16384): superblock edge to superblock edge
    docs.append(b"")
    docs.append(fill(rng, 1071))                                                # the ragged tail: n_bytes % 16 == 15
    assert sum(len(d) for d in docs) == 4 * SUPER + 1071
    return docs


def script_docs():
    return [t.encode("utf-8") for t in (
        "plain ASCII text, nothing else.", "", "héllo wörld, señor: ça va? Ωμέγα", "日本語のテキストを書きます。", "a\U0001F600b\U0001F355\U0001D11E c",
        "\U0001F469‍\U0001F373" * 5, "x", "é", "語", "\U00020000", "mixed: aé語\U0001F600" * 9, "")]


def malformed_docs():
    return [b"\x80\x80abc",                                  # starts with continuation bytes
            b"abc\xe6\x97",                                   # a 3-byte character cut off at the document's end
            b"ab\xf0",                                        # a lead byte alone at the end
            b"x" + b"\x80" * 7 + b"y" + b"\xbf" * 4,          # runs of more than 3 continuation bytes, one up to the end
            bytes(range(0xF8, 0x100)) + b"z",                 # bytes that are never part of UTF-8
            b"\xc0\xaf\xed\xa0\x80",                          # overlong form, a surrogate
            b"",
            b"tail \xf0\x9f",                                 # a 4-byte character cut by a document edge ...
            b"\x98\x80 head",                                 # ... whose rest starts the next document
            b"\x80",
            b"\xf4\x90\x80\x80 \xe2\x82"]


def cases():
    """(name, documents).  "edges" starts at byte 0, so its documents sit on the index's edges as edge_docs() lays them out."""
    e, s, m = edge_docs(), script_docs(), malformed_docs()
    return [("edges", e), ("scripts", s), ("malformed", m), ("all", e + m + s), ("one_empty", [b""]), ("none", []),
            ("whole_granules", [fill(random.Random(9), 32)])]


def edges_reached(docs):
    """What a batch of documents reaches, as a set of names."""
    out = set()
    text = b"".join(docs)
    if len(text) % 16:
        out.add("n_bytes % 16 != 0")
    pos = 0
    for d in docs:
        a, e = pos, pos + len(d)
        pos = e
        if not d:
            out.add("empty document")
            continue
        if a % BLOCK == 0 and e % BLOCK == 0 and a % SUPER and e % SUPER:
            out.add("document from block edge to block edge")
        if a % SUPER == 0 and e % SUPER == 0:
            out.add("document from superblock edge to superblock edge")
        if (d[0] & 0xC0) == 0x80:
            out.add("document starts with a continuation byte")
        if d[-1] >= 0xC0 or (len(d) >= 2 and d[-2] >= 0xE0 and (d[-1] & 0xC0) == 0x80):
            out.add("lead byte cut off at a document's end")
        if any(x >= 0xF8 for x in d):
            out.add("bytes 0xF8..0xFF")
        run = 0
        for x in d:
            run = run + 1 if (x & 0xC0) == 0x80 else 0
            if run > 3:
                out.add("more than 3 continuation bytes in a row")
        try:
            s = d.decode("utf-8")
        except UnicodeDecodeError:
            continue
        q = a
        for ch in s:
            w = len(ch.encode("utf-8"))
            out.add("%d-byte characters" % w)
            if w == 4 and q // BLOCK != (q + 3) // BLOCK:
                out.add("4-byte character across a block edge")
            if w == 4 and q // SUPER != (q + 3) // SUPER:
                out.add("4-byte character across a superblock edge")
            q += w
    if len(text) > 4 * SUPER and len(text) % SUPER:
        out.add("more than 4 superblocks and a ragged tail")
    return out


ALL_EDGES = {"n_bytes % 16 != 0", "empty document", "document from block edge to block edge",
             "document from superblock edge to superblock edge", "document starts with a continuation byte",
             "lead byte cut off at a document's end", "bytes 0xF8..0xFF", "more than 3 continuation bytes in a row",
             "1-byte characters", "2-byte characters", "3-byte characters", "4-byte characters",
             "4-byte character across a block edge", "4-byte character across a superblock edge",
             "more than 4 superblocks and a ragged tail"}
