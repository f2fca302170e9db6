"""The case set of the UTF-8 validation tests (CPU and GPU tier).  A case is a batch: a list of documents (bytes).  The batches
cover every byte class of the rule (jtokkit_amd/csrc/jtk_validate_rules.h) at both of its ends, every row of Unicode Table 3-7
cut at every length in every way a document can cut it, and they lay sequences on the edges of the validator's partition --
k_validate_utf8 takes one byte per lane, so its look-back p-1..p-3 and look-ahead p+1..p+3 cross wave, workgroup and docmask
word edges -- and on the chunk edges of a job larger than one chunk.  edges_reached() names what a batch reaches; the tests
assert on it.  Built on the CPU, seeded."""
import functools
import itertools
import random

import numpy as np

from utf16_cases import TABLE_3_7

# ---- the partition of k_validate_utf8 (jtk_kernels.hip) and of the job above it (jtk_abi.cpp)
LANE = 1                      # bytes per lane
WAVE = 64                     # bytes per wave
WORKGROUP = 256               # bytes per workgroup
DOCMASK_WORD = 64             # document-start bits per docmask word
TILE = 2048                   # a chunk's text origin is rounded down to a tile: `lead` = chunk start - origin
MIN_CHUNK = 65536             # the smallest JTK_OPT_CHUNK_BYTES / JTK_OPT_HOST_CHUNK_BYTES
TINY_JOB = 128 << 10          # host jobs up to this size are staged in one copy
SMALL_JOB = 1 << 20           # single-chunk jobs up to this size answer in one copy

CLASS_VALUES = [0x00, 0x7F, 0x80, 0x8F, 0x90, 0x9F, 0xA0, 0xBF, 0xC0, 0xC1, 0xC2, 0xDF, 0xE0, 0xE1, 0xEC, 0xED, 0xEE, 0xEF, 0xF0, 0xF1,
                0xF3, 0xF4, 0xF5, 0xFF]
N_PRODUCT = sum(len(CLASS_VALUES) ** n for n in (1, 2, 3, 4))            # 346,200 documents
N_PRODUCT_GOOD = 1926                                                    # of them well-formed

G4 = "\U0001F600".encode("utf-8")                                        # f0 9f 98 80
G3 = "日".encode("utf-8")                                                 # e6 97 a5
B4 = b"\xf4\x90\x80\x80"                                                 # above U+10FFFF: every byte of it is bad
ITEMS = (("good4", G4), ("good3", G3), ("bad4", B4))
_POOLS = {1: "abcdefghij klmnop,.\n", 2: "éñöüßжиΩλ", 3: "日本語のテキスト書€", 4: "\U0001F600\U0001F355\U0001D11E\U00020000"}
EMPTY_RUNS = (1, 2, 65)
CONT_RUNS = (2, 3, 4, 5, 7)
RUN_HEADS = (("ascii", b"a"), ("lead2", b"\xc3"), ("lead3", b"\xe4"), ("lead4", b"\xf1"))


def pack(docs):
    """(text uint8 [n_bytes], doc_off int64 [n_docs + 1]) of a batch."""
    doc_off = np.zeros(len(docs) + 1, dtype=np.int64)
    if docs:
        np.cumsum([len(d) for d in docs], out=doc_off[1:])
    return np.frombuffer(b"".join(docs), dtype=np.uint8), doc_off


# ---- every sequence of 1 to 4 class values, each a document
@functools.lru_cache(maxsize=None)
def class_product():
    return [bytes(t) for n in (1, 2, 3, 4) for t in itertools.product(CLASS_VALUES, repeat=n)]


@functools.lru_cache(maxsize=None)
def class_product_slice():
    """Every document of up to 3 values and every 17th of those of 4 (17 and 24 are coprime: the last value takes every class):
    under 128 KiB, for the tiny-job path."""
    docs = class_product()
    short = sum(len(CLASS_VALUES) ** n for n in (1, 2, 3))
    out = docs[:short] + docs[short::17]
    assert sum(len(d) for d in out) <= TINY_JOB
    return out


# ---- every row of Table 3-7, whole and cut
def table_cuts():
    """Each row whole; cut after k = 1..len-1 bytes by the document's end, by a following lead, by a following ASCII byte, by a
    document boundary (head in one document, tail in the next) and by the same with runs of empty documents in between."""
    out = []
    for c in TABLE_3_7:
        out.append(c)
        for k in range(1, len(c)):
            out += [b"a" + c[:k], c[:k] + "é".encode("utf-8") + b"z", c[:k] + b"z"]
            out += [b"a" + c[:k], c[k:] + b"z"]
            for n in EMPTY_RUNS:
                out += [b"a" + c[:k]] + [b""] * n + [c[k:] + b"z"]
    return out


def batch_end_cuts():
    """One batch per row and k: the row cut after k bytes by the end of the batch."""
    return [[b"ok", b"a" + c[:k]] for c in TABLE_3_7 for k in range(1, len(c))]


# ---- the malformed kinds
def bad_kinds():
    out = [b"\xc0\xaf", b"\xc1\xbf", b"\xe0\x80\x80", b"\xe0\x9f\xbf", b"\xed\xa0\x80", b"\xed\xbf\xbf", b"\xf0\x80\x80\x80", b"\xf0\x8f\xbf\xbf",
           b"\xf4\x90\x80\x80"]
    out += [bytes([x]) for x in range(0xF5, 0x100)] + [bytes([x]) + b"\x80\x80\x80" for x in range(0xF5, 0x100)]
    out.append(b"\x80abc")                                               # a stray continuation byte at a document start
    # runs of continuation bytes: behind an ASCII byte all are stray; behind a lead the first len - 1 are its own (the 3- and
    # 4-byte leads with exactly 2 and 3 are well-formed) and the rest must not find it: the look-back limit and `len > k`
    out += [head + b"\x80" * n for _, head in RUN_HEADS for n in CONT_RUNS]
    out.append(G4 + b"\x80")                                             # a good 4-byte character directly followed by one
    return out


# ---- sequences on the partition's edges
class _Layout:
    """Documents built at known batch positions; the fillers are well-formed characters of 1 to 4 bytes."""

    def __init__(self, seed):
        self.docs, self.cur, self.pos, self.rng = [], b"", 0, random.Random(seed)

    def put(self, b):
        self.cur += b
        self.pos += len(b)

    def fill_to(self, p):
        assert p >= self.pos, (p, self.pos)
        while self.pos < p:
            w = self.rng.choice([x for x in (1, 1, 1, 2, 3, 4) if x <= p - self.pos])
            self.put(self.rng.choice(_POOLS[w]).encode("utf-8"))

    def end(self):
        self.docs.append(self.cur)
        self.cur = b""


def edge_layout():
    """One batch.  Every item of ITEMS with each of its bytes in turn as the first byte of a wave (= of a docmask word) and of a
    workgroup, each placement closing a document of its own; document starts at bit 0 and at bit 63 of a docmask word directly
    before and directly after every item; an item as the first bytes and a cut one as the last bytes.  The positions count from
    the batch's start: in a longer batch this list comes first."""
    L = _Layout(17)
    L.put(G4); L.fill_to(40); L.end()                                    # the very first bytes of the batch
    base = 2 * WORKGROUP
    for _, item in ITEMS:
        for j in range(len(item)):
            for edge in (base + 3 * WAVE, base + 2 * WORKGROUP):         # a wave edge inside a workgroup; a workgroup edge
                L.fill_to(edge - j); L.put(item); L.end()
            base += 3 * WORKGROUP                                        # (three workgroups per byte of an item)
    for _, item in ITEMS:
        for bit in (0, DOCMASK_WORD - 1):
            base = (L.pos + 2 * DOCMASK_WORD) // DOCMASK_WORD * DOCMASK_WORD
            L.fill_to(base + bit); L.end()                               # a document start at `bit`, the item directly after it
            L.put(item); L.put(b"z"); L.end()
            base += 2 * DOCMASK_WORD
            L.fill_to(base + bit - len(item)); L.put(item); L.end()      # the item directly before a document start at `bit`
            L.put(b"y")
    end = L.pos + 300
    L.fill_to(end + (1 if (end + 2) % WAVE == 0 else 0)); L.put(G4[:2]); L.end()     # a cut character; a ragged last wave
    return L.docs


def small_batches():
    """Batches whose first or last bytes are the case: every item as the very first bytes, whole as the very last bytes, and cut
    to its first 1, 2 and 3 bytes by the end of the batch; the batches of one byte; the rows of Table 3-7 cut by the end of the
    batch."""
    out = []
    for _, item in ITEMS:
        out.append([item + b" tail", b"next"])
        out.append([b"head", b"x" + item])
        out += [[b"head", b"x" + item[:k]] for k in (1, 2, 3)]
    out += [[b"\x41"], [b"\x80"], [b"\xc3"], [b"\xf0"]]
    return out + batch_end_cuts()


# ---- sequences on chunk edges
def host_chunk_starts(doc_off, cb):
    """First documents of the chunks of a host-input job (plan_host_chunks, jtk_abi.cpp): the first document at or after the
    last chunk's start + cb, unless less than a quarter chunk is left."""
    n_bytes = int(doc_off[-1])
    starts, nxt = [0], cb
    for d in range(len(doc_off) - 1):
        if doc_off[d] >= nxt and d > starts[-1] and n_bytes - doc_off[d] > cb // 4:
            starts.append(d)
            nxt = int(doc_off[d]) + cb
    return starts


def device_chunk_starts(doc_off, cb):
    """The same for device input (plan_device_chunks, k_plan_chunks): the first document at or after c * cb, for a batch of more
    than one and a quarter chunks."""
    n_bytes, n_docs = int(doc_off[-1]), len(doc_off) - 1
    starts = [0]
    if n_bytes > cb + cb // 4 and n_docs > 1:
        for c in range(1, (n_bytes + cb - 1) // cb):
            d = int(np.searchsorted(doc_off[:n_docs], c * cb, side="left"))
            if d > starts[-1] and d < n_docs:
                starts.append(d)
    return starts


def chunk_layout(chunk_bytes=MIN_CHUNK):
    """About 4 chunks of filler documents of a few hundred bytes, laid out so that the host and the device plan cut it at the same
    three documents:
      boundary 1, at chunk_bytes exactly (a tile multiple: lead == 0): a good 4-byte character ends exactly at it;
      boundary 2, inside a tile (lead > 0): the chunk's last document ends in E4 B8, the next chunk's first begins with AD;
      boundary 3, inside a tile: the next chunk's first document is empty and the one after it starts with 80."""
    cb = chunk_bytes
    L = _Layout(29)

    def fill_docs(p):
        while p - L.pos > 700:
            L.fill_to(L.pos + L.rng.randrange(150, 500)); L.end()
        L.fill_to(p)
    fill_docs(cb - 4); L.put(G4); L.end()                                # ... ends at cb
    L.put(b"first of chunk 1 "); L.fill_to(cb + 200); L.end()
    fill_docs(2 * cb - 100); L.fill_to(2 * cb + 775); L.put(b"\xe4\xb8"); L.end()    # straddles 2 cb; ends at 2 cb + 777
    L.put(b"\xad tail of the cut character"); L.end()
    fill_docs(3 * cb - 100); L.fill_to(3 * cb + 777 + 500); L.end()      # straddles 3 cb and (start of chunk 2) + cb
    L.end()                                                              # the empty first document of chunk 3
    L.put(b"\x80 stray"); L.end()
    fill_docs(4 * cb - 3000); L.end()
    return L.docs


# ---- what a batch reaches
def _cut_names():
    return {"%s cut after %d by %s" % (c.hex(), k, how) for c in TABLE_3_7 for k in range(1, len(c))
            for how in ("a document end", "a lead", "an ASCII byte", "a document boundary", "the end of the batch")
            + tuple("%d empty documents" % n for n in EMPTY_RUNS)}


def edges_reached(docs, chunk_bytes=MIN_CHUNK):
    out = set()
    text = b"".join(docs)
    n = len(text)
    starts, pos = [], 0
    for d in docs:
        starts.append(pos)
        pos += len(d)
    start_set = set(starts) | {n}
    # the class product
    if len(docs) >= N_PRODUCT:
        # (a batch this long is asked for this alone: the other edges are those of the smaller batches)
        if set(class_product()) <= set(docs):
            out.add("every sequence of 1 to 4 class values")
        if n > SMALL_JOB:
            out.add("more than a small job")
        return out
    if 3 * WAVE < n <= TINY_JOB and set(class_product_slice()) <= set(docs):
        out.add("a slice of the class product as a tiny job")
    # Table 3-7
    for i, s in enumerate(docs):
        for c in TABLE_3_7:
            if c in s:
                out.add("%s whole" % c.hex())
            for k in range(1, len(c)):
                if s.endswith(c[:k]) and (len(s) == k or s[-k - 1] < 0x80):
                    out.add("%s cut after %d by a document end" % (c.hex(), k))
                    if i == len(docs) - 1:
                        out.add("%s cut after %d by the end of the batch" % (c.hex(), k))
                    j = i + 1
                    while j < len(docs) and not docs[j]:
                        j += 1
                    if j < len(docs) and docs[j].startswith(c[k:]):
                        out.add("%s cut after %d by %s" % (c.hex(), k, "a document boundary" if j == i + 1 else "%d empty documents" % (j - i - 1)))
                if s.startswith(c[:k] + b"\xc3"):
                    out.add("%s cut after %d by a lead" % (c.hex(), k))
                if s.startswith(c[:k] + b"z"):
                    out.add("%s cut after %d by an ASCII byte" % (c.hex(), k))
    # the malformed kinds
    for s in docs:
        for bad, name in ((b"\xc0\xaf", "C0 AF"), (b"\xc1\xbf", "C1 BF"), (b"\xe0\x80\x80", "E0 80 80"), (b"\xe0\x9f\xbf", "E0 9F BF"),
                          (b"\xed\xa0\x80", "ED A0 80"), (b"\xed\xbf\xbf", "ED BF BF"), (b"\xf0\x80\x80\x80", "F0 80 80 80"),
                          (b"\xf0\x8f\xbf\xbf", "F0 8F BF BF"), (b"\xf4\x90\x80\x80", "F4 90 80 80")):
            if s == bad:
                out.add(name)
        if len(s) == 1 and s[0] >= 0xF5:
            out.add("%02X alone" % s[0])
        if len(s) == 4 and s[0] >= 0xF5 and s[1:] == b"\x80\x80\x80":
            out.add("%02X and three continuation bytes" % s[0])
        if s[:1] == b"\x80" and len(s) > 1 and s[1] < 0x80:
            out.add("a stray continuation byte at a document start")
        for name, head in RUN_HEADS:
            for r in CONT_RUNS:
                if s == head + b"\x80" * r:
                    out.add("%d continuation bytes behind %s" % (r, name))
        if s == G4 + b"\x80":
            out.add("a good 4-byte character directly followed by a continuation byte")
    # the partition's edges
    for name, item in ITEMS:
        i = text.find(item)
        while i >= 0:
            whole = not any(i < e < i + len(item) for e in start_set if i < e < i + len(item))
            if whole:
                for j in range(len(item)):
                    if (i + j) % WORKGROUP == 0 and i + j > 0:
                        out.add("%s byte %d first in a workgroup" % (name, j))
                    elif (i + j) % WAVE == 0 and i + j > 0:
                        out.add("%s byte %d first in a wave and a docmask word" % (name, j))
                for bit in (0, DOCMASK_WORD - 1):
                    if i in start_set and i % DOCMASK_WORD == bit and i > 0:
                        out.add("document start at bit %d directly before %s" % (bit, name))
                    if i + len(item) in start_set and (i + len(item)) % DOCMASK_WORD == bit and i + len(item) < n:
                        out.add("document start at bit %d directly after %s" % (bit, name))
                if i == 0:
                    out.add("%s as the first bytes of the batch" % name)
                if i + len(item) == n:
                    out.add("%s as the last bytes of the batch" % name)
            i = text.find(item, i + 1)
        for k in (1, 2, 3):
            if text.endswith(item[:k]) and n > k and text[-k - 1] < 0x80:
                out.add("%s cut after %d as the last bytes of the batch" % (name, k))
    if n == 1:
        out.add("a batch of the one byte %02X" % text[0])
    if n > 2 * WORKGROUP and n % WAVE:
        out.add("more than two workgroups and a ragged tail")
    # empty documents that share their offset with a bad byte
    run = 0
    for i, s in enumerate(docs):
        if not s:
            run += 1
            continue
        if run and (s[0] & 0xC0) == 0x80:
            out.add("%d empty documents in front of a stray continuation byte" % run)
        run = 0
    # chunk edges
    doc_off = np.array(starts + [n], dtype=np.int64)
    host = host_chunk_starts(doc_off, chunk_bytes)
    if len(host) > 1:
        if host == device_chunk_starts(doc_off, chunk_bytes):
            out.add("the host and the device chunk plan agree")
        for d in host[1:]:
            b0 = starts[d]
            out.add("a chunk start on a tile multiple (lead == 0)" if b0 % TILE == 0 else "a chunk start inside a tile (lead > 0)")
            if text[b0 - 2:b0 + 1] == b"\xe4\xb8\xad":
                out.add("E4 B8 | AD across a chunk boundary")
            if text[b0 - 4:b0] == G4:
                out.add("a good 4-byte character ends at a chunk boundary")
            if not docs[d] and docs[d + 1][:1] == b"\x80":
                out.add("a chunk's first document is empty and the next starts with 80")
    return out


ALL_EDGES = ({"every sequence of 1 to 4 class values", "a slice of the class product as a tiny job", "more than a small job",
              "C0 AF", "C1 BF", "E0 80 80", "E0 9F BF", "ED A0 80", "ED BF BF", "F0 80 80 80", "F0 8F BF BF", "F4 90 80 80",
              "a stray continuation byte at a document start", "a good 4-byte character directly followed by a continuation byte",
              "more than two workgroups and a ragged tail", "the host and the device chunk plan agree",
              "a chunk start on a tile multiple (lead == 0)", "a chunk start inside a tile (lead > 0)", "E4 B8 | AD across a chunk boundary",
              "a good 4-byte character ends at a chunk boundary", "a chunk's first document is empty and the next starts with 80"}
             | _cut_names()
             | {"%s whole" % c.hex() for c in TABLE_3_7}
             | {"%02X %s" % (x, how) for x in range(0xF5, 0x100) for how in ("alone", "and three continuation bytes")}
             | {"%d continuation bytes behind %s" % (r, name) for name, _ in RUN_HEADS for r in CONT_RUNS}
             | {"%s byte %d first in a %s" % (name, j, where) for name, item in ITEMS for j in range(len(item))
                for where in ("workgroup", "wave and a docmask word")}
             | {"document start at bit %d directly %s %s" % (bit, side, name) for name, _ in ITEMS for bit in (0, DOCMASK_WORD - 1)
                for side in ("before", "after")}
             | {"%s as the %s bytes of the batch" % (name, which) for name, _ in ITEMS for which in ("first", "last")}
             | {"%s cut after %d as the last bytes of the batch" % (name, k) for name, _ in ITEMS for k in (1, 2, 3)}
             | {"a batch of the one byte %02X" % x for x in (0x41, 0x80, 0xC3, 0xF0)}
             | {"%d empty documents in front of a stray continuation byte" % r for r in EMPTY_RUNS})


def batches():
    """Every batch of the case set, by name: what both tiers run."""
    out = [("class_product", class_product()), ("class_product_slice", class_product_slice()),
           ("edges_cuts_kinds", edge_layout() + table_cuts() + bad_kinds()), ("chunks", chunk_layout())]
    return out + [("small_%02d" % i, b) for i, b in enumerate(small_batches())]
