"""Generator of split-rule cases placed on the structural edges of the pretok_split kernel -- shared by the CPU tier
(test_split_edges_cpu.py) and the GPU tier (test_split_edges_gpu.py).  Pure Python, seeded, deterministic; reads nothing.

The kernel gives one lane a 64-byte block, one wave a span of 62 blocks (3,968 bytes) and one workgroup 8 spans (31,744
bytes); carries travel between lanes by shuffles and stop at a wave's halo lanes.  A chain is a text of segments of
exactly `stride` bytes, so that the end of segment i (the "edge", byte (i + 1) * stride) is a block edge and, for the
3,968-byte stride, a wave edge and every 8th a workgroup edge.  Segment i ends with

    [neutral ASCII filler][context: a run of r bytes][construct body, first byte at edge - k][tail, past the edge]

Every construct body of m bytes is placed at every shift k in 0..m+1 (every split over the edge, and the two positions
wholly after / wholly before it).  The run that leads into it reaches back r bytes, r in R_WAVE; the last value,
"full", starts right behind the previous segment's tail, inside the wave's first emitting block: the state that block
works out has to travel through every later lane of the wave (61 rounds of the fixed-point loop).  "beyond" runs
(beyond_chains) also cover the block before the wave, so that lane 0's unknown flags are what travels.  All text is built
from whole characters; the filler is ASCII.

Skip rule (the one place): CONTEXTS_OF maps a construct family to the context types whose run can change where that
family's pieces start or what state reaches them; the other (family, context type) combinations are not generated.
r = 0 has no context and is generated once per (construct, k).

Document modes: "a" the whole text is one document; "b" a document starts on every edge; "c-1", "c0", "c+1" a document
boundary at edge - 1, edge, edge + 1 (on chains restricted to r in {0, 64}).  A boundary that would fall inside a
character moves back to that character's first byte: documents are always whole characters.

every_codepoint_docs(): one probe document "1" + c + "2345   " + c per code point.  The digit phase shows the N class
("1c2|345" against "1|c|234|5"), the three spaces before the second c show the W class (one white-space piece against
"  | c").  L against O changes only whether c joins the piece before or after it, and where neither neighbour merges
with c's bytes in the rank table both give the same tokens: that difference is visible for part of the code points
only (test_split_edges_cpu.py prints how many), and this limit is real.
"""
import numpy as np

BLOCK = 64
WAVE = 62 * BLOCK                    # 3,968: bytes a wave emits
WORKGROUP = 8 * WAVE                 # 31,744
BLOCK_STRIDE = 3 * BLOCK             # the block-only chain: 192-byte segments
MAX_BATCH = 16 << 20                 # below the 32 MiB host chunk and the 1 GiB device chunk: byte 0 is byte 0 of the grid

FULL = "full"
R_WAVE = (0, 1, 63, 64, 65, 130, FULL)
R_BLOCK = (0, 1, 63, 64)
R_MODE_C = (0, 64)

CONTEXT_UNIT = {"digits": "7", "spaces": " ", "nl": "\n", "crlf": "\r\n", "letters": "a", "dot": "."}

# the skip rule: which runs can interact with which constructs
CONTEXTS_OF = {
    "contraction": ("letters", "dot"),                     # a word takes the contraction; a symbol run swallows the apostrophe
    "digits": ("digits", "spaces"),                        # the phase of \p{N}{1,3}; the optional space of r50k's " ?\p{N}+"
    "white": ("digits", "spaces", "nl", "crlf", "letters", "dot"),
    "linebreak": ("spaces", "nl", "crlf", "dot"),          # \s*[\r\n]+, [\r\n]* after a symbol piece
    "prefix": ("spaces", "nl", "letters", "dot"),          # what the optional first character may be taken from
    "multibyte": ("digits", "spaces", "letters", "dot"),   # a run of each class before a character of each class
    "special": (),
    "regression": (),                                      # they bring their own run
}

_FILL = "The quick brown fox, jumps over; the lazy dog. "

SPECIALS = ("<|endoftext|>", "<|fim_prefix|>", "<|endofprompt|>")


def _name(s):
    return s.encode("unicode_escape").decode("ascii")


def constructs(kind):
    """[(family, name, body, tail)] for pattern kind 1 (cl100k) or 0 (r50k).  The tail follows the body directly."""
    out = []

    def add(family, body, tail, name=None):
        out.append((family, (name or _name(body)) + "+" + _name(tail), body, tail))

    lower = ["'s", "'t", "'m", "'d", "'re", "'ve", "'ll"]
    forms = list(lower)
    if kind == 1:                                          # (?i:...) only in cl100k
        forms += [c.upper() for c in lower] + ["'Re", "'vE", "'Ll", "'\u017f", "'\u212a"]
    for c in forms:
        add("contraction", c, "x z")                       # followed by a letter
        add("contraction", c, ". z")                       # followed by a non-letter
    for c in ("'rx", "'vx", "'lx"):                        # the first letter of a contraction, the wrong second one
        add("contraction", c, " z")

    if kind == 1:                                          # \p{N}{1,3}
        for n in range(1, 8):
            add("digits", "1234567"[:n], " z")
        for run in ("5\u0663\uff15\U0001d7d8", "\U0001d7d8\uff15\u06635", "\u0663\u0663\uff15\uff15\U0001d7d8\U0001d7d85"):
            add("digits", run, " z")
        add("digits", "12345", "ab ")
        add("digits", "12345", ". z")
    else:
        add("digits", "12345", " z")
        add("digits", "5\u0663\uff15\U0001d7d8", "ab ")

    for ws in (" ", "\t", "\u00a0", "\u2003", "\u3000"):
        add("white", ws + "ab", " z")

    for body in ("\r\n", "\n\n", "\r\r\n",
                 ".\r\n\r\n", "!\n\n", "?)\r\n",           # a symbol piece takes the CR/LF chain (cl100k)
                 " \n", "  \r\n", "\t\n", "\u3000\n",       # \s*[\r\n]+
                 "\n ", "\r\n\t", "\n\u00a0", "\n\n  "):    # white space right after a CR/LF: the slow position
        add("linebreak", body, "z ")

    for body in (" word", "!word", "\tword", "\nword", "\r\nword", " !!", "  !!", " 12", ".a", "\u20aca", "\u3002\u4e2d"):
        add("prefix", body, " z")

    chars = {"L": "\u00e9\u4e2d\ud55c\U0001d49c\u0416\u65e5", "N": "\u00b2\u0663\u2167\U0001d7d8",
             "W": "\u0085\u00a0\u2028\u3000", "O": "\u20ac\u3002\U0001f355\ufe0f\u200d\u0300\u4dc0"}
    for cls, cs in chars.items():
        for c in cs:
            add("multibyte", c, c + "a ", name=cls + "-U+%04X" % ord(c))

    # Found by this sweep: a CR/LF chain that a symbol piece has taken, covers the whole block before a wave edge and ends on
    # the edge, then white space and another CR/LF.  The wave's first lanes cannot see the chain's origin, and the character
    # right after the chain was decided as if no symbol piece had taken it.  (k = 131 puts the space on the edge.)
    if kind == 1:
        add("regression", "." + "\n" * 130 + " \n", "z ", name="symbol-130lf-space-lf")
        add("regression", "." + "\r\n" * 65 + "\t\r\n", "z ", name="symbol-65crlf-tab-crlf")
    return out


def _context(unit, r):
    s = unit * (r // len(unit) + 1)
    return s[len(s) - r:]                                   # ends on a whole unit ("\r\n" chains may start with "\n")


def _filler(n):
    return (_FILL * (n // len(_FILL) + 1))[:n]


# Full-span runs: every (construct, k) gets one after every context type the skip rule allows, and one of WG_FULL's type on a
# workgroup edge.  What they cost the oracle, whose bytePairMerge restates the reference's quadratic one, was measured per
# 3,968-byte run: cl100k digits 0.24 ms (pieces of three); r50k spaces and "\r\n" 0.48 ms; every other run is one piece of
# 13-17 ms (cl100k spaces 14.0, "\n" 16.5, "\r\n" 13.5, letters 15.1, "." 13.8; r50k digits 9.9, "\n" 10.7, letters 12.3,
# "." 13.2).  The cheap ones, and per construct one costly one at its middle split (COSTLY_FULL_OF), are part of the main
# chains, which also run as ONE document (the oracle is then single-threaded).  The other costly ones -- about 1,400 under
# cl100k, 20 s of oracle time as one document -- are chains of their own (full_span_chains) that the GPU tier runs with a
# document per segment only (8 oracle threads); the CPU tier, which only splits, runs them in every mode.
WG_FULL = {1: "digits", 0: "spaces"}
CHEAP_FULL = {1: ("digits",), 0: ("spaces", "crlf")}
COSTLY_FULL_OF = {"contraction": "letters", "digits": "spaces", "white": "nl", "linebreak": "crlf", "prefix": "nl",
                  "multibyte": "dot", "regression": "nl", "special": "dot"}
# A run that also covers the block before the wave's first block and the whole wave: 3,968 + 130 bytes.  Lane 0 of that wave
# starts with its "unknown" flags and no lane of the wave can clear them (beyond_chains; the segment before is filler and run).
BEYOND = "beyond"
BEYOND_OF = {"white": ("crlf", "nl"), "linebreak": ("crlf", "nl"), "regression": ("crlf",), "digits": ("digits",)}


def _specs(kind, rs):
    """(wg, rest, costly): specs (family, name, body, tail, k, ctx, r); wg are the ones that must meet a workgroup edge,
    costly the full-span runs kept out of the main chains."""
    wg, rest, costly = [], [], []
    for family, name, body, tail in constructs(kind):
        m = len(body.encode("utf-8"))
        for k in range(m + 2):
            for r in rs:
                if r == 0:
                    wg.append((family, name, body, tail, k, "none", 0))
                elif r == FULL:
                    wg.append((family, name, body, tail, k, WG_FULL[kind], r))
                    for ctx in CONTEXTS_OF[family]:
                        spec = (family, name, body, tail, k, ctx, r)
                        if ctx == WG_FULL[kind]:
                            continue
                        if ctx in CHEAP_FULL[kind] or (k == (m + 1) // 2 and ctx == COSTLY_FULL_OF[family]):
                            rest.append(spec)
                        else:
                            costly.append(spec)
                else:
                    rest += [(family, name, body, tail, k, ctx, r) for ctx in CONTEXTS_OF[family]]
    return wg, rest, costly


def _beyond_specs(kind):
    out = []
    for family, name, body, tail in constructs(kind):
        k = (len(body.encode("utf-8")) + 1) // 2
        for ctx in dict.fromkeys((WG_FULL[kind],) + BEYOND_OF.get(family, ())):
            out.append((family, name, body, tail, k, ctx, BEYOND))
    return out


def _order(wg, rest, every, phase, reserved=False):
    """Slots i with i % every == phase take the `wg` specs first (only those if `reserved`); None is a segment of filler only."""
    slots = []
    wg, rest = list(wg), list(rest)
    wi = ri = 0
    while wi < len(wg) or ri < len(rest):
        i = len(slots)
        if i % every == phase:
            if wi < len(wg):
                slots.append(wg[wi]); wi += 1
            elif ri < len(rest) and not reserved:
                slots.append(rest[ri]); ri += 1
            else:
                slots.append(None)
        elif ri < len(rest):
            slots.append(rest[ri]); ri += 1
        else:
            slots.append(None)
    return slots


class Chain:
    """text (np.uint8), stride, labels (one per segment), char_start (bool per byte: a character starts here)."""

    def __init__(self, slots, stride, forbid=None):
        parts, labels = [], []
        pos = 0
        for i, spec in enumerate(slots):
            edge = (i + 1) * stride
            if spec is None or (forbid and forbid(edge)):
                assert spec is None
                labels.append("pad#%d" % i)
                continue
            family, name, body, tail, k, ctx, r = spec
            bb, tb = body.encode("utf-8"), tail.encode("utf-8")
            start = edge - k
            want = start - ((stride - len(bb)) if r == FULL else (stride + 130) if r == BEYOND else r)
            c0 = max(pos, want)
            assert pos <= c0 <= start and (r == FULL or c0 == want), (spec, pos, want)
            parts.append(_filler(c0 - pos).encode())
            if start > c0:
                parts.append(_context(CONTEXT_UNIT[ctx], start - c0).encode())
            parts.append(bb); parts.append(tb)
            pos = start + len(bb) + len(tb)
            labels.append("%s:%s|k=%d|ctx=%s|r=%s" % (family, name, k, ctx, r))
        n_seg = len(slots) + 1                                # a closing segment holds the last tail
        assert pos <= n_seg * stride
        parts.append(_filler(n_seg * stride - pos).encode())
        labels.append("end")
        data = b"".join(parts)
        assert len(data) == n_seg * stride and len(data) < MAX_BATCH
        self.text = np.frombuffer(data, dtype=np.uint8)
        self.stride = stride
        self.labels = labels
        self.char_start = (self.text & 0xC0) != 0x80

    def n_segments(self):
        return len(self.labels)

    def _snap(self, p):
        while not self.char_start[p]:
            p -= 1
        return p

    def doc_off(self, mode):
        n = len(self.text)
        if mode == "a":
            return np.array([0, n], dtype=np.int64)
        delta = {"b": 0, "c-1": -1, "c0": 0, "c+1": 1}[mode]
        cuts = sorted({self._snap(e + delta) for e in range(self.stride, n, self.stride)})
        return np.array([0] + cuts + [n], dtype=np.int64)

    def batch(self, mode):
        return self.text, self.doc_off(mode), self.labels

    def label_at(self, byte_pos):
        """The label of the construct nearest to a byte: the one on the closer edge."""
        i = max(0, min(len(self.labels) - 1, (int(byte_pos) + self.stride // 2) // self.stride - 1))
        return self.labels[i]


_cache = {}


def _chunks(slots, stride):
    per = ((MAX_BATCH // stride) - 2) // 8 * 8                # segments per chain: a multiple of 8 keeps the slots' phase
    return [Chain(slots[i:i + per], stride) for i in range(0, len(slots), per)]


def wave_chains(kind, rs=R_WAVE):
    """The main sweep: chains of 3,968-byte segments, each under 16 MiB; (construct, k) meets a workgroup edge at r = 0
    and with a full-span context."""
    key = ("wave", kind, rs)
    if key not in _cache:
        wg, rest, _ = _specs(kind, rs)
        _cache[key] = _chunks(_order(wg, rest, 8, 7), WAVE)
    return _cache[key]


def full_span_chains(kind):
    """The full-span runs that are one costly piece each (see CHEAP_FULL)."""
    key = ("costly", kind)
    if key not in _cache:
        _cache[key] = _chunks(_specs(kind, R_WAVE)[2], WAVE)
    return _cache[key]


def beyond_chains(kind):
    """Runs that cover a whole wave and the block before it: every other segment, the one before being filler and run."""
    key = ("beyond", kind)
    if key not in _cache:
        slots = []
        for spec in _beyond_specs(kind):
            slots += [None, spec]
        _cache[key] = _chunks(slots, WAVE)
    return _cache[key]


def mode_c_chains(kind):
    return wave_chains(kind, R_MODE_C)


def block_chain(kind):
    """192-byte segments: the same constructs and shifts on block edges inside a wave (no edge is a multiple of 3,968)."""
    key = ("block", kind)
    if key not in _cache:
        wg, rest, _ = _specs(kind, R_BLOCK)
        every = WAVE // BLOCK                                  # lcm(192, 3968) = 62 segments: those slots stay filler
        slots = _order([], wg + rest, every, every - 1, reserved=True)
        _cache[key] = Chain(slots, BLOCK_STRIDE, forbid=lambda e: e % WAVE == 0)
    return _cache[key]


def special_chain():
    """encode() path, cl100k: each literal at every shift over a wave edge, a document per segment; '<' and cut literals
    beside them (text_tails() has the literals, whole and cut, that end exactly with the text)."""
    if "special" not in _cache:
        slots = []
        for lit in SPECIALS + ("<|endofx", "<", "<|"):
            m = len(lit)
            for k in range(m + 2):
                slots.append(("special", _name(lit), lit, " z", k, "none", 0))
        _cache["special"] = Chain(slots, WAVE)
    return _cache["special"]


TAIL_SIZES = (63, 64, 65, 3967, 3968, 3969, 31743, 31744, 31745, 63487, 63488, 63489)
TAIL_ENDINGS = (("char4", "\U0001f355"), ("half-contraction", "'l"), ("digits200", "7" * 200), ("dot-sp-crlf", ". \r\n"),
                ("cut-literal", "<|endof"), ("whole-literal", "<|endoftext|>"))


def text_tails():
    """[(label, text, doc_off)]: single documents of n bytes whose last bytes are each of TAIL_ENDINGS, longest first."""
    out = []
    for n in sorted(TAIL_SIZES, reverse=True):
        for name, end in TAIL_ENDINGS:
            eb = end.encode("utf-8")[-n:]
            data = _filler(n - len(eb)).encode() + eb
            assert len(data) == n
            out.append(("tail:%s|n=%d" % (name, n), np.frombuffer(data, dtype=np.uint8), np.array([0, n], dtype=np.int64)))
    return out


def _utf8_matrix(cps):
    """UTF-8 of code points that all have the same encoded length: uint8 [n, len]."""
    cps = np.asarray(cps, dtype=np.uint32)
    hi = int(cps.max())
    if hi < 0x80:
        return cps.astype(np.uint8)[:, None]
    if hi < 0x800:
        return np.stack([0xC0 | (cps >> 6), 0x80 | (cps & 63)], axis=1).astype(np.uint8)
    if hi < 0x10000:
        return np.stack([0xE0 | (cps >> 12), 0x80 | ((cps >> 6) & 63), 0x80 | (cps & 63)], axis=1).astype(np.uint8)
    return np.stack([0xF0 | (cps >> 18), 0x80 | ((cps >> 12) & 63), 0x80 | ((cps >> 6) & 63), 0x80 | (cps & 63)], axis=1).astype(np.uint8)


def probe_codepoints():
    cps = np.arange(1, 0x110000, dtype=np.uint32)
    return cps[(cps < 0xD800) | (cps > 0xDFFF)]


def probe(c):
    return "1" + c + "2345   " + c


def every_codepoint_docs():
    """(text, doc_off, cps): document d is probe(chr(cps[d])) for every code point 1..0x10FFFF but the surrogates:
    1,112,063 documents (the noncharacters are valid UTF-8 and are included)."""
    if "probes" not in _cache:
        cps = probe_codepoints()
        assert len(cps) == 0x10FFFF - 0x800
        blocks = []
        for lo, hi in ((1, 0x80), (0x80, 0x800), (0x800, 0x10000), (0x10000, 0x110000)):
            sel = cps[(cps >= lo) & (cps < hi)]
            u = _utf8_matrix(sel)
            n_u = u.shape[1]
            rows = np.empty((len(sel), 8 + 2 * n_u), dtype=np.uint8)
            rows[:, 0] = ord("1")
            rows[:, 1:1 + n_u] = u
            rows[:, 1 + n_u:8 + n_u] = np.frombuffer(b"2345   ", dtype=np.uint8)[None, :]
            rows[:, 8 + n_u:] = u
            blocks.append(rows)
        lens = np.concatenate([np.full(len(b), b.shape[1], dtype=np.int64) for b in blocks])
        doc_off = np.zeros(len(cps) + 1, dtype=np.int64)
        np.cumsum(lens, out=doc_off[1:])
        text = np.concatenate([b.reshape(-1) for b in blocks])
        _cache["probes"] = (text, doc_off, cps)
    return _cache["probes"]
