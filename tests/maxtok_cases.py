"""The case set of the device maxTokens tests (CPU and GPU tier): batches for jtk_batch_encode_device_max_tokens built on the
partition of its kernels (jtokkit_amd/csrc/jtk_maxtok.hip) -- k_mt_gather's alignment product, k_mt_decide's backward scan over
the piece mask (word, step and lane edges; base and top at the ends of a mask word; single-chunk jobs and the second chunk of a
chunked one), its wave sums at 63..129 tokens, the plan's 1024-item blocks in rounds 2 and 3, and k_mt_special's 16-byte blocks
and 4096-byte workgroups.  The model tests/maxtok_ref.py says where every document lands; edges_reached() names what a batch
reaches from the model's answer, and the tests assert on it.  Built on the CPU, seeded.

Traps are texts on which a scan that is too eager returns wrong tokens:
  margin trap      `... they'l|l`: the prefix ends inside a contraction.  cl100k matches `'l` as one piece where the whole text
                   has `'ll`; r50k matches `'` and `l`, a piece start the whole text does not have.  A scan that accepts starts
                   up to p sees the start at p (cl100k: the neighbour's first byte) or at p - 1 (r50k) and keeps max_tokens
                   tokens that end there: the last of them is not the whole text's.
  safe-start trap  `\\n` + 16 or 24 spaces | `\\n`: the prefix splits `\\n` from the spaces, the whole text (cl100k: `\\s*[\\r\\n]`) takes
                   both and the second `\\n` as one piece.  The start at the first space is at or below top but not safe; a scan
                   that ignores jtk_maxtok_safe_start keeps `\\n` as its last token.
Outcome of the searches (search_safe_start_trap below, 30,000 samples per pattern, seed 0): cl100k_base gives 8 traps, all of
the form above (`\\n` or `\\r\\n`, 16 or 24 spaces, the cut, a line break: the whole run is one token of the rank table); r50k_base
gives none -- under `\\s+(?!\\S)|\\s+` a white-space run is one piece up to its last character, so a piece start inside it is
always a boundary of the whole text too, so M_unsafe cannot be told from the rule by its tokens under that pattern.  Likewise
no text tells M_top1 from the rule by its tokens: the longest look-ahead of either pattern past a start that passes
jtk_maxtok_safe_start is a contraction's 3 bytes (4 for a cut character), so a start 15 bytes before the cut is always the whole
text's too -- the margin of 16 has slack.  M_top1 is told by q itself: the model's q differs from the rule header's on the
documents with a safe start at top + 1."""
import collections
import functools
import random

import maxtok_ref as ref
import oracle_lib

# ---- the partition of the kernels
BLOCK = 16                    # bytes per k_mt_special lane and per gather word
MASK_WORD = 64                # piece-mask bits per word
STEP_WORDS = 64               # mask words per scan step of k_mt_decide (one per lane)
MARGIN = 16                   # JTK_MAXTOK_MARGIN
PLAN_BLOCK = 1024             # plan items per workgroup (k_mt_count / k_mt_place)
PLAN_ITEMS = 4                # plan items per thread
SPECIAL_WG = 256 * BLOCK      # bytes per k_mt_special workgroup
MIN_CHUNK = 65536             # the smallest JTK_OPT_CHUNK_BYTES
TILE = ref.TILE

GATHER_LENGTHS = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 18, 31, 32, 33, 47, 48, 49)
GATHER_MAX_TOKENS = 64        # P = 576, a multiple of 16: a filler moves the source against the destination by its length
GATHER_OFFSETS = (0, 1, 7, 15)
SPECIAL_OFFSETS = (0, 3, 15)
EDGE_BITS = (0, 1, 62, 63)
SUM_LIMITS = (63, 64, 65, 127, 128, 129)
EMPTY_RUNS = (0, 1, 2, 65)
EOT = b"<|endoftext|>"

CUSTOM = dict(name="maxtok_custom", kind=1, file="r50k_base.tiktoken",
              specials={"^": 60001, "<<" + "=" * 36 + ">>": 60002, "[SEP]": 60003, "[SEP]+": 60004})

Case = collections.namedtuple("Case", "name kind enc docs max_tokens modes chunk_bytes offsets")
#   modes: the values of `ordinary` the batch runs under; chunk_bytes: None or JTK_OPT_CHUNK_BYTES; offsets: tensor offsets


def literals(enc):
    sp = CUSTOM["specials"] if enc == CUSTOM["name"] else oracle_lib.ENCODINGS[enc]["specials"]
    return [k.encode() for k in sp]


@functools.lru_cache(maxsize=None)
def oracle(enc):
    if enc == CUSTOM["name"]:
        import os
        with open(os.path.join(oracle_lib.DATA_DIR, CUSTOM["file"]), "rb") as f:
            return ref.Oracle(oracle_lib.OracleEncoding(enc, CUSTOM["kind"], f.read(), CUSTOM["specials"]))
    return ref.Oracle(oracle_lib.get(enc))


def prefixes(mx, n=6):
    out = [ref.first_prefix(mx)]
    while len(out) < n:
        out.append(ref.next_prefix(out[-1]))
    return out


# ---- text without safe piece starts
KANA, COMMA = "あ".encode(), "、".encode()


def unsafe_run(pos, end, cuts):
    """end - pos bytes for text positions [pos, end), behind a letter: units of `、あ` -- every piece start is the E3 of the
    comma, which jtk_maxtok_safe_start rejects -- and letters where a unit would lie across one of `cuts` (the prefix ends of the
    rounds: a prefix must not end inside a character) or past `end`.  Ends in a letter."""
    out = []
    while pos < end:
        nxt = min([c for c in cuts if pos < c < pos + 6] + [end])
        if nxt >= pos + 6:
            out.append(COMMA + KANA)
            pos += 6
        else:
            out.append(b"x" * (nxt - pos))
            pos = nxt
    return b"".join(out)


def stubborn(length, cuts):
    """A document of `length` bytes without a safe start: undecided until a round takes it whole."""
    return b"x" + unsafe_run(1, length, cuts)


def scan_doc(head, s, tail, length, cuts):
    """One safe start (` b`) at byte s behind a head without one -- head "a": one giant piece (empty mask words), "b": rejected
    starts (full words) -- and a tail of the same two kinds.  s None: no safe start at all."""
    if s is None:
        return b"a" * length if head == "a" else stubborn(length, cuts)
    h = b"a" * s if head == "a" else stubborn(s, cuts)
    t = b"b" * (length - s - 2) if tail == "a" else unsafe_run(s + 2, length, cuts)
    return h + b" b" + t


# ---- scan batches
ScanSpec = collections.namedtuple("ScanSpec", "base63 head s tail")           # s: int, None, or ("top", delta): P - 16 + delta


def scan_batch(mx, rnd, specs, chunked):
    """The documents of `specs`, all open until round `rnd`, each behind a padding document that sets base & 63 in that round's
    gather buffer.  A padding document is stubborn and of a length in (P of the round before, P]: the round takes it whole.
    chunked: fillers in front put the first of them at the start of the second 65536-byte chunk, fillers behind make the job
    longer than one and a quarter chunks."""
    ps = prefixes(mx)
    P, prev = ps[rnd - 1], ps[rnd - 2] if rnd > 1 else 0
    cuts = ps
    docs, cur = [], 0
    filler = stubborn(P, cuts)
    if chunked:
        n_front = -(-MIN_CHUNK // P)
        docs += [filler] * n_front
        cur = n_front * P
    for sp in specs:
        L = prev + 1
        while (cur + L) & 63 != sp.base63:
            L += 1
        assert prev < L <= P
        docs.append(stubborn(L, cuts))
        cur += L
        s = sp.s if not isinstance(sp.s, tuple) else P - MARGIN + sp.s[1]
        assert s is None or s > max(prev - MARGIN, 0) or rnd == 1
        docs.append(scan_doc(sp.head, s, sp.tail, P + 40, cuts))
        cur += P
    if chunked:
        while cur <= MIN_CHUNK + MIN_CHUNK // 4 + P:
            docs.append(filler)
            cur += P
    return docs


def _top_bases(P):
    """base & 63 for which top & 63 is an edge bit."""
    return [(t - (P - MARGIN)) & 63 for t in EDGE_BITS]


def scan_specs():
    """(name, max_tokens, round, specs).  Rounds of 72 and 512 bytes carry the product of the base and top bits with the places of
    the safe start; the long rounds carry what only a long prefix reaches."""
    out = []
    s1 = []
    for b in list(EDGE_BITS) + _top_bases(72):
        s1 += [ScanSpec(b, "a", ("top", 0), "a"), ScanSpec(b, "b", ("top", 0), "b"), ScanSpec(b, "b", ("top", 1), "a"),
               ScanSpec(b, "a", 1, "a"), ScanSpec(b, "b", 1, "b"), ScanSpec(b, "a", None, "a"), ScanSpec(b, "b", None, "b")]
    s1 += [ScanSpec(4, "a", 30, "b"), ScanSpec(60, "a", 2, "b"), ScanSpec(63, "b", 20, "b")]
    out.append(("scan_72", 1, 1, s1))
    s2 = []
    for b in list(EDGE_BITS) + _top_bases(512):
        s2 += [ScanSpec(b, "a", ("top", 0), "a"), ScanSpec(b, "b", ("top", 0), "b"), ScanSpec(b, "a", ("top", 1), "b"),
               ScanSpec(b, "b", None, "b")]
    s2 += [ScanSpec((8 - 300) & 63, "b", 300, "b"), ScanSpec((8 - 200) & 63, "a", 200, "b")]   # rejected bits above q in its word
    out.append(("scan_512", 8, 2, s2))
    # P = 8192, top - base = 8176 bits: two steps.  Lane 63 of the first step, lane 0 of the second, a start deep in the second
    top = 8192 - MARGIN
    out.append(("scan_8192", 8, 4, [ScanSpec(0, "a", top - 63 * 64, "a"), ScanSpec(63, "b", top - 64 * 64, "b"),
                                    ScanSpec(1, "b", top - 63 * 64 - 5, "a"), ScanSpec(62, "a", 2100, "a")]))
    # P = 4096 at max_tokens 24 (256, 1024, 4096): top - base = 4080 bits, exactly 64 words apart when base & 63 >= 16
    out.append(("scan_4096", 24, 3, [ScanSpec(62, "a", ("top", 0), "a"), ScanSpec(16, "b", 1100, "b"), ScanSpec(63, "b", None, "b")]))
    # P = 18432: 288 words, five steps when nothing is found
    out.append(("scan_18432", 1, 5, [ScanSpec(0, "a", None, "a"), ScanSpec(63, "b", None, "b"), ScanSpec(1, "a", 4700, "b")]))
    return out


# ---- traps
_WORDS = ("international understanding responsibility government development information university different important "
          "community president education experience technology environment performance organization relationship particularly "
          "significant opportunities characteristics administration representative recommendations responsibilities").split()


def _words_of(o, n_tokens, n_bytes, rng):
    """n_tokens words, each ` word` one token, n_bytes bytes together."""
    pool = [w for w in _WORDS if len(o.tokens((" " + w).encode())) == 1]
    lens = sorted({len(w) + 1 for w in pool})
    reach = [{0: None}]                                                      # reach[c][bytes] = length of the last word
    for c in range(n_tokens):
        reach.append({b + L: L for b in reach[c] for L in lens if b + L <= n_bytes})
    assert n_bytes in reach[n_tokens], (n_tokens, n_bytes)
    out, b = [], n_bytes
    for c in range(n_tokens, 0, -1):
        L = reach[c][b]
        out.append(" " + rng.choice([w for w in pool if len(w) + 1 == L]))
        b -= L
    text = "".join(out).encode()
    assert len(o.tokens(text)) == n_tokens and len(text) == n_bytes
    return text


def _tail(rng, n):
    return "".join(" " + rng.choice(_WORDS) for _ in range(n)).encode()


def margin_trap(o, mx, rng):
    """The prefix (8 mx + 64 bytes) holds exactly mx tokens and ends in ` they'l`."""
    p = ref.first_prefix(mx)
    cut = b" they'l"
    head = _words_of(o, mx - len(o.tokens(cut)), p - len(cut), rng)
    doc = head + cut + b"l go" + _tail(rng, 70)
    assert len(o.tokens(doc[:p])) == mx and o.tokens(doc[:p]) != o.whole(doc, mx)[0]
    return doc


def safe_start_trap(o, mx, spaces, rng):
    """mx - 1 words, `\\n`, the spaces, the cut, `\\n` U+3000 and a tail: token mx of the prefix is `\\n`."""
    p = ref.first_prefix(mx)
    head = _words_of(o, mx - 1, p - spaces - 1, rng)
    doc = head + b"\n" + b" " * spaces + b"\n\xe3\x80\x801 tail" + _tail(rng, 70)
    assert len(doc[:p]) == p and doc[p - 1:p + 1] == b" \n"
    return doc


TRAP_MAX_TOKENS = 16


def trap_batch(enc):
    """Every trap at each of the four top & 63 edge bits (padding documents of up to one prefix set base)."""
    o, rng, mx = oracle(enc), random.Random(41), TRAP_MAX_TOKENS
    P = ref.first_prefix(mx)
    docs, cur = [], 0
    for kind in ("margin", "safe16", "safe24"):
        for b in _top_bases(P):
            L = 1
            while (cur + L) & 63 != b:
                L += 1
            docs.append(stubborn(L, [P]))
            doc = margin_trap(o, mx, rng) if kind == "margin" else safe_start_trap(o, mx, 16 if kind == "safe16" else 24, rng)
            docs.append(doc)
            cur += L + P
    docs.append(b"the neighbour behind the last trap")
    return docs


def search_safe_start_trap(enc, n, seed=0):
    """The family `words ws-run | ws-run tail`: max_tokens - 1 one-token words, a white-space run of a few random characters and up
    to 40 spaces, the cut of round 1 inside or right behind the spaces, more white space and a tail.  Returns the samples on which
    a scan that ignores jtk_maxtok_safe_start (the model's M_unsafe) returns tokens that are not the whole text's."""
    o, rng, found = oracle(enc), random.Random(seed), []
    ws = [" ", " ", "\n", "\n", "\t", "\r\n", "\u00a0", "\u3000", "\u2003"]
    for _ in range(n):
        mx = rng.choice((8, 12, 16, 20))
        p = ref.first_prefix(mx)
        run1 = "".join(rng.choice(ws) for _ in range(rng.randint(1, 3))).encode()
        spaces = rng.randint(0, 40)
        before = rng.randint(0, spaces)                                      # the spaces in front of the cut
        run2 = "".join(rng.choice(ws) for _ in range(rng.randint(0, 3))).encode()
        try:
            head = _words_of(o, mx - 1, p - len(run1) - before, rng)
        except AssertionError:
            continue                                                         # (no such words)
        doc = head + run1 + b" " * spaces + run2 + rng.choice(("tail", "1", "\u3000x", ".", "'ll")).encode() + b" and more text"
        got = ref.run(o, [doc], mx, mutant="M_unsafe")[0][0]
        if (got.ids, got.truncated) != o.whole(doc, mx):
            found.append((doc, mx))
    return found


# ---- the gather batch
_POOLS = {1: "abcdefghijklmnopqrstuvwxyz ,.ETAOIN0123456789", 2: "éñöüßжиΩλ", 3: "日本語のテキスト書€", 4: "\U0001F600\U0001F355\U0001D11E\U00020000"}


def _text_of(rng, n):
    """n bytes of characters of 1 to 4 bytes."""
    out = b""
    while len(out) < n:
        w = rng.choice([x for x in (1, 1, 1, 2, 3, 4) if x <= n - len(out)])
        out += rng.choice(_POOLS[w]).encode()
    return out


def gather_batch():
    """Short documents (the row is the whole document's tokens: a misplaced byte changes it) at every source alignment, destination
    alignment and length of GATHER_LENGTHS.  Sixteen groups, one per difference of the two alignments, each opened by a filler
    longer than the prefix (the source moves by its length, the destination by P, a multiple of 16) and by a document with a
    literal (24 bytes: under encode() it is refused and moves the source alone, which permutes the differences).  Within a group
    one-to-15-byte shims step the destination through all sixteen residues for every length."""
    rng = random.Random(23)
    P = ref.first_prefix(GATHER_MAX_TOKENS)
    assert P % 16 == 0 and max(GATHER_LENGTHS) < P
    docs, src, dst = [], 0, 0
    for delta in range(16):
        F = P + 1
        while (src + F - (dst + P)) % 16 != delta:
            F += 1
        docs.append(_tail(rng, 80)[:F])
        assert len(docs[-1]) == F
        src, dst = src + F, dst + P
        lit = b"say " + EOT + b" again."
        assert len(lit) == 24
        docs.append(lit)
        src, dst = src + 24, dst + 24
        for L in GATHER_LENGTHS:
            for want in range(16):
                shim = (want - dst) % 16
                if shim:
                    docs.append(_text_of(rng, shim))
                    src, dst = src + shim, dst + shim
                docs.append(_text_of(rng, L))
                src, dst = src + L, dst + L
    return docs


# ---- token-sum batches
def _word_tokens(o, rng, n):
    """ASCII words of exactly n tokens (no leading space)."""
    if n <= 0:
        return b""
    short = ["the", "of", "and", "to", "in", "is", "that", "for", "it", "with", "as", "was", "on", "be", "at", "by", "this", "have", "from"]
    ws = [rng.choice(short) for _ in range(n)]
    text = " ".join(ws).encode()
    assert len(o.tokens(text)) == n
    return text


RARE4, RARE3 = "\U0002A6D6".encode(), "䶮".encode()                         # cl100k: one token per byte


def sum_batch(enc, mx):
    """Documents around the wave sums of k_mt_decide at max_tokens = mx."""
    o, rng = oracle(enc), random.Random(100 + mx)
    P = ref.first_prefix(mx)
    docs = []
    for n in (mx - 1, mx, mx + 1):
        docs.append(_word_tokens(o, rng, n))                                 # short: p == len
        assert len(docs[-1]) < P
        docs.append(_words_of(o, n, 14 * n, rng))                            # long and few tokens: the prefix holds fewer than mx
        assert len(docs[-1]) > P
        docs.append(_word_tokens(o, rng, n) + _tail(rng, mx))                # long: decided from the prefix
        assert len(docs[-1]) > P
    # tokens 65 and later run past q: 64 word tokens, then one giant piece to the end of the prefix and beyond
    docs.append(_word_tokens(o, rng, 64) + b" " + b"q" * (P + 100))
    docs.append(_word_tokens(o, rng, 60) + b" " + b"q" * (P + 100))
    # a character cut by the limit in every byte phase, short and long; the back-off drops up to three tokens
    for rare in (RARE4, RARE3):
        run = rare * 3
        for t in range(0, len(run) + 2):
            head = _word_tokens(o, rng, mx - t - 1) + b" " if mx - t - 1 > 0 else b""
            docs.append(head + run + b" z")
            docs.append(head + run + _tail(rng, mx))
    # token 64 ends inside a character (a wave sum that stops at 64 tokens backs off from there)
    for t in (1, 2, 3):
        docs.append(_word_tokens(o, rng, 64 - t - 1) + b" " + RARE4 * 2 + b" " + _word_tokens(o, rng, mx - 64))
    # U+FFFD in the text at the limit
    docs.append(_word_tokens(o, rng, mx - 1) + b" \xef\xbf\xbd\xef\xbf\xbd and more")
    docs.append(_word_tokens(o, rng, mx - 2) + b" \xef\xbf\xbd" + RARE4 + b"\xef\xbf\xbd end")
    return docs


def small_limit_batch():
    """max_tokens 2: the back-off down to keep == 0."""
    return [RARE4 + b" tail", RARE4 * 2, RARE3 + b"x", b"a" + RARE4, RARE4 + _tail(random.Random(3), 30), b"ab", b"",
            b"\xef\xbf\xbd" + RARE4]


# ---- round batches
def round_batch(variant):
    """2100 documents at max_tokens 1 (prefixes 72, 288, 1152), 1100 of them stubborn for two rounds (and every eleventh of those
    for three).  "empty_block": 1030 leading documents decided in round 1, so the first plan block of round 2 is empty, and the
    survivors lie across the block edge at item 2048; "edge": survivors at items 1023 and 1024 of round 2.  Round 3 has 1100
    items in two blocks, all open."""
    rng = random.Random(7 if variant == "empty_block" else 8)
    cuts = prefixes(1)
    n, n_st = 2100, 1100
    lead = 1030 if variant == "empty_block" else 0
    is_st = [False] * n
    free = list(range(lead, n))
    forced = [2047, 2048] if variant == "empty_block" else [1023, 1024]
    for i in forced:
        is_st[i] = True
    rest = [i for i in free if not is_st[i]]
    rng.shuffle(rest)
    for i in rest[:n_st - len(forced)]:
        is_st[i] = True
    docs, k = [], 0
    for i in range(n):
        if is_st[i]:
            k += 1
            docs.append(stubborn(1200 + k % 9 if k % 11 == 0 else 289 + k % 40, cuts))
        else:
            docs.append(_tail(rng, rng.randint(1, 6)))
    return docs


# ---- special batches
_CLEAN = "abcdefghijklmnopqrstuvwxyz   "


def _clean(rng, n):
    return "".join(rng.choice(_CLEAN) for _ in range(n)).encode()


def special_batch(enc):
    """Literals of `enc` on the edges of k_mt_special's partition; every other byte is a lower-case letter or a space."""
    lits = literals(enc)
    rng = random.Random(len(lits))
    docs, pos = [], [0]

    def add(d):
        docs.append(d)
        pos[0] += len(d)

    def nxt(i):
        return lits[i % len(lits)]
    add(nxt(0) + _clean(rng, 20))                                            # a literal at text byte 0
    add(_clean(rng, 11))
    for r in range(16):                                                      # a literal at every offset of a block
        lit = nxt(r)
        pad = (r - pos[0]) % 16
        add(_clean(rng, pad) + lit + _clean(rng, 3))
        add(_clean(rng, rng.randint(1, 30)))
    for i, lit in enumerate(lits):                                           # near misses: nothing is flagged
        if len(lit) > 1:
            add(_clean(rng, 4) + lit[:-1] + b"x")
            add(lit[1:] + _clean(rng, 2))
    for i, run in enumerate(EMPTY_RUNS):                                     # a literal split across two documents
        lit = max(lits, key=len) if i % 2 else nxt(i)
        if len(lit) < 2:
            lit = max(lits, key=len)
        k = len(lit) // 2
        add(_clean(rng, 5) + lit[:k])
        for _ in range(run):
            add(b"")
        add(lit[k:] + _clean(rng, 5))
    add(_clean(rng, 9) + nxt(1))                                             # ends at its document's end
    add(nxt(2) + _clean(rng, 9))                                             # starts at its document's start
    add(b"")
    add(_clean(rng, 3) + nxt(0) + nxt(1) + _clean(rng, 3))                   # two adjacent literals
    long_lit = max(lits, key=len)
    add(_clean(rng, 2) + long_lit[:2] + long_lit + _clean(rng, 2))           # `<|<|endoftext|>`
    for lit in lits:                                                         # each literal alone
        add(lit)
    # a literal across a 4096-byte workgroup edge for every tensor offset: memory k * 4096 = text k * 4096 - offset
    assert pos[0] < SPECIAL_WG - 200
    for k, off in enumerate(SPECIAL_OFFSETS, 1):
        start = k * SPECIAL_WG - off - len(long_lit) // 2
        while start - pos[0] > 100:
            add(_clean(rng, rng.randint(20, 90)))
        add(_clean(rng, start - pos[0]) + long_lit + _clean(rng, 1))
    add(_clean(rng, 40))
    add(_clean(rng, 7) + nxt(3))                                             # the last bytes of the text
    return docs


# ---- the cases
@functools.lru_cache(maxsize=None)
def cases():
    out = [Case("gather", "gather", "cl100k_base", gather_batch(), GATHER_MAX_TOKENS, (True, False), None, GATHER_OFFSETS)]
    for name, mx, rnd, specs in scan_specs():
        out.append(Case(name, "scan", "cl100k_base", scan_batch(mx, rnd, specs, False), mx, (True,), None, (0,)))
        out.append(Case(name + "_chunked", "scan", "cl100k_base", scan_batch(mx, rnd, specs, True), mx, (True,), MIN_CHUNK, (0,)))
    for enc in ("cl100k_base", "r50k_base"):
        out.append(Case("traps_" + enc, "trap", enc, trap_batch(enc), TRAP_MAX_TOKENS, (True,), None, (0,)))
    for mx in SUM_LIMITS:
        out.append(Case("sum_%d" % mx, "sum", "cl100k_base", sum_batch("cl100k_base", mx), mx, (True,), None, (0,)))
    out.append(Case("sum_small", "sum", "cl100k_base", small_limit_batch(), 2, (True,), None, (0,)))
    for v in ("empty_block", "edge"):
        out.append(Case("round_" + v, "round", "cl100k_base", round_batch(v), 1, (True,), None, (0,)))
    for enc in ("p50k_edit", "cl100k_base", CUSTOM["name"]):
        out.append(Case("special_" + enc, "special", enc, special_batch(enc), 3, (False, True), None, SPECIAL_OFFSETS))
    return out


@functools.lru_cache(maxsize=None)
def model(name, ordinary=True, offset=0, mutant=None):
    c = {c.name: c for c in cases()}[name]
    return ref.run(oracle(c.enc), c.docs, c.max_tokens, ordinary, c.chunk_bytes, offset, literals(c.enc), mutant)


# ---- what a batch reaches
def edges_reached(c, ordinary=True, offset=0):
    """The edges a case reaches under one call and tensor offset, by name (gather: triples); the required sets are SCAN_EDGES (scan
    batches and traps together), GATHER_EDGES (for every offset and call), SUM_EDGES, ROUND_EDGES and special_edges_required()."""
    res, rounds = model(c.name, ordinary, offset)
    if c.kind in ("scan", "trap"):
        return scan_edges(oracle(c.enc), c.docs, res)
    if c.kind == "sum":
        return sum_edges(oracle(c.enc), c.docs, res, c.max_tokens)
    if c.kind == "round":
        return round_edges(res, rounds)
    if c.kind == "gather":
        return gather_edges(c.docs, res, c.max_tokens)
    assert c.kind == "special"
    return special_edges(c.enc, c.docs, offset)


def _job(sc):
    return "a single-chunk job" if sc.n_chunks == 1 else "the second chunk" if sc.chunk == 1 else None


def scan_edges(o, docs, results):
    out = set()
    for doc, r in zip(docs, results):
        for sc in r.scans:
            job = _job(sc)
            if job is None or sc.top <= sc.base:
                continue
            e = []
            if sc.base & 63 in EDGE_BITS:
                e.append("base & 63 == %d" % (sc.base & 63))
            if sc.top & 63 in EDGE_BITS:
                e.append("top & 63 == %d" % (sc.top & 63))
            tw, bw, wl = sc.top >> 6, sc.base >> 6, (sc.base + 1) >> 6
            if tw == bw:
                e.append("top and base in the same word")
            elif tw == bw + 1:
                e.append("top and base in adjacent words")
            elif tw - bw == STEP_WORDS:
                e.append("top and base exactly 64 words apart")
            elif tw - bw > STEP_WORDS and sc.steps in (2, 5):
                e.append("top and base more than 64 words apart: a scan of %d steps" % sc.steps)
            starts = o.starts(doc[:sc.p])
            if sc.q == sc.p - MARGIN:
                e.append("the safe start at top")
            if sc.q < sc.p - MARGIN and sc.p - MARGIN + 1 in starts and ref.safe_start(doc[sc.p - MARGIN + 1], doc[sc.p - MARGIN + 2]):
                e.append("a safe start at top + 1, not taken")
            if sc.q == 1:
                e.append("the safe start at prefix byte 1")
            if sc.q == 0:
                e.append("no safe start")
            else:
                if (sc.step, sc.lane) == (0, 0):
                    e.append("found by lane 0")
                if (sc.step, sc.lane) == (0, 63):
                    e.append("found by lane 63")
                if (sc.step, sc.lane) == (1, 0):
                    e.append("found by lane 0 of the second step")
                if sc.word == wl:
                    e.append("found in word wl")
                above = [x for x in starts if sc.q < x <= sc.p - MARGIN and (sc.base + x) >> 6 == sc.word]
                if len(above) >= 2:
                    e.append("the safe start below several rejected bits of its word")
            out |= {"%s (%s)" % (x, job) for x in e}
    return out


SCAN_EDGES = {"%s (%s)" % (x, job) for job in ("a single-chunk job", "the second chunk") for x in
              ["base & 63 == %d" % b for b in EDGE_BITS] + ["top & 63 == %d" % b for b in EDGE_BITS]
              + ["top and base in the same word", "top and base in adjacent words", "top and base exactly 64 words apart",
                 "top and base more than 64 words apart: a scan of 2 steps", "top and base more than 64 words apart: a scan of 5 steps",
                 "the safe start at top", "a safe start at top + 1, not taken", "the safe start at prefix byte 1", "no safe start",
                 "found by lane 0", "found by lane 63", "found by lane 0 of the second step", "found in word wl",
                 "the safe start below several rejected bits of its word"]}


def gather_edges(docs, results, max_tokens):
    """(source % 16, destination % 16, length) of every document that one round gathers whole and decides."""
    P = ref.first_prefix(max_tokens)
    return {(g[1], g[2], g[3]) for doc, r in zip(docs, results) if r.status == 0 and len(doc) < P for g in r.gathers
            if g[3] == len(doc) and len(doc) in GATHER_LENGTHS}


GATHER_EDGES = {(s, d, L) for s in range(16) for d in range(16) for L in GATHER_LENGTHS}


def sum_edges(o, docs, results, mx):
    out = set()
    P = ref.first_prefix(mx)
    for doc, r in zip(docs, results):
        n = len(o.tokens(doc))
        branch = "p == len" if not r.scans or r.round > r.scans[-1].round else "the prefix"
        if mx in SUM_LIMITS:
            for k in (-1, 0, 1):
                if n == mx + k:
                    out.add("max_tokens %d: %d tokens, a %s document" % (mx, n - mx, "short" if len(doc) < P else "long"))
            out.add("max_tokens %d: decided by %s" % (mx, branch))
            for sc in r.scans:
                if sc.q > 0 and sc.n_tokens >= mx > 64 and sc.cum64 <= sc.q < sc.cum:
                    out.add("max_tokens %d: tokens 65 and later run past q" % mx)
        # the cut of the limit inside a character
        tl = o.tok_len(o.tokens(doc))
        nb = sum(tl[:mx])
        if nb < len(doc) and (doc[nb] & 0xC0) == 0x80:
            c = nb
            while (doc[c] & 0xC0) == 0x80:
                c -= 1
            width = 4 if doc[c] >= 0xF0 else 3 if doc[c] >= 0xE0 else 2
            out.add("max_tokens %d: the limit cuts a %d-byte character after %d bytes, %s" % (mx, width, nb - c, branch))
            if min(n, mx) - r.kept >= 2 and mx in SUM_LIMITS:
                out.add("max_tokens %d: the back-off drops %d tokens" % (mx, min(n, mx) - r.kept))
            if r.kept == 0:
                out.add("max_tokens %d: the back-off ends at keep == 0" % mx)
        if b"\xef\xbf\xbd" in doc[max(nb - 3, 0):nb + 3] and mx in SUM_LIMITS:
            out.add("max_tokens %d: U+FFFD at the limit" % mx)
    return out


SUM_EDGES = ({"max_tokens %d: %d tokens, a %s document" % (mx, k, w) for mx in SUM_LIMITS for k in (-1, 0, 1) for w in ("short", "long")}
             | {"max_tokens %d: decided by %s" % (mx, b) for mx in SUM_LIMITS for b in ("p == len", "the prefix")}
             | {"max_tokens %d: tokens 65 and later run past q" % mx for mx in SUM_LIMITS if mx > 64}
             | {"max_tokens %d: the limit cuts a %d-byte character after %d bytes, %s" % (mx, w, k, b) for mx in SUM_LIMITS
                for w, ks in ((4, (1, 2, 3)), (3, (1, 2))) for k in ks for b in ("p == len", "the prefix")}
             | {"max_tokens %d: the back-off drops %d tokens" % (mx, k) for mx in SUM_LIMITS for k in (2, 3)}
             | {"max_tokens %d: U+FFFD at the limit" % mx for mx in SUM_LIMITS}
             | {"max_tokens 2: the back-off ends at keep == 0", "max_tokens 2: the limit cuts a 4-byte character after 1 bytes, p == len",
                "max_tokens 2: the limit cuts a 4-byte character after 2 bytes, p == len",
                "max_tokens 2: the limit cuts a 4-byte character after 2 bytes, the prefix",
                "max_tokens 2: the limit cuts a 3-byte character after 2 bytes, p == len"})


def round_edges(results, rounds):
    out = set()
    for r, rd in enumerate(rounds, 1):
        if r < 2 or not rd.open_items:
            continue
        op = set(rd.open_items)
        blocks = -(-rd.n_in // PLAN_BLOCK)
        for b in range(1, blocks):
            if b * PLAN_BLOCK - 1 in op and b * PLAN_BLOCK in op:
                out.add("round %d: survivors at items %d and %d" % (r, b * PLAN_BLOCK - 1, b * PLAN_BLOCK))
        if not any(j < PLAN_BLOCK for j in op) and rd.n_in > PLAN_BLOCK:
            out.add("round %d: the first plan block is empty" % r)
        if rd.n_act > PLAN_BLOCK:
            out.add("round %d: more than 1024 survivors" % r)
        if blocks >= 2 and r >= 3:
            out.add("round %d: two plan blocks" % r)
        if any(j % 2 for j in op) and any(j % 2 == 0 for j in op) and any(j % PLAN_ITEMS for j in op):
            out.add("round %d: survivors at indices neither all even nor all multiples of 4" % r)
        if r >= 3 and 0 < rd.n_act < rd.n_in:
            out.add("round %d: some items closed, some open" % r)
    return out


ROUND_EDGES = {"round 2: survivors at items 2047 and 2048", "round 2: survivors at items 1023 and 1024", "round 3: survivors at items 1023 and 1024",
               "round 2: the first plan block is empty", "round 2: more than 1024 survivors", "round 3: two plan blocks",
               "round 2: survivors at indices neither all even nor all multiples of 4",
               "round 3: survivors at indices neither all even nor all multiples of 4", "round 3: more than 1024 survivors",
               "round 4: some items closed, some open", "round 4: two plan blocks",
               "round 4: survivors at indices neither all even nor all multiples of 4"}


def special_edges(enc, docs, offset):
    lits = literals(enc)
    out = set()
    starts, pos = [], 0
    for d in docs:
        starts.append(pos)
        pos += len(d)
    n_bytes = pos
    firsts = collections.Counter(l[0] for l in lits)
    for d, s0 in zip(docs, starts):
        hits = [(i, lit) for lit in lits for i in range(len(d)) if d.startswith(lit, i)]
        for i, lit in hits:
            mem = offset + s0 + i
            out.add("offset %d: a literal at byte %d of a block" % (offset, mem % BLOCK))
            if mem // BLOCK != (mem + len(lit) - 1) // BLOCK:
                out.add("offset %d: a literal across a block edge" % offset)
            if mem // SPECIAL_WG != (mem + len(lit) - 1) // SPECIAL_WG:
                out.add("offset %d: a literal across a workgroup edge" % offset)
            if s0 + i == 0:
                out.add("offset %d: a literal at text byte 0" % offset)
            if s0 + i + len(lit) == n_bytes:
                out.add("offset %d: a literal ending at n_bytes" % offset)
            if i + len(lit) == len(d):
                out.add("a literal ending at its document's end")
            if i == 0:
                out.add("a literal starting at its document's start")
            if any(j == i + len(lit) for j, _ in hits):
                out.add("two adjacent literals")
            if len(lit) > 1 and d[max(i - 2, 0):i] == lit[:2]:
                out.add("a literal behind its own first two bytes")
            if len(lit) == 1:
                out.add("a 1-byte literal")
            if len(lit) > 32:
                out.add("a literal of more than 32 bytes")
            if lit[:1] != b"<":
                out.add("a literal that does not start with <")
            if any(o != lit and o.startswith(lit) for o in lits) and not any(d.startswith(o, i) for o in lits if o != lit and o.startswith(lit)):
                out.add("a literal that is a prefix of another, alone")
            if firsts[lit[0]] == 4:
                out.add("literal %d of four sharing a first byte" % sorted(l for l in lits if l[0] == lit[0]).index(lit))
    for a in range(len(docs)):
        b = a + 1
        while b < len(docs) and not docs[b]:
            b += 1
        if b < len(docs) and docs[a]:
            for lit in lits:
                for k in range(1, len(lit)):
                    if docs[a].endswith(lit[:k]) and docs[b].startswith(lit[k:]) and not any(l in docs[a] or l in docs[b] for l in lits):
                        out.add("a literal split across two documents with %d empty ones between" % (b - a - 1))
    return out


def special_edges_required(enc):
    lits = literals(enc)
    out = {"offset %d: a literal at byte %d of a block" % (o, r) for o in SPECIAL_OFFSETS for r in range(BLOCK)}
    out |= {"offset %d: %s" % (o, x) for o in SPECIAL_OFFSETS for x in
            ("a literal across a block edge", "a literal across a workgroup edge", "a literal at text byte 0", "a literal ending at n_bytes")}
    out |= {"a literal ending at its document's end", "a literal starting at its document's start", "two adjacent literals",
            "a literal behind its own first two bytes"}
    out |= {"a literal split across two documents with %d empty ones between" % r for r in EMPTY_RUNS}
    if enc == CUSTOM["name"]:
        out |= {"a 1-byte literal", "a literal of more than 32 bytes", "a literal that does not start with <",
                "a literal that is a prefix of another, alone"}
    else:
        assert all(l[:1] == b"<" for l in lits)
    if enc == "p50k_edit":
        out |= {"literal %d of four sharing a first byte" % i for i in range(4)}
    return out
