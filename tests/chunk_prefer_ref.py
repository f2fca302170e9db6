"""Test infrastructure: a plain restatement of the boundary-preferring chunking rule of jtk_batch_chunk_prefer
(jtokkit_amd/csrc/jtk_chunk_prefer_rules.h), on the byte strings of a document's tokens.  The product never imports it."""

WORD, SENTENCE, LINE, PARAGRAPH = 1, 2, 4, 8
SPLIT_, CHAR_, WORD_, SENTENCE_, LINE_, PARAGRAPH_, DOC_END_ = range(7)
WS = frozenset(b" \t\n\v\f\r")
STOPS = frozenset(b".!?")
CJK_STOPS = (b"\xe3\x80\x82", b"\xef\xbc\x81", b"\xef\xbc\x9f")

PARA = ("The quick brown fox jumps over the lazy dog. Is it done? Yes! It costs 3.14 dollars, e.g. today.\nA second line "
        "follows here.\n\nNew paragraph: they'll see.\r\n\r\nWindows paragraph.  Two spaces.\n    indented code(line);\n")
CJK = "日本語のテキストを分割する。次の文です！本当に？はい。"
EMOJI = "\U0001F355\U0001F680" * 6 + " ok "
PROBE = (PARA * 6 + CJK * 3 + EMOJI * 2 + "漢字龘靐齉" * 4) * 2


def token_bytes(o, toks, cache={}):
    """The byte string of every token of `toks`, from the oracle, id by id."""
    out = []
    for t in toks:
        key = (o.name, int(t))
        if key not in cache:
            cache[key] = o.decode_bytes([int(t)])
        out.append(cache[key])
    return out


def levels(tok_bytes, prefer):
    """level(i) for every token i of one document (6 for i = 0), from the decoded stream D."""
    D = b"".join(tok_bytes)
    out = []
    p = 0
    for i, tb in enumerate(tok_bytes):
        if i == 0:
            out.append(DOC_END_)
            p += len(tb)
            continue
        y = D[p]
        x = D[max(p - 3, 0):p][::-1]                      # x[0] = x(1), ...; shorter at the document's start
        x1 = x[0] if len(x) > 0 else None
        x2 = x[1] if len(x) > 1 else None
        x3 = x[2] if len(x) > 2 else None
        if (y & 0xC0) == 0x80:
            lv = SPLIT_
        else:
            lv = CHAR_
            if prefer & WORD and (y in WS or x1 in WS):
                lv = WORD_
            if prefer & SENTENCE and ((x1 in STOPS and y in WS) or (x1 in WS and x2 in STOPS)
                                      or (len(x) == 3 and bytes(x[::-1]) in CJK_STOPS)):
                lv = SENTENCE_
            line = x1 == 0x0A and y not in (0x0A, 0x0D)
            if prefer & LINE and line:
                lv = LINE_
            if prefer & PARAGRAPH and line and (x2 == 0x0A or (x2 == 0x0D and x3 == 0x0A)):
                lv = PARAGRAPH_
        out.append(lv)
        p += len(tb)
    return out


def chunks_fast(level, N, overlap, min_tokens):
    """chunks() with the two window searches done by numpy where the window is wide: for the GPU tier's long documents and
    large N.  The CPU tier holds it equal to chunks()."""
    import numpy as np
    level = np.asarray(level, dtype=np.uint8)
    lv = level.tolist()
    n = len(lv)

    def search(a, b, last):
        """(m, the last / first i in [a, b) with level m), m the maximum there; (0, None) for an empty range."""
        if b <= a:
            return 0, None
        if b - a <= 16:
            seg = lv[a:b]
            m = max(seg)
            return m, (b - 1 - seg[::-1].index(m)) if last else (a + seg.index(m))
        seg = level[a:b]
        m = int(seg.max())
        hit = np.flatnonzero(seg == m)
        return m, a + int(hit[-1] if last else hit[0])

    out = []
    s = 0
    while s < n:
        hi = min(s + N, n)
        if hi == n:
            e, end_level = n, DOC_END_
        else:
            m, e = search(min(s + min_tokens, hi), hi + 1, True)
            if m == 0:                                    # the back-off: the last i in (s, hi] with B(i), or hi
                hit = np.flatnonzero(level[s + 1:hi + 1])
                e = s + 1 + int(hit[-1]) if len(hit) else hi
            end_level = lv[e]
        out.append((s, e, not ((s == 0 or lv[s] != 0) and (e == n or lv[e] != 0)), end_level))
        if e == n:
            break
        m, i = search(max(e - overlap, s + 1), e, False)
        s = i if m >= 1 else e
    return out


def chunks(level, N, overlap, min_tokens):
    """level[i] as levels() gives it -> [(s, e, split, end_level)] by the walk, verbatim."""
    n = len(level)

    def B(i):
        return i == 0 or i == n or level[i] != 0

    out = []
    s = 0
    while s < n:
        hi = min(s + N, n)
        if hi == n:
            e, end_level = n, DOC_END_
        else:
            lo = min(s + min_tokens, hi)
            m = max(level[i] for i in range(lo, hi + 1))
            if m >= 1:
                e = max(i for i in range(lo, hi + 1) if level[i] == m)
            else:
                e = next((i for i in range(hi, s, -1) if B(i)), hi)
            end_level = level[e]
        out.append((s, e, not (B(s) and B(e)), end_level))
        if e == n:
            break
        R = range(max(e - overlap, s + 1), e)
        m = max((level[i] for i in R), default=0)
        s = min(i for i in R if level[i] == m) if m >= 1 else e
    return out
