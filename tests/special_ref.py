"""Plain restatement of the allow-special encode (JTK_ENCODE_ALLOW_SPECIAL, include/jtokkit_amd.h) -- test infrastructure only.

matches(): scan from the document's start; the next match is the leftmost position where some allowed literal occurs entirely
inside the document, the longest of those that match there; scanning resumes after it.  encode(): the segments between the
matches encoded as encodeOrdinary(segment) by the CPU oracle, each match's id in between."""


def matches(doc, allowed):
    """doc: bytes; allowed: {literal bytes: id} -> [(start, end, id)]."""
    out = []
    p = 0
    nxt = {lit: -2 for lit in allowed}         # next occurrence of each literal at or after p (-1: none)
    while True:
        best = None
        for lit, i in allowed.items():
            if nxt[lit] != -1 and nxt[lit] < p:
                nxt[lit] = doc.find(lit, p)
            q = nxt[lit]
            if q >= 0 and (best is None or q < best[0] or (q == best[0] and len(lit) > len(best[1]))):
                best = (q, lit, i)
        if best is None:
            break
        q, lit, i = best
        out.append((q, q + len(lit), i))
        p = q + len(lit)
    return out


def disallowed_in(doc, literals, allowed):
    """text.contains over the literals that are not allowed."""
    return any(lit in doc for lit in literals if lit not in allowed)


def encode(o, doc, allowed, literals=(), ordinary=False):
    """The token list, or None where the document is refused (a disallowed literal under encode())."""
    if not ordinary and disallowed_in(doc, literals, allowed):
        return None
    toks = []
    p = 0
    for s, e, i in matches(doc, allowed):
        toks += o.encode_ordinary(doc[p:s])
        toks.append(i)
        p = e
    toks += o.encode_ordinary(doc[p:])
    return toks
