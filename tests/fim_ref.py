"""A plain restatement of the fill-in-the-middle rule (JTK_ENCODE_FIM), written from its description and not from the header
jtokkit_amd/csrc/jtk_fim_rules.h: test infrastructure only.  Python integers, one document at a time, no tiles.

    draws   mix = the splitmix64 finaliser; draw(g, k) = mix(mix(seed + 0x9E3779B97F4A7C15 (g + 1)) + k) modulo 2^64
    kind    0 for an empty document, 0 when the top 32 bits of draw(g, 0) are >= fim_rate (unless fim_rate is 0xFFFFFFFF),
            else 2 (SPM) when the top 32 bits of draw(g, 1) are < spm_rate or spm_rate is 0xFFFFFFFF, else 1 (PSM)
    cuts    floor(draw(g, 2 + k) (len + 1) / 2^64) for k = 0, 1, each moved back over at most 3 continuation bytes while it is
            strictly inside the document; a = the smaller, b = the larger
    ids     PSM: PRE enc(prefix) SUF enc(suffix) MID enc(middle);  SPM: PRE SUF enc(suffix) MID enc(prefix) enc(middle)
"""
import numpy as np

M64 = (1 << 64) - 1
ALWAYS = 0xFFFFFFFF
NONE, PSM, SPM = 0, 1, 2
BAD_UTF8 = -6


def rate_u32(rate):
    return min(int(rate * 2 ** 32), 2 ** 32 - 1)


def mix(x):
    x &= M64
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & M64
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & M64
    x ^= x >> 31
    return x


def draw(seed, g, k):
    return mix(mix(seed + 0x9E3779B97F4A7C15 * (g + 1)) + k)


def kind_of(seed, g, length, fim_rate, spm_rate):
    if length == 0:
        return NONE
    if fim_rate != ALWAYS and (draw(seed, g, 0) >> 32) >= fim_rate:
        return NONE
    if spm_rate == ALWAYS or (draw(seed, g, 1) >> 32) < spm_rate:
        return SPM
    return PSM


def raw_cut(seed, g, k, length):
    """Before snapping: uniform over [0, length]."""
    return (draw(seed, g, 2 + k) * (length + 1)) >> 64


def snap(doc, p):
    steps = 0
    while p < len(doc) and p > 0 and 0x80 <= doc[p] <= 0xBF and steps < 3:
        p -= 1
        steps += 1
    return p


def cuts_of(doc, seed, g):
    p = [snap(doc, raw_cut(seed, g, k, len(doc))) for k in (0, 1)]
    return min(p), max(p)


def transform(doc, seed, g, fim_rate, spm_rate):
    """(kind, a, b) of one document (bytes); a = b = len for an untouched one."""
    kind = kind_of(seed, g, len(doc), fim_rate, spm_rate)
    if kind == NONE:
        return kind, len(doc), len(doc)
    a, b = cuts_of(doc, seed, g)
    return kind, a, b


def well_formed(doc):
    try:
        doc.decode("utf-8")
        return True
    except UnicodeDecodeError:
        return False


def encode_doc(encode, doc, kind, a, b, ids, validate=False):
    """(status, ids, part_tok) of one document.  encode(bytes) -> list of ids, or a negative status."""
    if validate and not well_formed(doc):
        return BAD_UTF8, [], (0, 0, 0)
    if kind == NONE:
        parts = [encode(doc), [], []]
    else:
        parts = [encode(doc[:a]), encode(doc[a:b]), encode(doc[b:])]
    bad = [p for p in parts if not isinstance(p, list)]
    if bad:
        return min(bad), [], (0, 0, 0)
    pre, mid, suf = parts
    count = tuple(len(p) for p in parts)
    if kind == NONE:
        return 0, pre, count
    if kind == PSM:
        return 0, [ids[0]] + pre + [ids[2]] + suf + [ids[1]] + mid, count
    return 0, [ids[0], ids[2]] + suf + [ids[1]] + pre + mid, count


class Result:
    pass


def encode_batch(encode, docs, seed, doc_index_base, fim_rate, spm_rate, ids, validate=False):
    """ids = (prefix_id, middle_id, suffix_id).  Arrays as the ABI hands them back, plus sub_off."""
    r = Result()
    n = len(docs)
    r.kind = np.zeros(n, dtype=np.uint8)
    r.cut = np.zeros((n, 2), dtype=np.int64)
    r.part_tok = np.zeros((n, 3), dtype=np.int64)
    r.status = np.zeros(n, dtype=np.int32)
    r.tok_off = np.zeros(n + 1, dtype=np.int64)
    r.sub_off = np.zeros(3 * n + 1, dtype=np.int64)
    r.docs = []
    pos = 0
    for d, doc in enumerate(docs):
        kind, a, b = transform(doc, seed, doc_index_base + d, fim_rate, spm_rate)
        st, toks, count = encode_doc(encode, doc, kind, a, b, ids, validate)
        r.kind[d], r.cut[d], r.part_tok[d], r.status[d] = kind, (a, b), count, st
        r.sub_off[3 * d:3 * d + 3] = (pos, pos + a, pos + b)
        pos += len(doc)
        r.tok_off[d + 1] = r.tok_off[d] + len(toks)
        r.docs.append(toks)
    r.sub_off[3 * n] = pos
    r.tokens = np.array([t for toks in r.docs for t in toks], dtype=np.int32)
    return r
