"""The plain restatement of the line / paragraph rule (jtk_batch_line_units, jtk_batch_line_repeats; the rule is quoted in
include/jtokkit_amd.h): per document bytes.split(b"\\n"), a dict from k to (first, count), and the sums.  It shares no code with
jtokkit_amd/csrc/jtk_lines_rules.h, walks no tiles and knows no table.  `wrong` names one of WRONG_RULES: a plausible misreading
of the rule, which the case set must tell from the right one."""
import types

import numpy as np

G = 0x9E3779B97F4A7C15
M64 = (1 << 64) - 1
LINE, PARAGRAPH = 0, 1
MARK_FIRST, TRIM = 1, 2
KEY_C = 161
BLANKS = b" \t\r"
OUTS = ("unit_begin", "unit_end", "unit_flags", "unit_off", "n_dup", "dup_bytes", "dup_chars", "unit_bytes", "unit_chars", "doc_chars",
        "top_count", "top_first")
WRONG_RULES = ("cr_break", "trim_ignored", "trim_inner", "cross_doc", "para_single_newline", "modes_swapped", "chars_are_bytes",
               "hash_without_plus_one", "first_is_last", "refused_counted")
_H = {}


def mix(x):
    """The splitmix64 finaliser."""
    x &= M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def key_of(seed, unit):
    return mix(seed + G * (unit + KEY_C))


def doc_key(key, base, d):
    return mix(key + G * (((base + d) & M64) + 1))


def horner(data, plus=1):
    """H = H * G + byte + 1 over the bytes, from 0 (computed once per distinct byte string)."""
    if (data, plus) not in _H:
        h = 0
        for x in data:
            h = (h * G + x + plus) & M64
        _H[data, plus] = h
    return _H[data, plus]


def k_of(data, kd, plus=1):
    return mix(horner(data, plus) ^ kd) or G


def chars_of(data):
    a = np.frombuffer(data, dtype=np.uint8)
    return int(((a & 0xC0) != 0x80).sum())


def units_of(doc, unit, trim, wrong=None):
    """[(begin, end)] relative to the document, in text order."""
    blanks = BLANKS if trim and wrong != "trim_ignored" else b""
    brk = b"\n"
    text = doc.replace(b"\r", b"\n") if wrong == "cr_break" else doc
    lines, at = [], 0                                            # the non-blank raw lines as (begin, end) of their ink, None for a blank one
    for raw in text.split(brk):
        core = raw.strip(blanks) if blanks else raw
        if core:
            b = at + (len(raw) - len(raw.lstrip(blanks)) if blanks else 0)
            lines.append((b, b + len(core)))
        else:
            lines.append(None)
        at += len(raw) + 1
    if unit == LINE or wrong == "para_single_newline":
        return [x for x in lines if x]
    out, run = [], None
    for x in lines + [None]:
        if x:
            run = (run[0], x[1]) if run else x
        elif run:
            out.append(run)
            run = None
    return out


def repeats(docs, status, unit, trim=False, mark_first=False, seed=0, base=0, wrong=None):
    """Every result of the rule for a batch of documents (bytes) with their statuses."""
    if wrong == "modes_swapped":
        mark_first = not mark_first
    nd = len(docs)
    doc_off = np.zeros(nd + 1, dtype=np.int64)
    if nd:
        np.cumsum([len(x) for x in docs], out=doc_off[1:])
    key = key_of(seed, unit)
    per_doc = []
    for d, doc in enumerate(docs):
        per_doc.append([] if status[d] < 0 and wrong != "refused_counted" else [(doc_off[d] + b, doc_off[d] + e) for b, e in units_of(doc, unit, trim, wrong)])
    text = b"".join(docs)
    if wrong == "cross_doc":                                     # the batch as one text; a unit belongs to the document it begins in
        per_doc = [[] for _ in docs]
        for b, e in units_of(text, unit, trim):
            d = int(np.searchsorted(doc_off, b, side="right")) - 1
            if status[d] >= 0:
                per_doc[d].append((b, e))
    r = types.SimpleNamespace(ks=[])
    begin, end, flags = [], [], []
    r.unit_off = np.zeros(nd + 1, dtype=np.int64)
    r.n_dup, r.top_count = np.zeros(nd, dtype=np.int32), np.zeros(nd, dtype=np.int32)
    for name in ("dup_bytes", "dup_chars", "unit_bytes", "unit_chars", "doc_chars", "top_first"):
        setattr(r, name, np.zeros(nd, dtype=np.int64))
    for d, units in enumerate(per_doc):
        kd = doc_key(key, base, d)
        r.doc_chars[d] = len(docs[d]) if wrong == "chars_are_bytes" else chars_of(docs[d])
        seen, ks = {}, []
        for i, (b, e) in enumerate(units):
            data = text[b:e]
            if wrong == "trim_inner" and trim:
                data = bytes(x for x in data if x not in BLANKS)
            k = k_of(data, kd, 0 if wrong == "hash_without_plus_one" else 1)
            ks.append(k)
            first, count = seen.get(k, (i, 0))
            seen[k] = (i if wrong == "first_is_last" else first, count + 1)
        r.ks.append(ks)
        best = (0, -1)
        for i, ((b, e), k) in enumerate(zip(units, ks)):
            first, count = seen[k]
            rep = count >= 2 if mark_first else first < i
            nb, nc = e - b, (e - b if wrong == "chars_are_bytes" else chars_of(text[b:e]))
            begin.append(b), end.append(e), flags.append(1 if rep else 0)
            r.unit_bytes[d] += nb
            r.unit_chars[d] += nc
            if rep:
                r.n_dup[d] += 1
                r.dup_bytes[d] += nb
                r.dup_chars[d] += nc
            if first == i and count > best[0]:
                best = (count, i)
        r.top_count[d], r.top_first[d] = best
        r.unit_off[d + 1] = r.unit_off[d] + len(units)
    r.unit_begin, r.unit_end = np.array(begin, dtype=np.int64), np.array(end, dtype=np.int64)
    r.unit_flags = np.array(flags, dtype=np.uint8)
    return r


def capacity(m):
    c = 64
    while c < 2 * m:
        c *= 2
    return c


def groups(unit_counts, budget, slot_bytes=20):
    """[(d0, d1, units)]: whole consecutive documents while the table of their units stays within the budget."""
    out, d0 = [], 0
    while d0 < len(unit_counts):
        have, d = 0, d0
        while d < len(unit_counts) and not (d > d0 and capacity(have + unit_counts[d]) * slot_bytes > budget):
            have += unit_counts[d]
            d += 1
        out.append((d0, d, have))
        d0 = d
    return out
