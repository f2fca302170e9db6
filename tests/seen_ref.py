"""The plain restatement of the seen-set rule (jtk_seen_set_*, jtk_batch_seen_mark; the rule is quoted in include/jtokkit_amd.h):
units by Python string operations (lines_ref.units_of; DOCUMENT is a strip of the document), the hash in Python integers modulo
2^64, the set a dict key -> [first, count].  It shares no code with jtokkit_amd/csrc/jtk_seen_rules.h and knows no table."""
import numpy as np

import lines_ref as lr

LINE, PARAGRAPH, DOCUMENT = 0, 1, 2
TRIM = 2
ADD, QUERY = 1, 2
DUP, FREQUENT = 1, 2
KEY_C = 193
ABSENT = lr.M64
PER_UNIT = (("unit_begin", np.int64), ("unit_end", np.int64), ("unit_first", np.uint64), ("unit_count", np.uint64), ("unit_flags", np.uint8))
PER_DOC = (("n_dup", np.int32), ("dup_bytes", np.int64), ("dup_chars", np.int64), ("unit_bytes", np.int64), ("unit_chars", np.int64))


def key_of(seed, unit):
    return lr.mix(seed + lr.G * (unit + KEY_C))


def pos_of(D, u):
    assert 0 <= D < 1 << 40 and 0 <= u < 1 << 24
    return (D << 24) | u


def capacity(c, m):
    cap = 64
    while cap < 2 * (c + m):
        cap *= 2
    return cap


def units_of(doc, unit, trim):
    if unit != DOCUMENT:
        return lr.units_of(doc, unit, trim)
    strip = b"\n" + (lr.BLANKS if trim else b"")
    core = doc.strip(strip)
    b = len(doc) - len(doc.lstrip(strip))
    return [(b, b + len(core))] if core else []


class Set:
    def __init__(self, unit=LINE, trim=False, seed=0):
        self.unit, self.trim, self.key = unit, trim, key_of(seed, unit)
        self.d, self.cap = {}, 64

    def add_entries(self, keys, first, count):
        self.cap = max(self.cap, capacity(len(self.d), len(keys)))
        for k, f, c in zip(keys, first, count):
            e = self.d.setdefault(int(k), [ABSENT, 0])
            e[0], e[1] = min(e[0], int(f)), e[1] + int(c)

    def entries(self):
        ks = sorted(self.d)
        return tuple(np.array(x, dtype=np.uint64) for x in (ks, [self.d[k][0] for k in ks], [self.d[k][1] for k in ks]))

    def mark(self, docs, status, mode=ADD | QUERY, base=0, min_count=0):
        nd = len(docs)
        off = np.concatenate([[0], np.cumsum([len(x) for x in docs])]).astype(np.int64)
        units = []                                               # (d, begin, end, k, pos)
        for d, doc in enumerate(docs):
            for u, (b, e) in enumerate([] if status[d] < 0 else units_of(doc, self.unit, self.trim)):
                units.append((d, off[d] + b, off[d] + e, lr.k_of(doc[b:e], self.key), pos_of(base + d, u), lr.chars_of(doc[b:e])))
        if mode & ADD and units:
            self.add_entries([x[3] for x in units], [x[4] for x in units], [1] * len(units))
        if not mode & QUERY:
            return None
        r = {name: np.zeros(len(units), dtype=dt) for name, dt in PER_UNIT}
        r.update({name: np.zeros(nd, dtype=dt) for name, dt in PER_DOC})
        r["unit_off"] = np.zeros(nd + 1, dtype=np.int64)
        for i, (d, b, e, k, pos, chars) in enumerate(units):
            first, count = self.d.get(k, (ABSENT, 0))
            dup = first < pos
            r["unit_begin"][i], r["unit_end"][i], r["unit_first"][i], r["unit_count"][i] = b, e, first, count
            r["unit_flags"][i] = (DUP if dup else 0) | (FREQUENT if min_count > 0 and count >= min_count else 0)
            r["unit_off"][d + 1] += 1
            r["unit_bytes"][d] += e - b
            r["unit_chars"][d] += chars
            if dup:
                r["n_dup"][d] += 1
                r["dup_bytes"][d] += e - b
                r["dup_chars"][d] += chars
        r["unit_off"] = np.cumsum(r["unit_off"])
        return r
