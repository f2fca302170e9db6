"""Plain restatement of the character-position rule (jtokkit_amd/csrc/jtk_charpos_rules.h), independent of the header's
formulation: no index, no word tricks.  For a well-formed document the counts come from Python's own decoder --
len(bytes[:q].decode("utf-8")) for code points, len(s.encode("utf-16-le")) // 2 for UTF-16 units --, for any other document from
a loop over its bytes.  Used by the CPU tier (against the header through tests/charpos_sim) and the GPU tier."""
import bisect

import numpy as np

BYTE, UTF16, CODEPOINT = 0, 1, 2
FLOOR, CEIL = 0, 1
UNITS = (BYTE, UTF16, CODEPOINT)
ROUNDS = (FLOOR, CEIL)


def well_formed(doc):
    try:
        doc.decode("utf-8")
        return True
    except UnicodeDecodeError:
        return False


def _str_units(s, unit):
    if unit == CODEPOINT:
        return len(s)
    if unit == UTF16:
        return len(s.encode("utf-16-le")) // 2
    return len(s.encode("utf-8"))


def _weight(x, unit):
    if unit == BYTE:
        return 1
    return (0 if (x & 0xC0) == 0x80 else 1) + (1 if unit == UTF16 and x >= 0xF0 else 0)


class DocRef:
    """One document: U[q] = U(a, a + q) for q = 0 .. len, and its boundaries (offsets from a, ascending)."""

    def __init__(self, doc, unit):
        n = len(doc)
        self.n = n
        self.well_formed = well_formed(doc)
        if self.well_formed and unit != BYTE:
            s = doc.decode("utf-8")
            starts = [0]
            for ch in s:
                starts.append(starts[-1] + len(ch.encode("utf-8")))
            assert starts[-1] == n
            self.bounds = sorted(set(starts))                              # character starts and the end
            U = [0] * (n + 1)
            for i, ch in enumerate(s):
                q0, q1 = starts[i], starts[i + 1]
                before = _str_units(doc[:q0].decode("utf-8"), unit)
                U[q0] = before
                for q in range(q0 + 1, q1):                                # inside the character: its first byte is counted
                    U[q] = before + _str_units(ch, unit)
            U[n] = _str_units(s, unit)
            self.U = U
        else:
            U = [0]
            for x in doc:
                U.append(U[-1] + _weight(x, unit))
            self.U = U
            self.bounds = [q for q in range(n + 1) if q == 0 or q == n or (doc[q] & 0xC0) != 0x80]
        self.units = self.U[n]

    def snap(self, p, rnd):
        i = bisect.bisect_right(self.bounds, p) - 1 if rnd == FLOOR else bisect.bisect_left(self.bounds, p)
        q = self.bounds[i]
        return q if abs(q - p) <= 3 else p

    def char_index(self, p, rnd):
        return self.U[self.snap(p, rnd)]

    def byte_pos(self, k):
        """The largest boundary q with U[q] <= k (offset from a); -1 for k < 0."""
        if k < 0:
            return -1
        if k >= self.units:
            return self.n
        best = 0
        for q in self.bounds:                                              # (U is non-decreasing along the boundaries)
            if self.U[q] <= k:
                best = q
            else:
                break
        return best


class Ref:
    def __init__(self, docs):
        self.docs = [bytes(d) for d in docs]
        self.doc_off = np.zeros(len(docs) + 1, dtype=np.int64)
        if docs:
            np.cumsum([len(d) for d in docs], out=self.doc_off[1:])
        self.n_bytes = int(self.doc_off[-1])
        self.text = np.frombuffer(b"".join(self.docs), dtype=np.uint8) if self.n_bytes else np.zeros(0, dtype=np.uint8)
        self._cache = {}

    def doc(self, d, unit):
        if (d, unit) not in self._cache:
            self._cache[(d, unit)] = DocRef(self.docs[d], unit)
        return self._cache[(d, unit)]

    def doc_units(self, unit):
        return np.array([self.doc(d, unit).units for d in range(len(self.docs))], dtype=np.int64)

    def doc_of(self, p):
        """The last d with doc_off[d] <= p; n_bytes belongs to the last document; -1 outside the text or without documents."""
        if p < 0 or p > self.n_bytes or not self.docs:
            return -1
        return min(int(np.searchsorted(self.doc_off, p, side="right")) - 1, len(self.docs) - 1)

    def char_index(self, d, p, unit, rnd):
        if d < 0 or d >= len(self.docs):
            return -1
        a, e = int(self.doc_off[d]), int(self.doc_off[d + 1])
        if p < a or p > e:
            return -1
        return self.doc(d, unit).char_index(p - a, rnd)

    def byte_pos(self, d, k, unit):
        if d < 0 or d >= len(self.docs) or k < 0:
            return -1
        return int(self.doc_off[d]) + self.doc(d, unit).byte_pos(k)

    # ---- the query sets of both tiers
    def all_positions(self):
        """Every byte position 0 .. n_bytes, plus one on either side (outside: -1), with the document each belongs to when the
        caller names it: positions on a document edge are asked for BOTH documents."""
        pos, doc = [], []
        for d in range(len(self.docs)):
            a, e = int(self.doc_off[d]), int(self.doc_off[d + 1])
            for p in range(a, e + 1):
                pos.append(p)
                doc.append(d)
            pos += [a - 1, e + 1]                                          # outside [a, e]
            doc += [d, d]
        pos += [0, 0]
        doc += [-1, len(self.docs)]                                        # bad documents
        return np.array(pos, dtype=np.int64), np.array(doc, dtype=np.int64)

    def free_positions(self):
        return np.arange(-1, self.n_bytes + 2, dtype=np.int64)

    def expected_char_positions(self, unit, rnd, pos, doc=None):
        if doc is None:
            return np.array([self.char_index(self.doc_of(int(p)), int(p), unit, rnd) for p in pos], dtype=np.int64)
        return np.array([self.char_index(int(d), int(p), unit, rnd) for p, d in zip(pos, doc)], dtype=np.int64)

    def all_char_queries(self, unit):
        """Every (d, k) with k from -1 to doc_units + 2, and two bad documents."""
        doc, k = [], []
        for d, u in enumerate(self.doc_units(unit)):
            for x in range(-1, int(u) + 3):
                doc.append(d)
                k.append(x)
        doc += [-1, len(self.docs)]
        k += [0, 0]
        return np.array(doc, dtype=np.int64), np.array(k, dtype=np.int64)

    def expected_byte_positions(self, unit, doc, k):
        return np.array([self.byte_pos(int(d), int(x), unit) for d, x in zip(doc, k)], dtype=np.int64)
