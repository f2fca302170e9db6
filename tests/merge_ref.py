"""bytePairMerge (reference GptBytePairEncoding.java:200-275) on byte strings, as plainly as it can be said: parts are byte slices
of the piece, the rank of two neighbouring parts is a dict lookup of their joined bytes, the leftmost minimum wins (strict `<`,
:236), and after each merge the ranks of the merged part and of the part before it are looked up again (:254-257).  Nothing of
oracle/ or of the product is used; numpy only finds each step's minimum.

merge_ref returns the tokens and a trace of the steps, from which the case tests read what a piece exercises.  `mutant=` makes
the same function wrong in one of the ways a kernel can be wrong (a part that is then no table entry comes out as id -1):
  "rightmost"   the last minimum wins a tie
  "stale_prev"  the rank of the part before the merged one is not looked up again
  "stale_next"  the merged part's own rank is not looked up again: it keeps the rank that the removed part had with the part
                after it, as in a kernel that closes the gap and forgets the lookup
Every variant still ends with the piece: a rank other than NONE always belongs to a part that has a part after it.
"""
import base64
import os

import numpy as np

NONE = np.iinfo(np.int64).max
MUTANTS = ("rightmost", "stale_prev", "stale_next")
DATA_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "jtokkit_amd", "data")

_ranks = {}


def load_ranks(name):
    """bytes -> rank of a shipped rank file (p50k_edit shares p50k_base's)"""
    if name not in _ranks:
        r = {}
        with open(os.path.join(DATA_DIR, name + ".tiktoken"), "rb") as f:
            for line in f:
                if line.strip():
                    k, v = line.split()
                    r[base64.b64decode(k)] = int(v)
        _ranks[name] = r
    return _ranks[name]


class Trace:
    """One entry per merge step, all byte positions inside the piece.
    pos       where the chosen part starts
    last      where the last part with the minimum rank starts (== pos: no tie)
    tie       the minimum rank stood at more than one part
    removed   where the part that is merged into the chosen one starts
    ahead     bytes from the chosen part's start to the start of the part after next (0: there is none)
    prev_len  byte length of the part before the chosen one (0: there is none)"""
    FIELDS = ("pos", "last", "tie", "removed", "ahead", "prev_len")

    def __init__(self, rows):
        a = np.array(rows, dtype=np.int64).reshape(-1, len(self.FIELDS))
        for k, f in enumerate(self.FIELDS):
            setattr(self, f, a[:, k])
        self.tie = self.tie.astype(bool)

    def __len__(self):
        return len(self.pos)


def merge_ref(piece, ranks, mutant=None):
    """(token ids, Trace) of one piece (bytes) under the rank map `ranks`."""
    assert mutant is None or mutant in MUTANTS
    n = len(piece)
    start = list(range(n + 1))                      # start[i]: where part i begins; the last entry is the end of the piece
    rk = np.full(n + 1, NONE, dtype=np.int64)       # rk[i]: rank of part i joined with part i + 1

    def rank(i, j):                                 # of the bytes of parts i .. j - 1
        return ranks.get(piece[start[i]:start[j]], NONE) if j < len(start) else NONE

    for i in range(n - 1):
        rk[i] = rank(i, i + 2)
    rows = []
    m = n + 1                                       # live entries of start / rk
    while m > 1:
        live = rk[:m - 1]
        i = int(np.argmin(live))                    # the first of equal minima
        lowest = live[i]
        if lowest == NONE:
            break
        where = np.nonzero(live == lowest)[0]
        last = int(where[-1])
        if mutant == "rightmost":
            i = last
        rows.append((start[i], start[last], len(where) > 1, start[i + 1], start[i + 2] - start[i] if i + 3 < m else 0,
                     start[i] - start[i - 1] if i > 0 else 0))
        # both ranks are those of the parts as they will be once part i + 1 is gone
        rk[i] = rk[i + 1] if mutant == "stale_next" else rank(i, i + 3)
        if i > 0 and mutant != "stale_prev":
            rk[i - 1] = rank(i - 1, i + 2)
        del start[i + 1]
        rk[i + 1:m - 1] = rk[i + 2:m]
        m -= 1
    return [ranks.get(piece[start[i]:start[i + 1]], -1) for i in range(m - 1)], Trace(rows)
