"""Test infrastructure: a plain restatement of the token-budget chunking rule of jtk_batch_chunk
(jtokkit_amd/csrc/jtk_chunk_rules.h), and per-id byte tables from the CPU oracle.  The product never imports it."""
import numpy as np

import oracle_lib


def chunks(first_bytes, N, overlap):
    """first_bytes[i]: first byte of token i's byte string (0 if empty) -> [(s, e, split)] by the rule, verbatim."""
    n = len(first_bytes)

    def B(i):
        return i == 0 or i == n or (int(first_bytes[i]) & 0xC0) != 0x80

    out = []
    s = 0
    while s < n:
        hi = min(s + N, n)
        e = next((i for i in range(hi, s, -1) if B(i)), hi)
        out.append((s, e, not (B(s) and B(e))))
        if e == n:
            break
        if overlap == 0:
            s = e
        else:
            s = next((i for i in range(max(e - overlap, s + 1), e + 1) if B(i)), e)
    return out


class IdTables:
    """First byte and byte length of every id the oracle can decode (rank table and special tokens)."""

    def __init__(self, o, max_id=None):
        if max_id is None:
            max_id = 0
            for cfg in oracle_lib.ENCODINGS.values():
                max_id = max(max_id, max(cfg["specials"].values()))
            max_id = max(max_id, 100300)
        self.first = np.zeros(max_id + 1, dtype=np.uint8)
        self.length = np.zeros(max_id + 1, dtype=np.int64)
        for i in range(max_id + 1):
            try:
                b = o.decode_bytes([i])
            except oracle_lib.OracleError:
                continue
            self.length[i] = len(b)
            self.first[i] = b[0] if b else 0


def first_bytes(o, toks, cache={}):
    """First byte of every token of `toks` (a list), looked up id by id."""
    out = np.zeros(len(toks), dtype=np.uint8)
    for j, t in enumerate(toks):
        key = (o.name, t)
        if key not in cache:
            b = o.decode_bytes([t])
            cache[key] = b[0] if b else 0
        out[j] = cache[key]
    return out
