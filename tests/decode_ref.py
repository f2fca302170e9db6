"""Plain restatement of batch decode (Encoding.decodeBytes for many token lists, GptBytePairEncoding.java:137-151, 302-314),
by the contract in include/jtokkit_amd.h: the checker of tests/test_decode_gpu.py.  Python and numpy only; it builds its own
id -> bytes table from a rank map or a .tiktoken file and shares no code with the library or with the CPU oracle
(tests/test_decode_ref_cpu.py shows the two agree before the device is judged by this one).
"""
import base64

import numpy as np

JTK_OK = 0
JTK_ERR_UNKNOWN_TOKEN = -3


def parse_tiktoken(data):
    """The lines `base64(bytes) rank` of a .tiktoken file -> {bytes: rank}."""
    ranks = {}
    for line in data.splitlines():
        if line.strip():
            tok, rank = line.split()
            ranks[base64.b64decode(tok)] = int(rank)
    return ranks


class DecodeTable:
    """id -> bytes of one encoding: the rank table, then the special tokens' literals for ids the table does not hold
    (GptBytePairEncoding.java:302-314 looks in the table first, so a table id wins over a special with the same id)."""

    def __init__(self, ranks, specials=None):
        self.table = {}
        for tok, rank in ranks.items():
            self.table[int(rank)] = bytes(tok)
        self.specials = {}
        for lit, i in (specials or {}).items():
            self.specials[int(i)] = lit if isinstance(lit, bytes) else lit.encode("utf-8")
        self.n_table = max(self.table) + 1                                # ids of the rank table lie below this
        for i, lit in self.specials.items():
            self.table.setdefault(i, lit)
        self.n_ids_table = max(self.table) + 1                            # every id at or above this has no entry
        self._len = np.zeros(self.n_ids_table, dtype=np.int64)
        for i, tok in self.table.items():
            self._len[i] = len(tok)
        self._by_len = None

    @classmethod
    def from_tiktoken(cls, path_or_bytes, specials=None):
        data = path_or_bytes
        if not isinstance(data, (bytes, bytearray)):
            with open(path_or_bytes, "rb") as f:
                data = f.read()
        return cls(parse_tiktoken(bytes(data)), specials)

    def lengths(self, ids):
        """Byte length of every id; 0 where the id has no entry (negative, at or above n_ids_table, or a hole)."""
        ids = np.asarray(ids, dtype=np.int64)
        out = np.zeros(ids.shape, dtype=np.int64)
        ok = (ids >= 0) & (ids < self.n_ids_table)
        out[ok] = self._len[ids[ok]]
        return out

    def ids_by_length(self):
        """{byte length: the ids of that length, ascending}."""
        if self._by_len is None:
            by = {}
            for i in sorted(self.table):
                by.setdefault(len(self.table[i]), []).append(i)
            self._by_len = {l: np.array(v, dtype=np.int64) for l, v in by.items()}
        return self._by_len

    def holes(self):
        """Ids below n_ids_table without an entry, ascending."""
        return np.flatnonzero(self._len == 0)

    def decode_ref(self, ids, seq_off):
        """-> (out: bytes, byte_off: int64[n_seqs+1], status: int32[n_seqs]).  An id without an entry contributes no bytes and
        gives JTK_ERR_UNKNOWN_TOKEN to the sequence that contains it, and to no other."""
        ids = np.asarray(ids).tolist()
        seq_off = np.asarray(seq_off).tolist()
        n_seqs = len(seq_off) - 1
        parts = []
        byte_off = np.zeros(n_seqs + 1, dtype=np.int64)
        status = np.zeros(n_seqs, dtype=np.int32)
        get = self.table.get
        n = 0
        for q in range(n_seqs):
            toks = [get(i) for i in ids[seq_off[q]:seq_off[q + 1]]]
            if None in toks:
                status[q] = JTK_ERR_UNKNOWN_TOKEN
                toks = [t for t in toks if t is not None]
            s = b"".join(toks)
            parts.append(s)
            n += len(s)
            byte_off[q + 1] = n
        return b"".join(parts), byte_off, status
