"""Plain restatement of the stop-string rule (include/jtokkit_amd.h, jtk_batch_decode_find_stops), independent of
jtokkit_amd/csrc/jtk_stop_rules.h: bytes.find per string, the minimum over (p, i), the held-back tail by brute force over
every start, the column by a linear walk.  What the CPU shim and the GPU are compared with."""
import numpy as np


def as_bytes(strings):
    return [s.encode("utf-8") if isinstance(s, str) else bytes(s) for s in strings]


def find_stops(out, byte_off, strings, frm=None, cell_byte=None):
    """out: bytes; byte_off: n + 1 ascending positions; strings: list of bytes; frm: n ints or None; cell_byte: int array
    [n, width] or None -> (stop_pos int64, stop_which int32, hold int32, stop_col int64), each [n]."""
    out = bytes(out)
    strings = as_bytes(strings)
    n = len(byte_off) - 1
    maxlen = max([len(s) for s in strings], default=0)
    pos, col = np.zeros(n, dtype=np.int64), np.full(n, -1, dtype=np.int64)
    which, hold = np.full(n, -1, dtype=np.int32), np.zeros(n, dtype=np.int32)
    for q in range(n):
        b, e = int(byte_off[q]), int(byte_off[q + 1])
        f = 0 if frm is None else int(frm[q])
        s0 = b + min(max(f, 0), e - b)
        best = None
        for i, s in enumerate(strings):
            p = out.find(s, s0, e)                                  # (the whole match inside [s0, e))
            if p >= 0 and (best is None or (p, i) < best):
                best = (p, i)
        if best is not None:
            pos[q], which[q] = best
            if cell_byte is not None:
                c = -1
                for k in range(cell_byte.shape[1]):
                    if cell_byte[q, k] <= best[0]:
                        c = k
                col[q] = c
            continue
        pos[q] = e
        for p in range(max(s0, e - (maxlen - 1)), e):
            tail = out[p:e]
            if any(len(s) > len(tail) and s.startswith(tail) for s in strings):
                hold[q] = e - p
                break
    return pos, which, hold, col


def cut_rows(out, byte_off, pos, which, strings, keep_stop_string=False):
    """The rows cut at their stops, as the host methods return them."""
    out = bytes(out)
    strings = as_bytes(strings)
    return [out[int(byte_off[q]):int(pos[q]) + (len(strings[which[q]]) if keep_stop_string and which[q] >= 0 else 0)]
            for q in range(len(pos))]
