"""Plain restatement of the decode of an id matrix (jtk_batch_decode_rows*, by the contract in include/jtokkit_amd.h): the
checker of tests/test_decode_rows_rules_cpu.py and tests/test_decode_rows_gpu.py.  It picks the contributing cells of every row
in Python and hands the resulting lists to decode_ref.DecodeTable.decode_ref; it shares no code with the library.
"""
import numpy as np


def _clamp(v, width):
    return 0 if v < 0 else width if v > width else v


def decode_rows_ref(tab, rows, begin=None, end=None, pad_id=0, stop=(), skip_pad=False, keep_stop=False):
    """rows: 2-d integer array (any 64-bit values).  -> dict(out bytes, byte_off int64[n_rows + 1], status int32[n_rows],
    cell_byte int64[n_rows, width], first_stop int64[n_rows] (-1: none), contributes bool[n_rows, width])."""
    rows = np.asarray(rows)
    n_rows, width = rows.shape
    stop = set(int(s) for s in stop)
    lists, picked, first_stop = [], np.zeros((n_rows, width), dtype=bool), np.full(n_rows, -1, dtype=np.int64)
    for r in range(n_rows):
        row = rows[r].tolist()
        b = 0 if begin is None else _clamp(int(begin[r]), width)
        e = width if end is None else _clamp(int(end[r]), width)
        for c in range(b, e):                                             # the stop test comes first
            if row[c] in stop:
                first_stop[r] = c
                e = c + 1 if keep_stop else c
                break
        ids = []
        for c in range(b, e):
            if skip_pad and row[c] == pad_id:
                continue
            ids.append(row[c])
            picked[r, c] = True
        lists.append(ids)
    seq_off = np.zeros(n_rows + 1, dtype=np.int64)
    if n_rows:
        np.cumsum([len(x) for x in lists], out=seq_off[1:])
    flat = [i for x in lists for i in x]
    out, byte_off, status = tab.decode_ref(np.array(flat, dtype=np.int64) if flat else np.zeros(0, dtype=np.int64), seq_off)
    # where every cell's bytes start: the bytes of the contributing cells before it in row-major order
    lens = np.where(picked, tab.lengths(rows.astype(np.int64)), 0).reshape(-1)
    cell_byte = (np.cumsum(lens) - lens).reshape(n_rows, width).astype(np.int64)
    return dict(out=out, byte_off=byte_off, status=status, cell_byte=cell_byte, first_stop=first_stop, contributes=picked)
