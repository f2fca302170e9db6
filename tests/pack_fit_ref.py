"""Plain restatement of the best-fit-decreasing rule of jtk_batch_pack_best_fit (jtokkit_amd/csrc/jtk_pack_fit_rules.h), written
from the rule text: one rest at a time into the row with the least free space that fits, oldest change first among equals;
segments and positions read off the finished rows."""
import numpy as np

import pack_ref


def pack(docs, status, L, sep_id=-1, sep_first=False, pad_id=-1):
    """docs: per-document id lists, status: per-document status.  The result dict of pack_ref.pack."""
    rows, rests = [], []                             # a row: a list of (document, id)
    for d, u in pack_ref.units(docs, status, sep_id, sep_first):
        for i in range(0, len(u) - len(u) % L, L):
            rows.append([(d, t) for t in u[i:i + L]])
        if len(u) % L:
            rests.append((d, u[len(u) - len(u) % L:]))
    rests.sort(key=lambda x: (-len(x[1]), x[0]))
    open_rows = []                                   # [free, stamp of the last placed rest, row]
    for stamp, (d, ids) in enumerate(rests):
        fits = [o for o in open_rows if o[0] >= len(ids)]
        if fits:
            o = min(fits, key=lambda x: (x[0], x[1]))
        else:
            o = [L, stamp, []]
            open_rows.append(o)
            rows.append(o[2])
        o[2].extend((d, t) for t in ids)
        o[0] -= len(ids)
        o[1] = stamp
    cells = [row + [(-1, pad_id)] * (L - len(row)) for row in rows]
    n_rows = len(cells)
    out_rows = np.array([[t for _, t in row] for row in cells], dtype=np.int32).reshape(n_rows, L)
    positions = np.zeros((n_rows, L), dtype=np.int32)
    seg_len, seg_doc = [], []
    for r, row in enumerate(cells):
        for c, (d, _) in enumerate(row):
            # a new segment at the row start, at a change of document or between a piece and pad (two pieces of one document
            # never share a row)
            if c == 0 or d != row[c - 1][0]:
                seg_len.append(0)
                seg_doc.append(d)
            positions[r, c] = seg_len[-1]
            seg_len[-1] += 1
    cu = np.zeros(len(seg_len) + 1, dtype=np.int32)
    if seg_len:
        np.cumsum(seg_len, out=cu[1:])
    return dict(rows=out_rows, positions=positions, cu_seqlens=cu, seg_doc=np.array(seg_doc, dtype=np.int64),
                max_seqlen=max(seg_len) if seg_len else 0)
