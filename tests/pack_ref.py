"""Plain restatement of the packing rule of jtk_batch_pack (jtokkit_amd/csrc/jtk_pack_rules.h), written from the rule text
and nothing else: units, the stream or next-fit of items, then segments and positions read off the finished rows."""
import numpy as np


def units(docs, status, sep_id=-1, sep_first=False):
    """[(document, unit ids)] in document order; documents with status < 0 and empty units are left out."""
    out = []
    for d, (ids, st) in enumerate(zip(docs, status)):
        if st < 0:
            continue
        ids = list(ids)
        if sep_id >= 0:
            u = [sep_id] + ids if sep_first else ids + [sep_id]
        else:
            u = ids
        if u:
            out.append((d, u))
    return out


def pack(docs, status, L, sep_id=-1, sep_first=False, whole=False, drop_last=False, pad_id=-1):
    """docs: per-document id lists (the last encode's ids), status: per-document status.  Returns a dict of rows, positions
    (int32 [n_rows, L]), cu_seqlens (int32 [n_seg + 1]), seg_doc (int64 [n_seg]) and max_seqlen."""
    us = units(docs, status, sep_id, sep_first)
    cells = []                                       # per row: a list of (document or -1, id)
    if not whole:
        stream = [(d, t) for d, u in us for t in u]
        n_rows = len(stream) // L if drop_last else -(-len(stream) // L)
        for r in range(n_rows):
            row = stream[r * L:(r + 1) * L]
            cells.append(row + [(-1, pad_id)] * (L - len(row)))
    else:
        assert not drop_last
        cur = None
        for d, u in us:
            for i in range(0, len(u), L):
                item = [(d, t) for t in u[i:i + L]]
                if cur is not None and len(cur) + len(item) <= L:
                    cur.extend(item)
                else:
                    if cur is not None:
                        cells.append(cur)
                    cur = list(item)
        if cur is not None:
            cells.append(cur)
        cells = [row + [(-1, pad_id)] * (L - len(row)) for row in cells]
    n_rows = len(cells)
    rows = np.array([[t for _, t in row] for row in cells], dtype=np.int32).reshape(n_rows, L)
    positions = np.zeros((n_rows, L), dtype=np.int32)
    seg_len, seg_doc = [], []
    for r, row in enumerate(cells):
        for c, (d, _) in enumerate(row):
            # a new segment at the row start, at a change of unit or between unit and pad.  Two units of the same document
            # never touch: a document has one unit.
            if c == 0 or d != row[c - 1][0]:
                seg_len.append(0)
                seg_doc.append(d)
            positions[r, c] = seg_len[-1]
            seg_len[-1] += 1
    cu = np.zeros(len(seg_len) + 1, dtype=np.int32)
    if seg_len:
        np.cumsum(seg_len, out=cu[1:])
    return dict(rows=rows, positions=positions, cu_seqlens=cu, seg_doc=np.array(seg_doc, dtype=np.int64),
                max_seqlen=max(seg_len) if seg_len else 0)


# ---- the same for batches too large for a per-cell loop: rows as slices of the stream S ---------------------------------

def row_starts(lengths, L, whole=False, drop_last=False):
    """lengths: the non-empty units' lengths in order.  Row r holds S[a[r], a[r + 1]) and then pad; returns a (n_rows + 1)."""
    S = int(sum(lengths))
    if not whole:
        n_rows = S // L if drop_last else -(-S // L)
        return np.array([r * L for r in range(n_rows)] + [min(n_rows * L, S)], dtype=np.int64)
    a, fill, pos = [], None, 0
    for n in lengths:
        for i in range(0, n, L):
            it = min(L, n - i)
            if fill is not None and fill + it <= L:
                fill += it
            else:
                a.append(pos)
                fill = it
            pos += it
    return np.array(a + [pos], dtype=np.int64)


def segments(unit_start, unit_doc, a, L):
    """cu_seqlens, seg_doc and max_seqlen from the rows' slices a (row_starts) and the non-empty units' starts in S."""
    a = np.asarray(a, dtype=np.int64)
    U = np.asarray(unit_start, dtype=np.int64)
    D = np.asarray(unit_doc, dtype=np.int64)
    n_rows = len(a) - 1
    if n_rows == 0:
        return np.zeros(1, dtype=np.int32), np.zeros(0, dtype=np.int64), 0
    r = np.arange(n_rows, dtype=np.int64)
    cells = [r * L]
    docs = [D[np.searchsorted(U, a[:-1], "right") - 1]]
    ru = np.searchsorted(a, U, "right") - 1                      # the row whose slice holds each unit's start
    m = (ru < n_rows) & (U != a[np.minimum(ru, n_rows)])
    cells.append(ru[m] * L + U[m] - a[ru[m]])
    docs.append(D[m])
    fill = a[1:] - a[:-1]
    p = fill < L
    cells.append(r[p] * L + fill[p])
    docs.append(np.full(int(p.sum()), -1, dtype=np.int64))
    cells, docs = np.concatenate(cells), np.concatenate(docs)
    order = np.argsort(cells, kind="stable")
    cu = np.append(cells[order], n_rows * L).astype(np.int32)
    return cu, docs[order], int(np.diff(cu).max())


def row(S, unit_start, a, r, L, pad_id):
    """Row r's ids and positions from the stream S (numpy) and the non-empty units' starts."""
    U = np.asarray(unit_start, dtype=np.int64)
    s = np.arange(a[r], a[r + 1], dtype=np.int64)
    u0 = U[np.searchsorted(U, s, "right") - 1]
    n = len(s)
    ids = np.concatenate([S[a[r]:a[r + 1]], np.full(L - n, pad_id)]).astype(np.int32)
    pos = np.concatenate([s - np.maximum(u0, a[r]), np.arange(L - n)]).astype(np.int32)
    return ids, pos
