"""Plain restatement of the label rule of jtk_batch_token_spans / jtk_batch_pack_labels (jtokkit_amd/csrc/jtk_label_rules.h),
written from the rule text: token positions by a linear scan of token lengths, every span tried for every token, and the labels
read off the finished rows of pack_ref.pack by walking each document's unit through its segments."""
import numpy as np

import pack_ref

WHOLE, START, ANY = 0, 1, 2


def token_positions(doc_lens, doc_off):
    """doc_lens: per document the decoded byte length of each of its tokens.  Returns (p, q) int64 [n_tokens]."""
    p, q = [], []
    for d, lens in enumerate(doc_lens):
        pos = int(doc_off[d])
        for n in lens:
            p.append(pos)
            pos += int(n)
            q.append(pos)
    return np.array(p, dtype=np.int64), np.array(q, dtype=np.int64)


def token_spans(doc_lens, doc_off, spans, rule):
    """spans: [(begin, end)] in batch positions, sorted and disjoint.  tok_span int32 [n_tokens]: the lowest span for which the
    rule holds, or -1.  An empty span holds no token."""
    p, q = token_positions(doc_lens, doc_off)
    B = np.array([s[0] for s in spans], dtype=np.int64)
    E = np.array([s[1] for s in spans], dtype=np.int64)
    out = np.full(len(p), -1, dtype=np.int32)
    if not len(B):
        return out
    for t in range(len(p)):
        if rule == WHOLE:
            m = (B <= p[t]) & (q[t] <= E)
        elif rule == START:
            m = (B <= p[t]) & (p[t] < E)
        else:
            m = (p[t] < E) & (q[t] > B)
        m &= E > B
        if m.any():
            out[t] = int(np.argmax(m))
    return out


def labels(docs, status, L, sep_id=-1, sep_first=False, whole=False, drop_last=False, tok_span=None, ignore_index=-100,
           shift=False, label_sep=False, packed=None):
    """labels int32 [n_rows, L] for the rows of pack_ref.pack(docs, status, L, ...) (packed: that call's result, when the
    caller has it already).  tok_span: flat over the documents' tokens (in document order, refused documents included), or
    None: every token is trainable."""
    if packed is None:
        packed = pack_ref.pack(docs, status, L, sep_id, sep_first, whole, drop_last, pad_id=-1)
    rows, cu, seg_doc = packed["rows"], packed["cu_seqlens"], packed["seg_doc"]
    first = np.concatenate([[0], np.cumsum([len(d) for d in docs])]).astype(np.int64)
    unit_ids, unit_lab = {}, {}
    for d, ids in enumerate(docs):
        train = [True if tok_span is None else bool(tok_span[first[d] + i] >= 0) for i in range(len(ids))]
        lab = [t if ok else ignore_index for t, ok in zip(ids, train)]
        ids = list(ids)
        if sep_id >= 0 and sep_first:
            ids, lab = [sep_id] + ids, [ignore_index] + lab
        elif sep_id >= 0:
            stop = label_sep and (train[-1] if train else tok_span is None)
            ids, lab = ids + [sep_id], lab + [sep_id if stop else ignore_index]
        unit_ids[d], unit_lab[d] = ids, lab
    flat = np.full(rows.size, ignore_index, dtype=np.int32)
    used = {}
    for k, d in enumerate(seg_doc.tolist()):
        a, b = int(cu[k]), int(cu[k + 1])
        if d < 0:
            continue                                      # a pad run
        o = used.get(d, 0)                                # the unit goes on where its previous segment stopped
        assert unit_ids[d][o:o + b - a] == rows.reshape(-1)[a:b].tolist()
        seg = unit_lab[d][o:o + b - a]
        used[d] = o + b - a
        if shift:
            seg = seg[1:] + [ignore_index]
        flat[a:b] = seg
    return flat.reshape(rows.shape)
