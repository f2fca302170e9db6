// jtk_label_rules.h -- training labels for the packed rows of jtk_batch_pack from byte spans of the batch text
// (jtk_batch_token_spans, jtk_batch_pack_labels): the rule the device kernels (jtk_label.hip) and the CPU test shim
// tests/label_sim share.
//
// The rule.
//   Spans: [begin[i], end[i]) for i < n_spans, byte positions in the batch text (the coordinates of byte_begin / byte_end of
//     jtk_batch_chunk), sorted and disjoint: begin[i] <= end[i] <= begin[i + 1].
//   Token t occupies [p_t, q_t): p_t = doc_off[d] + the decoded bytes of the document's tokens before t (what
//     jtk_batch_token_offsets gives; a special token taken as an id counts its literal), q_t = p_t + its decoded length (> 0).
//   tok_span[t] = the lowest i for which the rule holds, or -1:
//     whole (0)   begin[i] <= p_t && q_t <= end[i]     no byte outside the span is ever trained on
//     start (1)   begin[i] <= p_t && p_t < end[i]      the usual offset-mapping rule
//     any   (2)   p_t < end[i] && q_t > begin[i], and the span is not empty
//   An empty span holds no token under any rule.  Membership goes by byte position alone: a span may cross documents.
//   Labels of the packed cells (on top of jtk_pack_cell, whose results do not change).  The unshifted label of a cell is
//     its id        when it holds token t of a document and tok_span[t] >= 0 (tok_span NULL: every token is trainable);
//     its id        when it is an EOS-style separator (sep_id >= 0, not JTK_PACK_SEP_FIRST), label_sep is asked for and the
//                   unit's last token is trainable (a unit without tokens: only when tok_span is NULL);
//     ignore_index  otherwise: BOS-style separators and pad cells always.
//   shift: cell (r, c) gets the unshifted label of cell (r, c + 1) when both lie in the same segment (the same row and the same
//     unit, or both pad: what cu_seqlens delimits), else ignore_index: next-token targets never cross a document boundary, a
//     row end, or into pad.
//
// How it is computed.  Tokens and spans are both ordered by position, so one cursor k = the last span with begin[k] <= p_t
// serves all three rules: the spans before k end at or before begin[k] <= p_t, the spans after k begin after p_t.  whole and
// start can only hold for k; any holds for k when end[k] > p_t, else for the first non-empty span after k that begins before
// q_t.  A lane finds k for its first token by binary search and then moves it forward by galloping (as jtk_pack_seek does).
// Every index the search reads lies in [0, n_spans) whatever the arrays hold, and a cursor that finds itself past p_t starts
// again, so spans that are not sorted give unspecified values of tok_span and never an access out of bounds.
#ifndef JTK_LABEL_RULES_H
#define JTK_LABEL_RULES_H

#include "jtk_pack_rules.h"

#define JTK_LB_WHOLE 0          // = JTK_SPAN_WHOLE, JTK_SPAN_START, JTK_SPAN_ANY of jtokkit_amd.h
#define JTK_LB_START 1
#define JTK_LB_ANY 2
#define JTK_LB_FRESH (-2)       // a span cursor that has not searched yet

// The cursor k moved to the last span with begin <= p (-1: none).  From JTK_LB_FRESH, or from a span that begins after p, a
// binary search over all spans (jtk_pack_last_le from lo = -1, its answer when there is none: begin[-1] is never read); else
// galloping forward from k.
JTK_PK_HD int64_t jtk_label_seek(const int64_t* begin, int64_t n, int64_t k, int64_t p) {
    if (k < -1 || k >= n || (k >= 0 && begin[k] > p)) return jtk_pack_last_le(begin, -1, n - 1, p);
    int64_t step = 1;
    while (k + step < n && begin[k + step] <= p) { k += step; step *= 2; }
    return jtk_pack_last_le(begin, k, k + step < n ? k + step - 1 : n - 1, p);
}

// tok_span of the token [p, q); k: the lane's cursor (JTK_LB_FRESH at first)
JTK_PK_HD int32_t jtk_label_tok_span(const int64_t* begin, const int64_t* end, int64_t n, int rule, int64_t p, int64_t q,
                                     int64_t& k) {
    if (n <= 0) return -1;
    k = jtk_label_seek(begin, n, k, p);
    if (rule == JTK_LB_WHOLE) return k >= 0 && q <= end[k] ? (int32_t)k : -1;
    if (rule == JTK_LB_START) return k >= 0 && p < end[k] ? (int32_t)k : -1;
    if (k >= 0 && p < end[k]) return (int32_t)k;
    for (int64_t i = k + 1; i < n && begin[i] < q; i++)        // (spans that begin inside the token: empty ones are passed over)
        if (end[i] > begin[i]) return (int32_t)i;
    return -1;
}

struct JtkLabelView {
    const int32_t* tok_span;    // [n_tokens] of the last encode, or NULL: every token is trainable
    int32_t ignore_index;
    bool label_sep;             // JTK_LABEL_SEP
};

JTK_PK_HD bool jtk_label_trainable(const JtkLabelView& lv, int64_t t) { return !lv.tok_span || lv.tok_span[t] >= 0; }

// The unshifted label of the cell that jtk_pack_cell(v, row, r, c, ., u) has just returned.
JTK_PK_HD int32_t jtk_label_cell(const JtkPackView& v, const JtkPackRow& row, int64_t c, const JtkPackCell& cell,
                                 const JtkPackUnit& u, const JtkLabelView& lv) {
    if (cell.doc < 0) return lv.ignore_index;
    const int64_t t = jtk_pack_cell_token(v, row, c, u);
    if (t >= 0) return jtk_label_trainable(lv, t) ? cell.id : lv.ignore_index;
    if (v.sep_first || !lv.label_sep) return lv.ignore_index;
    const bool last = u.n_ids > 0 ? jtk_label_trainable(lv, u.tb + u.n_ids - 1) : lv.tok_span == nullptr;
    return last ? cell.id : lv.ignore_index;
}

// shift: the label of a cell in column c of segment seg from the unshifted label and segment of the next cell of the row
// (next_label and next_seg are not looked at when c is the row's last column)
JTK_PK_HD int32_t jtk_label_shift(int64_t c, int64_t L, int64_t seg, int64_t next_seg, int32_t next_label, int32_t ignore_index) {
    return c + 1 < L && seg == next_seg ? next_label : ignore_index;
}

#endif
