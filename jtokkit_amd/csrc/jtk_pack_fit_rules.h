// jtk_pack_fit_rules.h -- best-fit-decreasing packing of whole documents into rows of L = seq_len tokens
// (jtk_batch_pack_best_fit): the rule the device kernels (jtk_pack_fit.hip) and the CPU test shim tests/pack_fit_sim share.
//
// The rule.
//   Units: exactly those of jtk_batch_pack (jtk_pack_unit_len, jtk_pack_unit_id of jtk_pack_rules.h): a negative status
//     contributes no unit; the separator sits after the ids (EOS style), before them (JTK_PACK_SEP_FIRST) or is absent
//     (sep_id == -1); empty units are dropped.
//   Pieces: a unit of length l gives floor(l / L) full pieces of L cells and, if l mod L > 0, one rest of l mod L cells.
//   Full pieces: in document order, then piece order, each full piece is a row of its own: rows 0 .. F - 1.
//   Rests: taken in order of (length descending, document index ascending).  Each rest goes into the open row with free >= its
//     length and the smallest free; among equal free, into the row whose content changed longest ago (the smallest sequence
//     number of its last placed rest).  If no row fits it opens the next row: F, F + 1, ... in order of opening.  Inside a row
//     the pieces stand in order of placement, then pad.  A document has at most one rest, so two pieces of one document never
//     share a row.
//   Segments, positions, cu_seqlens, seg_doc and max_seqlen: as jtk_pack_rules.h defines them (maximal runs of one piece or of
//     pad inside a row, row-major).  n_rows = F + the rows opened.
//   The tie rule makes every class of rows with the same free a FIFO queue, and that is what lets a whole group of equal
//   rests be placed in one step (below) with the result of the one-at-a-time rule, bit for bit.  Ties by lowest row index
//   would need the queues merged in sorted order.
//
// How it is computed.
//   FR     exclusive scan of the full pieces per document: F = FR[n], row r < F is piece r - FR[d] of the last d with
//          FR[d] <= r.
//   order  the rests sorted stably by key L - rest (documents without a rest have key L: they sort last and are cut off): R
//          rests in sorted slots 0 .. R - 1, and per distinct length its first slot.
//   driver serial over the distinct lengths, longest first (jtk_fit_step).  State: per free value c in 1 .. L - 1 a FIFO queue
//          of runs; a run is a range of consecutively numbered rows with an identical history -- the same free, the same
//          number of pieces, the same columns -- {row_lo, count, pieces}.  Free L is an endless supply of fresh rows.  Runs
//          are only ever split, never merged, so every quantity of a placed rest is closed-form in its index inside the step.
//          A step takes length l with k rests left: c = the smallest non-empty class >= l (L if none).  The first rest goes
//          to the front row of the class's front run; that row then sits alone in class c - l, which was empty because
//          [l, c) was, so the next rest joins it, until the row holds per = floor(c / l) of them; it ends in class
//          c - per l < l, at the tail (its content changed last).  Then the run's next row takes its per rests.  So the step
//          takes min(k, count per) rests, gives the rows it filled to the tail of class c - per l as one run (when that
//          is > 0), a last partly filled row as a run of one to class c - j l, leaves the rest of the front run where it is, and
//          emits one record {first sorted slot, n, l, c, per, row_lo, pieces}: rest i of the step stands in row
//          row_lo + i / per at column L - c + (i % per) l as piece number pieces + i % per of that row.
//          A step places at least one rest: records <= R, runs <= 2 R.  Typical corpora need a few thousand steps per million
//          documents; the worst case (all rests distinct and longer than L / 2) is one step per document.
//   rows   every opened row lies in exactly one run at the end: its number of pieces and its fill L - free.  Two scans give a
//          row's first segment and a CSR of its pieces; the records are expanded into the CSR, one lane per rest, without
//          atomics.
//   cells  jtk_fit_row / jtk_fit_cell map a cell to its id, position and segment; the cursor they leave is a JtkPackUnit, so
//          jtk_label_cell of jtk_label_rules.h labels the cell unchanged.
// Row numbers inside the driver count from the first opened row (row F is 0): they stay below n whatever F is.
#ifndef JTK_PACK_FIT_RULES_H
#define JTK_PACK_FIT_RULES_H

#include "jtk_pack_rules.h"

#define JTK_FIT_MAX_LEN 262144                       // = JTK_PACK_FIT_MAX_LEN of jtokkit_amd.h: the class bitmap is 32 KiB
#define JTK_FIT_WORDS (JTK_FIT_MAX_LEN / 64)         // bitmap words of 64 classes
#define JTK_FIT_SUMS (JTK_FIT_WORDS / 64)            // summary words: bit j of sum[i] = bits[64 i + j] != 0

struct JtkFitRun { int32_t row_lo, count, pieces, next, free; };
struct JtkFitRec { int32_t slot, n, l, c, per, row_lo, pieces, unused; };

struct JtkFitState {
    uint64_t* bits;             // [JTK_FIT_WORDS]  class c is non-empty (LDS on the device); cleared up to L by the caller
    uint64_t* sum;              // [JTK_FIT_SUMS]
    int32_t* head;              // [L] front and back run of every non-empty class (not read for an empty one)
    int32_t* tail;
    JtkFitRun* runs;            // [2 R]
    JtkFitRec* recs;            // [R]
    int64_t L;
    int32_t n_runs, n_recs, next_row;
};

// the smallest non-empty class >= l (0 < l < L), or L
JTK_PK_HD int64_t jtk_fit_find(const JtkFitState& st, int64_t l) {
    int64_t w = l >> 6;
    const uint64_t m = st.bits[w] & (~0ull << (l & 63));
    if (m) return w * 64 + __builtin_ctzll(m);
    int64_t sw = w >> 6;
    const int64_t n_sum = ((st.L - 1) >> 12) + 1;                          // (classes end at L - 1 <= JTK_FIT_MAX_LEN - 1)
    uint64_t sm = (w & 63) == 63 ? 0ull : st.sum[sw] & (~0ull << ((w & 63) + 1));
    for (;;) {
        if (sm) {
            w = sw * 64 + __builtin_ctzll(sm);
            return w * 64 + __builtin_ctzll(st.bits[w]);
        }
        if (++sw >= n_sum) return st.L;
        sm = st.sum[sw];
    }
}

// run r to the tail of class c (0 < c < L)
JTK_PK_HD void jtk_fit_push(JtkFitState& st, int64_t c, int32_t r) {
    st.runs[r].next = -1;
    st.runs[r].free = (int32_t)c;
    const uint64_t bit = 1ull << (c & 63);
    if (st.bits[c >> 6] & bit) {
        st.runs[st.tail[c]].next = r;
    } else {
        st.head[c] = r;
        st.bits[c >> 6] |= bit;
        st.sum[c >> 12] |= 1ull << ((c >> 6) & 63);
    }
    st.tail[c] = r;
}

// the front run of the non-empty class c leaves it
JTK_PK_HD void jtk_fit_pop(JtkFitState& st, int64_t c) {
    const int32_t nx = st.runs[st.head[c]].next;
    if (nx >= 0) { st.head[c] = nx; return; }
    st.bits[c >> 6] &= ~(1ull << (c & 63));
    if (!st.bits[c >> 6]) st.sum[c >> 12] &= ~(1ull << ((c >> 6) & 63));
}

JTK_PK_HD void jtk_fit_new_run(JtkFitState& st, int64_t row_lo, int64_t count, int64_t pieces, int64_t free) {
    const int32_t r = st.n_runs++;
    JtkFitRun& run = st.runs[r];
    run.row_lo = (int32_t)row_lo; run.count = (int32_t)count; run.pieces = (int32_t)pieces; run.next = -1; run.free = (int32_t)free;
    if (free > 0) jtk_fit_push(st, free, r);
}

// One step: k > 0 rests of length l (0 < l < L) from sorted slot `slot` on.  Returns how many it placed (>= 1).
JTK_PK_HD int64_t jtk_fit_step(JtkFitState& st, int64_t l, int64_t slot, int64_t k) {
    const int64_t c = jtk_fit_find(st, l), per = c / l;
    const int32_t r = c < st.L ? st.head[c] : -1;
    const int64_t row_lo = r >= 0 ? st.runs[r].row_lo : st.next_row, pieces = r >= 0 ? st.runs[r].pieces : 0;
    int64_t n;
    if (r >= 0 && k >= (int64_t)st.runs[r].count * per) {                  // the whole run moves on
        n = (int64_t)st.runs[r].count * per;
        jtk_fit_pop(st, c);
        st.runs[r].pieces = (int32_t)(pieces + per);
        st.runs[r].free = (int32_t)(c - per * l);
        if (c - per * l > 0) jtk_fit_push(st, c - per * l, r);
    } else {                                                               // q rows filled, then one with j < per rests
        n = k;
        const int64_t q = k / per, j = k % per, used = q + (j > 0 ? 1 : 0);
        if (r >= 0) {
            st.runs[r].row_lo += (int32_t)used;
            st.runs[r].count -= (int32_t)used;
            if (st.runs[r].count == 0) jtk_fit_pop(st, c);
        } else {
            st.next_row += (int32_t)used;
        }
        if (q > 0) jtk_fit_new_run(st, row_lo, q, pieces + per, c - per * l);
        if (j > 0) jtk_fit_new_run(st, row_lo + q, 1, pieces + j, c - j * l);
    }
    JtkFitRec& rec = st.recs[st.n_recs++];
    rec.slot = (int32_t)slot; rec.n = (int32_t)n; rec.l = (int32_t)l; rec.c = (int32_t)c; rec.per = (int32_t)per;
    rec.row_lo = (int32_t)row_lo; rec.pieces = (int32_t)pieces; rec.unused = 0;
    return n;
}

// the record of sorted slot i: the last one with slot <= i (recs[0].slot == 0)
JTK_PK_HD int64_t jtk_fit_rec_of(const JtkFitRec* recs, int64_t n_recs, int64_t i) {
    int64_t lo = 0, hi = n_recs - 1;
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo + 1) / 2;
        if (recs[mid].slot <= i) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// What the mapping of cells reads.  Rows r >= F are numbered r - F in ITEM, SEGR and row_fill.
struct JtkFitView {
    const int32_t* tokens;      // the last encode's ids
    const int64_t* tok_off;     // [n + 1]
    const int64_t* FR;          // [n + 1] first full row of every document
    const int64_t* ITEM;        // [n + 1] the pieces of opened row i are items ITEM[i] .. ITEM[i + 1] - 1
    const int64_t* SEGR;        // [n + 1] F + SEGR[i] = the first segment of opened row i
    const int32_t* row_fill;    // [n]     cells of opened row i that hold pieces
    const int32_t* item_doc;    // [R]     document and first column of every piece of the opened rows
    const int32_t* item_col;
    int64_t n, L, F;
    int32_t sep_id;
    bool sep_first;
};

// Row r as jtk_label_cell wants it (a = 0, b = fill) with its items [io, io + np); np = 0: a row of one full piece
struct JtkFitRow { JtkPackRow row; int64_t io, np, seg0; };

JTK_PK_HD JtkFitRow jtk_fit_row(const JtkFitView& v, int64_t r) {
    JtkFitRow f;
    f.row.a = 0;
    if (r < v.F) {
        f.row.b = v.L; f.row.seg_pad = -1; f.io = 0; f.np = 0; f.seg0 = r;
    } else {
        const int64_t i = r - v.F;
        f.io = v.ITEM[i]; f.np = v.ITEM[i + 1] - f.io; f.seg0 = v.F + v.SEGR[i];
        f.row.b = v.row_fill[i]; f.row.seg_pad = f.seg0 + f.np;
    }
    return f;
}

// The piece under a cursor: u.p0 = the column at which the unit's offset 0 would stand (so c - u.p0 is the offset in the
// unit, as jtk_pack_cell_token reads it), u.p1 = the column after the piece, u.seg0 = its segment; rank -1: none yet.
struct JtkFitCursor { JtkPackUnit u; int64_t rank, col; };

JTK_PK_HD void jtk_fit_load(const JtkFitView& v, int64_t d, int64_t piece, int64_t col, int64_t end, int64_t seg, JtkFitCursor& k) {
    k.u.d = d; k.u.tb = v.tok_off[d]; k.u.n_ids = v.tok_off[d + 1] - k.u.tb;
    const int64_t full = piece >= 0 ? piece : (k.u.n_ids + (v.sep_id >= 0 ? 1 : 0)) / v.L;   // (the rest follows the full pieces)
    k.col = col; k.u.p0 = col - full * v.L; k.u.p1 = end; k.u.seg0 = seg;
}

// Cell c of row r (jtk_fit_row).  k: the cursor, rank -1 at the start of a row or of a lane; the cells one caller asks for in
// a row must not go backwards.
JTK_PK_HD JtkPackCell jtk_fit_cell(const JtkFitView& v, const JtkFitRow& f, int64_t r, int64_t c, int32_t pad_id, JtkFitCursor& k) {
    JtkPackCell out;
    if (c < f.row.b) {
        if (f.np == 0) {
            if (k.rank < 0) {
                const int64_t d = jtk_pack_last_le(v.FR, 0, v.n - 1, r);
                jtk_fit_load(v, d, r - v.FR[d], 0, v.L, r, k);
                k.rank = 0;
            }
        } else if (k.rank < 0 || c >= k.u.p1) {
            if (k.rank < 0) {
                int64_t lo = 0, hi = f.np - 1;                            // the last piece with col <= c
                while (lo < hi) {
                    const int64_t mid = lo + (hi - lo + 1) / 2;
                    if (v.item_col[f.io + mid] <= c) lo = mid; else hi = mid - 1;
                }
                k.rank = lo;
            } else {
                k.rank++;                                                 // (pieces are not empty and c moves by cells)
            }
            const int64_t i = f.io + k.rank;
            jtk_fit_load(v, v.item_doc[i], -1, v.item_col[i], k.rank + 1 < f.np ? (int64_t)v.item_col[i + 1] : f.row.b,
                         f.seg0 + k.rank, k);
        }
        out.id = jtk_pack_unit_id(v.tokens + k.u.tb, k.u.n_ids, c - k.u.p0, v.sep_id, v.sep_first);
        out.pos = (int32_t)(c - k.col);
        out.seg = k.u.seg0;
        out.doc = k.u.d;
    } else {
        out.id = pad_id;
        out.pos = (int32_t)(c - f.row.b);
        out.seg = f.row.seg_pad;
        out.doc = -1;
    }
    out.start = out.pos == 0;
    return out;
}

#endif
