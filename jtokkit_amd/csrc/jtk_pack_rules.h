// jtk_pack_rules.h -- packing of the last batch encode into fixed rows of L = seq_len tokens (jtk_batch_pack): the rule the
// device kernels (jtk_pack.hip) and the CPU test shim tests/pack_sim share.
//
// The rule.
//   Unit of document d: none when status[d] < 0 (it contributes nothing, not even a separator).  Otherwise its ids (those of
//   the last encode, whatever its flags) followed by sep_id (sep_id >= 0, EOS style), or sep_id followed by its ids
//   (JTK_PACK_SEP_FIRST, BOS style), or the ids alone (sep_id == -1).  A unit of length 0 is dropped.
//   concat (no JTK_PACK_WHOLE_DOCS): S = the units in document order; row r = S[rL, rL + L).  A partial last row is padded
//     with pad_id, or omitted with JTK_PACK_DROP_LAST: n_rows = ceil(|S| / L), or floor.  A unit that crosses a row boundary
//     goes on in the next row (in BOS style its separator appears once, at its start).
//   whole (JTK_PACK_WHOLE_DOCS): a unit of length l is cut into ceil(l / L) items of L tokens, the last holding the rest; the
//     items are placed in order by next-fit: an item goes into the current row if it fits in the cells left, else it starts a
//     new row.  Every row is padded with pad_id to L.  JTK_PACK_DROP_LAST with JTK_PACK_WHOLE_DOCS is an invalid argument.
//   Segments: a maximal run of cells of one row that hold tokens of one unit, or a maximal run of pad cells of one row; listed
//     in row-major order, they tile the n_rows * L cells.  cu_seqlens[0] = 0, cu_seqlens[k + 1] = cu_seqlens[k] + len(segment
//     k) (so cu_seqlens[n_seg] = n_rows * L: flash-attention's varlen layout of the rows flattened); seg_doc[k] = the document
//     of segment k, or -1 for pad; max_seqlen = the longest segment, 0 when there are no rows.
//   Positions: positions[r][c] = the offset of cell c in its segment: 0 at every document boundary and every row start; pad
//     runs count the same way.
//
// How it is computed (kernels in parallel, the shim serially), over documents d < n:
//   P      exclusive scan of the unit lengths l[d] (0 for documents without a unit); |S| = P[n].  The unit at stream position
//          s < |S| is the last d with P[d] <= s (jtk_pack_last_le): that d has P[d + 1] > s, so l[d] > 0.
//   concat row r = S[rL, min(rL + L, |S|)).
//   whole  A full item (L tokens) fits only an empty row and every row is opened by an item, so each full item fills a row of
//          its own: next-fit over items is next-fit over units, where unit h, opening a row, leaves tail(h) = (l_h - 1) mod L
//          + 1 cells of its last row used, and a later unit joins that row only whole.  The unit that opens the row after h is
//          nxt(h) = the first j > h with tail(h) + P[j + 1] - P[h + 1] > L (n if none; jtk_pack_next_head, a binary search
//          over P).  The heads are the chain h0 -> nxt(h0) -> ... from h0 = the first unit with l > 0 (the kernels find it by
//          binary lifting over the documents: 4 * ceil(log2(n + 1)) bytes of scratch per document, one launch per level).  Head h has ceil(l_h / L) rows and its last row also holds the units h + 1 .. nxt(h) - 1.  RS =
//          exclusive scan of those row counts over the heads (0 for the others); row RS[h] + j is S[P[h] + jL, P[h] + (j + 1)L)
//          for j < rows - 1, and S[P[h] + jL, P[nxt(h)]) for the last.
//   So in both modes row r is one slice S[a_r, b_r) with 0 < b_r - a_r <= L, then pad cells (jtk_pack_row).
//   SEG    exclusive scan of the segments per unit.  concat: the rows that the kept part [P[d], min(P[d + 1], n_rows L)) of
//          the unit touches, floor((end - 1) / L) - floor(begin / L) + 1.  whole: ceil(l / L) for a head, 1 for another unit,
//          plus 1 for the last unit of a group whose last row has pad (the pad segment follows it).  The segment of unit d
//          in row r is SEG[d] + r - firstrow(d), firstrow = floor(P[d] / L) (concat), RS[d] for a head and RS[d] - 1 for
//          another unit (whole).  The pad segment of a row: SEG[n] (concat: the last row only; n_seg = SEG[n] + 1 then), or
//          SEG[nxt(h)] - 1 (whole; n_seg = SEG[n]).
#ifndef JTK_PACK_RULES_H
#define JTK_PACK_RULES_H

#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define JTK_PK_HD __host__ __device__ inline
#else
#define JTK_PK_HD inline
#endif

#define JTK_PK_HEAD 1u        // flag bits per document (whole mode): the unit opens a row group ...
#define JTK_PK_PAD_AFTER 2u   // ... / a pad segment follows the unit (the last of a group whose last row has pad)

JTK_PK_HD int64_t jtk_pack_unit_len(int64_t n_ids, int32_t status, int32_t sep_id) {
    return status < 0 ? 0 : n_ids + (sep_id >= 0 ? 1 : 0);
}

// id at offset o (< unit length) of the unit of a document with ids[0 .. n_ids)
JTK_PK_HD int32_t jtk_pack_unit_id(const int32_t* ids, int64_t n_ids, int64_t o, int32_t sep_id, bool sep_first) {
    if (sep_id < 0) return ids[o];
    if (sep_first) return o == 0 ? sep_id : ids[o - 1];
    return o < n_ids ? ids[o] : sep_id;
}

JTK_PK_HD int64_t jtk_pack_concat_rows(int64_t S, int64_t L, bool drop_last) { return drop_last ? S / L : (S + L - 1) / L; }

// concat: segments of the unit [p, q) of S when the rows keep the cells [0, K)
JTK_PK_HD int64_t jtk_pack_concat_segs(int64_t p, int64_t q, int64_t L, int64_t K) {
    if (q > K) q = K;
    return q <= p ? 0 : (q - 1) / L - p / L + 1;
}

// concat: the longest of those segments (0 without one)
JTK_PK_HD int64_t jtk_pack_concat_max(int64_t p, int64_t q, int64_t L, int64_t K) {
    if (q > K) q = K;
    if (q <= p) return 0;
    const int64_t r0 = p / L, r1 = (q - 1) / L;
    if (r0 == r1) return q - p;
    if (r1 - r0 >= 2) return L;
    const int64_t a = (r0 + 1) * L - p, b = q - r1 * L;
    return a > b ? a : b;
}

// whole: cells of its last row that a unit of length l > 0 uses when it opens a row, and its rows then
JTK_PK_HD int64_t jtk_pack_tail(int64_t l, int64_t L) { return (l - 1) % L + 1; }
JTK_PK_HD int64_t jtk_pack_unit_rows(int64_t l, int64_t L) { return (l + L - 1) / L; }

// the last i in [lo, hi] with A[i] <= x (A non-decreasing, A[lo] <= x)
JTK_PK_HD int64_t jtk_pack_last_le(const int64_t* A, int64_t lo, int64_t hi, int64_t x) {
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo + 1) / 2;
        if (A[mid] <= x) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// the same for a cursor that moves forward: galloping from lo, O(log(answer - lo)) reads
JTK_PK_HD int64_t jtk_pack_seek(const int64_t* A, int64_t lo, int64_t hi, int64_t x) {
    int64_t step = 1;
    while (lo + step <= hi && A[lo + step] <= x) { lo += step; step *= 2; }
    return jtk_pack_last_le(A, lo, lo + step <= hi ? lo + step - 1 : hi, x);
}

// whole: nxt(h) for a unit h with l > 0; P has n + 1 entries
JTK_PK_HD int64_t jtk_pack_next_head(const int64_t* P, int64_t n, int64_t h, int64_t L) {
    const int64_t lim = P[h + 1] + L - jtk_pack_tail(P[h + 1] - P[h], L);   // j joins while P[j + 1] <= lim
    if (P[n] <= lim) return n;
    // the last m in [h + 1, n] with P[m] <= lim (P[h + 1] <= lim < P[n]) has P[m + 1] > lim: unit m is the first that does
    // not fit
    return jtk_pack_last_le(P, h + 1, n, lim);
}

// whole: pad cells of the last row of the group of head h (nx = nxt(h))
JTK_PK_HD int64_t jtk_pack_group_pad(const int64_t* P, int64_t h, int64_t nx, int64_t L) {
    return L - (jtk_pack_tail(P[h + 1] - P[h], L) + P[nx] - P[h + 1]);
}

// What the mapping of cells reads.  RS, flag and nxt are used in whole mode only.
struct JtkPackView {
    const int32_t* tokens;      // the last encode's ids
    const int64_t* tok_off;     // [n + 1]
    const int64_t* P;           // [n + 1]
    const int64_t* SEG;         // [n + 1]
    const int64_t* RS;          // [n + 1]
    const uint8_t* flag;        // [n]  JTK_PK_HEAD | JTK_PK_PAD_AFTER
    const int32_t* nxt;         // [n]  nxt(h) of every unit with l > 0
    int64_t n, L;
    int32_t sep_id;
    bool sep_first, whole;
};

struct JtkPackRow { int64_t a, b, seg_pad; };   // row r = S[a, b), then pad cells (segment seg_pad)

// Row r.  h: whole mode's cursor over the heads, moved forward to the head of row r (-1: none yet; the rows one caller asks
// for must not go backwards).
JTK_PK_HD JtkPackRow jtk_pack_row(const JtkPackView& v, int64_t r, int64_t& h) {
    JtkPackRow row;
    if (!v.whole) {
        row.a = r * v.L;
        row.b = row.a + v.L < v.P[v.n] ? row.a + v.L : v.P[v.n];
        row.seg_pad = v.SEG[v.n];
        return row;
    }
    h = h < 0 ? jtk_pack_last_le(v.RS, 0, v.n - 1, r) : jtk_pack_seek(v.RS, h, v.n - 1, r);
    const int64_t j = r - v.RS[h], k = jtk_pack_unit_rows(v.P[h + 1] - v.P[h], v.L), nx = v.nxt[h];
    row.a = v.P[h] + j * v.L;
    row.b = j < k - 1 ? row.a + v.L : v.P[nx];
    row.seg_pad = v.SEG[nx] - 1;
    return row;
}

// The unit under a cursor: document d (-1: none yet), its span [p0, p1) of S, seg0 = SEG[d] - firstrow(d), its ids.
struct JtkPackUnit { int64_t d, p0, p1, seg0, tb, n_ids; };

JTK_PK_HD void jtk_pack_load_unit(const JtkPackView& v, int64_t d, JtkPackUnit& u) {
    u.d = d; u.p0 = v.P[d]; u.p1 = v.P[d + 1];
    const int64_t first = !v.whole ? u.p0 / v.L : (v.flag[d] & JTK_PK_HEAD) ? v.RS[d] : v.RS[d] - 1;
    u.seg0 = v.SEG[d] - first;
    u.tb = v.tok_off[d]; u.n_ids = v.tok_off[d + 1] - u.tb;
}

struct JtkPackCell { int32_t id, pos; int64_t seg, doc; bool start; };   // doc -1: a pad cell

// Cell c of row r (jtk_pack_row).  u: the cursor, moved forward to the unit of the cell (the cells one caller asks for must
// not go backwards in S).
JTK_PK_HD JtkPackCell jtk_pack_cell(const JtkPackView& v, const JtkPackRow& row, int64_t r, int64_t c, int32_t pad_id,
                                    JtkPackUnit& u) {
    JtkPackCell out;
    const int64_t s = row.a + c;
    if (s < row.b) {
        if (u.d < 0) jtk_pack_load_unit(v, jtk_pack_last_le(v.P, 0, v.n - 1, s), u);
        else if (s >= u.p1) jtk_pack_load_unit(v, jtk_pack_seek(v.P, u.d + 1, v.n - 1, s), u);
        out.id = jtk_pack_unit_id(v.tokens + u.tb, u.n_ids, s - u.p0, v.sep_id, v.sep_first);
        out.pos = (int32_t)(s - (u.p0 > row.a ? u.p0 : row.a));
        out.seg = u.seg0 + r;
        out.doc = u.d;
    } else {
        out.id = pad_id;
        out.pos = (int32_t)(s - row.b);
        out.seg = row.seg_pad;
        out.doc = -1;
    }
    out.start = out.pos == 0;
    return out;
}

// The source token of cell c of row `row`, as an index into the last encode's ids, with u the cursor that jtk_pack_cell has
// just left on that cell: -1 for a separator and for a pad cell.
JTK_PK_HD int64_t jtk_pack_cell_token(const JtkPackView& v, const JtkPackRow& row, int64_t c, const JtkPackUnit& u) {
    const int64_t s = row.a + c;
    if (s >= row.b) return -1;
    const int64_t o = s - u.p0 - (v.sep_id >= 0 && v.sep_first ? 1 : 0);
    return o >= 0 && o < u.n_ids ? u.tb + o : -1;
}

#endif
