// jtk_decode_rows_rules.h -- decode of a matrix of token ids, row by row (jtk_batch_decode_rows*): the rule the device kernels
// (jtk_decode_rows.hip) and the CPU test shim tests/decode_rows_sim share.  Every row is one Encoding.decodeBytes(List<Integer>)
// (GptBytePairEncoding.java:137-151, 302-314) of the cells that the row's window, its stop ids and the pad id leave.
//
// The rule.  n_rows x width ids of 4 or 8 bytes, signed; row r starts at element r * row_stride.  For row r:
//   window  [b, e) = begin[r] / end[r] clamped into [0, width] (without the arrays: 0 and width); empty when e <= b.
//   stop    s = the first column in [b, e) whose id is one of the stop ids.  The row ends at e' = s, or at s + 1 with keep_stop;
//           without such a column e' = e.  A stop id left of b is not seen.  The stop test comes before the pad test: a pad
//           that is a stop id ends the row.
//   cells   cell c contributes the byte string of its id when b <= c < e' and not (skip_pad and id == pad_id).  A contributing
//           cell whose id has no entry (negative, at or above the table, a hole, any 64-bit value outside the table -- all 64
//           bits are compared, 2^32 + id is not id) contributes no bytes and makes the row JTK_ERR_UNKNOWN_TOKEN; a cell that
//           does not contribute never does.
//   output  the rows' bytes back to back; byte_off[r] = the position of row r's first byte, byte_off[n_rows] = the total;
//           cell_byte[r * width + c] = the position of the first byte of cell (r, c) -- for a cell without bytes, where the
//           next byte of the matrix goes.
//
// How it is computed: the first stop column per row (first[r], JTK_DR_NO_STOP without one; the kernels take a minimum over
// the row's hits, the shim walks the row), then the byte length of every cell of the flattened matrix t = r * width + c
// (jtk_dr_cell_len) and an exclusive scan of the lengths over t.
#ifndef JTK_DECODE_ROWS_RULES_H
#define JTK_DECODE_ROWS_RULES_H

#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define JTK_DR_HD __host__ __device__ inline
#else
#define JTK_DR_HD inline
#endif

#define JTK_DR_MAX_STOP 8                                   // == JTK_DECODE_MAX_STOP_IDS of the C ABI
#define JTK_DR_NO_STOP 0xFFFFFFFFFFFFFFFFull                // first[r] of a row without a stop column (all bytes 0xFF)

struct JtkDecodeRowsRule {
    int64_t pad_id;
    int64_t stop[JTK_DR_MAX_STOP];
    int32_t n_stop;
    bool skip_pad, keep_stop;
};

struct JtkDecodeRowsSpan { int64_t b, e; };                 // cells [b, e) of a row

JTK_DR_HD int64_t jtk_dr_clamp(int64_t v, int64_t width) { return v < 0 ? 0 : v > width ? width : v; }

// the window of row r (begin / end may be NULL)
JTK_DR_HD JtkDecodeRowsSpan jtk_dr_window(const int64_t* begin, const int64_t* end, int64_t r, int64_t width) {
    JtkDecodeRowsSpan w;
    w.b = begin ? jtk_dr_clamp(begin[r], width) : 0;
    w.e = end ? jtk_dr_clamp(end[r], width) : width;
    return w;
}

JTK_DR_HD bool jtk_dr_is_stop(const JtkDecodeRowsRule& rule, int64_t id) {
    for (int k = 0; k < rule.n_stop; k++)
        if (rule.stop[k] == id) return true;
    return false;
}

// [b, e') from the window and first = the first stop column inside it (JTK_DR_NO_STOP: none)
JTK_DR_HD JtkDecodeRowsSpan jtk_dr_cut(JtkDecodeRowsSpan w, uint64_t first, bool keep_stop) {
    if (first != JTK_DR_NO_STOP) w.e = (int64_t)first + (keep_stop ? 1 : 0);      // (b <= first < e, so e' <= e)
    return w;
}

// bytes of cell c of a row with the cells [b, e'), holding `id` (sign-extended to 64 bits when it is a 32-bit id);
// *unknown is set when the cell contributes and its id has no entry, left alone otherwise
JTK_DR_HD uint32_t jtk_dr_cell_len(const JtkDecodeRowsRule& rule, const uint32_t* tab_off, uint32_t n_ids_table, int64_t id,
                                   int64_t c, JtkDecodeRowsSpan row, bool* unknown) {
    if (c < row.b || c >= row.e) return 0;
    if (rule.skip_pad && id == rule.pad_id) return 0;
    const uint32_t l = ((uint64_t)id < (uint64_t)n_ids_table) ? tab_off[id + 1] - tab_off[id] : 0u;
    if (l == 0) *unknown = true;                                                   // GptBytePairEncoding.java:313
    return l;
}

#endif
