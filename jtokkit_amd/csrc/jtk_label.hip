// jtk_label.hip -- training labels of the packed rows from byte spans of the batch text (jtk_batch_token_spans and
// jtk_batch_pack_labels in jtk_abi.cpp), by the rule of jtk_label_rules.h.
//
//   lb_spans   per tile of 2048 tokens, 8 tokens per lane: the walk of k_ck_tokpos (jtk_tile_tok_prefix, tile_off and
//              dbase of the chunk work's byte scan), but the positions stay in registers: each lane finds the span cursor of
//              its first token by one binary search over begin[], moves it forward by galloping for the other seven, and
//              writes int32 tok_span -- 4 bytes per token, no [n_tokens] int64 array in between.
//   lb_pack    the cell walk of k_pk_write, 4 cells per lane and one int4 store: the label of every cell from tok_span of the
//              cell's source token (jtk_pack_cell_token).  With shift a lane also maps the cell after its fourth, in the same
//              lane (the lane after it may belong to another tile run, and a row's last cell needs no lookup), and hands every
//              cell the label of its right neighbour within the segment.
// Neither kernel shuffles inside a divergent expression: the tile prefix of lb_spans runs before any lane leaves.
#include "jtk_device_prims.h"
#include "jtk_kernels.h"

namespace {

constexpr int CT = JTK_DEC_TILE;      // tokens per tile of the byte scan
constexpr int LB_TILE = 1024;         // cells per workgroup step (256 lanes x 4)
constexpr int LB_MAX_BLOCKS = 4096;   // workgroups of lb_pack; each takes a contiguous run of tiles
static_assert(CT == 256 * 8, "a tile is 256 lanes x 8 tokens");

// the document that holds token t: the last d in [0, n_docs) with tok_off[d] <= t (as ck_doc_of of jtk_chunk.hip)
__device__ __forceinline__ int64_t lb_doc_of(const JtkChunkWork& w, int64_t t) {
    return jtk_first_gt(w.tok_off, 1, w.n_docs, t) - 1;
}

__global__ void __launch_bounds__(256) k_lb_spans(JtkChunkWork w, const int64_t* begin, const int64_t* end, int64_t n_spans,
                                                  int rule, int32_t* tok_span) {
    const int64_t t0 = (int64_t)blockIdx.x * CT + threadIdx.x * 8;
    uint32_t len[8];
    const uint32_t pre = jtk_tile_tok_prefix(w.tokens, w.n_tok, t0, w.tab_off, w.n_ids_table, 1u, len);
    if (t0 >= w.n_tok) return;                                            // (behind the prefix: it holds a barrier)
    int64_t pos = w.tile_off[blockIdx.x] + pre;
    int64_t d = lb_doc_of(w, t0);
    int64_t cur = JTK_LB_FRESH;
    int32_t out[8];
#pragma unroll
    for (int j = 0; j < 8; j++) {
        out[j] = -1;
        const int64_t t = t0 + j;
        if (t >= w.n_tok) continue;
        if (w.tok_off[d + 1] <= t) d = lb_doc_of(w, t);
        const int64_t p = w.dbase[d] + pos;
        out[j] = jtk_label_tok_span(begin, end, n_spans, rule, p, p + len[j], cur);
        pos += len[j];
    }
    int32_t* dst = tok_span + t0;                                         // (t0 is a multiple of 8)
    if (t0 + 8 <= w.n_tok && ((uintptr_t)dst & 15u) == 0) {
        reinterpret_cast<int4*>(dst)[0] = make_int4(out[0], out[1], out[2], out[3]);
        reinterpret_cast<int4*>(dst)[1] = make_int4(out[4], out[5], out[6], out[7]);
    } else {
        for (int j = 0; j < 8; j++) if (t0 + j < w.n_tok) dst[j] = out[j];
    }
}

template <bool SHIFT>
__global__ void __launch_bounds__(256) k_lb_pack(JtkPackWork w, JtkLabelView lv, int32_t* labels, int64_t total,
                                                 int64_t tiles_per_block) {
    const JtkPackView& v = w.v;
    const int64_t L = v.L;
    constexpr int NC = SHIFT ? 5 : 4;                                     // cells a lane maps: its four, and the one after
    const int64_t n_tiles = (total + LB_TILE - 1) / LB_TILE;
    const int64_t t0 = (int64_t)blockIdx.x * tiles_per_block;
    const int64_t t1 = t0 + tiles_per_block < n_tiles ? t0 + tiles_per_block : n_tiles;
    int64_t h = -1;
    JtkPackUnit u;
    u.d = -1;
    for (int64_t t = t0; t < t1; t++) {
        const int64_t e0 = t * LB_TILE + threadIdx.x * 4;
        if (e0 >= total) break;
        int64_t r = e0 / L, c = e0 - r * L;
        JtkPackRow row = jtk_pack_row(v, r, h);
        int32_t lab[NC];
        int64_t seg[NC], col[NC];
#pragma unroll
        for (int j = 0; j < NC; j++) {
            lab[j] = lv.ignore_index; seg[j] = -1; col[j] = c;
            // (the fifth cell is looked at only when it continues the fourth's row: c == L there means a row end, and so does
            // the end of the rows, total = n_rows * L)
            if (e0 + j >= total || (j == 4 && c == L)) continue;
            if (c == L) { r++; c = 0; col[j] = 0; row = jtk_pack_row(v, r, h); }
            const JtkPackCell cell = jtk_pack_cell(v, row, r, c, 0, u);
            lab[j] = jtk_label_cell(v, row, c, cell, u, lv);
            seg[j] = cell.seg;
            c++;
        }
        int32_t o[4];
#pragma unroll
        for (int j = 0; j < 4; j++)
            o[j] = SHIFT ? jtk_label_shift(col[j], L, seg[j], seg[j + NC - 4], lab[j + NC - 4], lv.ignore_index) : lab[j];
        int32_t* dl = labels + e0;
        if (e0 + 4 <= total && ((uintptr_t)dl & 15u) == 0) *reinterpret_cast<int4*>(dl) = make_int4(o[0], o[1], o[2], o[3]);
        else for (int j = 0; j < 4; j++) if (e0 + j < total) dl[j] = o[j];
    }
}

}  // namespace

void jtk_launch_label_spans(const JtkChunkWork& w, const int64_t* begin, const int64_t* end, int64_t n_spans, int rule,
                            int32_t* tok_span, hipStream_t s) {
    if (w.n_tok > 0) hipLaunchKernelGGL(k_lb_spans, dim3((unsigned)w.n_tiles), dim3(256), 0, s, w, begin, end, n_spans, rule, tok_span);
}

void jtk_launch_label_pack(const JtkPackWork& w, const JtkLabelView& lv, bool shift, int32_t* labels, hipStream_t s) {
    const int64_t total = w.n_rows * w.v.L;
    if (total <= 0) return;
    const int64_t n_tiles = (total + LB_TILE - 1) / LB_TILE;
    const int64_t blocks = n_tiles < LB_MAX_BLOCKS ? n_tiles : LB_MAX_BLOCKS;
    const int64_t per = (n_tiles + blocks - 1) / blocks;
    const dim3 grid((unsigned)((n_tiles + per - 1) / per));
    if (shift) hipLaunchKernelGGL(k_lb_pack<true>, grid, dim3(256), 0, s, w, lv, labels, total, per);
    else hipLaunchKernelGGL(k_lb_pack<false>, grid, dim3(256), 0, s, w, lv, labels, total, per);
}
