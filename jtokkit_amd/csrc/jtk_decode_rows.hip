// jtk_decode_rows.hip -- decode of a matrix of token ids, row by row: Encoding.decodeBytes(List<Integer>)
// (GptBytePairEncoding.java:137-151, 302-314) of the cells that every row's window, stop ids and pad id leave.  The rule is
// jtk_decode_rows_rules.h.  The matrix is walked as flattened cells t = r * width + c in tiles of 2048 cells, 8 consecutive
// cells per lane, like the token stream of jtk_decode.hip; a lane finds its row and column once and steps them along.
//
//   dr_row_end   (only with stop ids) first stop column inside every row's window: a minimum over the row's hits, taken by
//                the first cell of every run of hits only -- the EOS fill behind the first EOS is one run, one atomic
//   dr_count     bytes per tile (lengths from the offset table); unknown ids -> status of their row, by index
//   scan         exclusive scan of the tile sizes (jtk_launch_scan_u32)
//   dr_scatter   per tile: byte offset of every cell (block scan) -> cell_byte, byte_off at column 0; the tile's bytes
//                assembled in LDS and written in aligned 4-byte words, or straight to global memory when they do not fit
// Integer / byte gather work, as the flat decode: bound by the random reads of the token byte strings (L2-resident blob).
#include "jtk_decode_rows_rules.h"
#include "jtk_device_prims.h"
#include "jtk_kernels.h"

namespace {

constexpr int DT = JTK_DEC_TILE;           // cells per tile
constexpr int DSTAGE = 16384;              // bytes of a tile assembled in LDS

// Row and column of a lane's cells, stepped along the flattened matrix; the row's cells [b, e') are loaded when the row changes.
struct RowCursor {
    int64_t r, c;
    JtkDecodeRowsSpan span;
    __device__ __forceinline__ void load(const JtkDecodeRowsWork& w) {
        span = jtk_dr_window(w.begin, w.end, r, w.width);
        if (w.first_stop) span = jtk_dr_cut(span, w.first_stop[r], w.rule.keep_stop);
    }
    __device__ __forceinline__ void start(const JtkDecodeRowsWork& w, int64_t t) {     // t < n_cells (so width > 0)
        r = t / w.width;
        c = t - r * w.width;
        load(w);
    }
    __device__ __forceinline__ void step(const JtkDecodeRowsWork& w, int64_t t_next) {
        if (++c == w.width) {
            c = 0; r++;
            if (t_next < w.n_cells) load(w);
        }
    }
};

// the byte lengths of the lane's 8 cells t0 .. t0 + 7 (0 past n_cells), their ids, and the sum of the lengths.  flag: unknown
// ids are reported to their rows (one atomic per lane and row).  col0: bit j set when cell j is column 0 of a row.
template <class IdT>
__device__ __forceinline__ uint32_t lane_cells(const JtkDecodeRowsWork& w, int64_t t0, bool flag, uint32_t (&len)[8], int64_t (&id)[8],
                                               int64_t* row0, uint32_t* col0) {
    const IdT* rows = (const IdT*)w.rows;
    uint32_t sum = 0, c0 = 0;
    RowCursor cur;
    cur.r = 0; cur.c = 0; cur.span.b = cur.span.e = 0;
    if (t0 < w.n_cells) cur.start(w, t0);
    *row0 = cur.r;
    int64_t flagged = -1;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const int64_t t = t0 + j;
        len[j] = 0; id[j] = -1;
        if (t < w.n_cells) {
            id[j] = (int64_t)rows[cur.r * w.row_stride + cur.c];                     // all 64 bits of a 64-bit id
            bool unknown = false;
            len[j] = jtk_dr_cell_len(w.rule, w.tab_off, w.n_ids_table, id[j], cur.c, cur.span, &unknown);
            if (unknown && flag && flagged != cur.r) { atomicMin(&w.status[cur.r], -3 /* JTK_ERR_UNKNOWN_TOKEN */); flagged = cur.r; }
            if (cur.c == 0) c0 |= 1u << j;
            sum += len[j];
            cur.step(w, t + 1);
        }
    }
    if (col0) *col0 = c0;
    return sum;
}

template <class IdT>
__global__ void __launch_bounds__(256) k_dr_row_end(JtkDecodeRowsWork w) {
    const IdT* rows = (const IdT*)w.rows;
    const int64_t t0 = (int64_t)blockIdx.x * DT + threadIdx.x * 8;
    if (t0 >= w.n_cells) return;
    int64_t r = t0 / w.width, c = t0 - r * w.width;
    JtkDecodeRowsSpan win = jtk_dr_window(w.begin, w.end, r, w.width);
    // was the cell before the lane's first a hit of the same row?  (the cell left of b is outside the window: no hit)
    bool prev = c > win.b && c - 1 < win.e && jtk_dr_is_stop(w.rule, (int64_t)rows[r * w.row_stride + c - 1]);
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const int64_t t = t0 + j;
        if (t < w.n_cells) {
            const bool hit = c >= win.b && c < win.e && jtk_dr_is_stop(w.rule, (int64_t)rows[r * w.row_stride + c]);
            if (hit && !prev) atomicMin(&w.first_stop[r], (unsigned long long)c);
            prev = hit;
            if (++c == w.width) {
                c = 0; r++; prev = false;
                if (t + 1 < w.n_cells) win = jtk_dr_window(w.begin, w.end, r, w.width);
            }
        }
    }
}

template <class IdT>
__global__ void __launch_bounds__(256) k_dr_count(JtkDecodeRowsWork w) {
    const int64_t t0 = (int64_t)blockIdx.x * DT + threadIdx.x * 8;
    uint32_t len[8];
    int64_t id[8], row0;
    const uint32_t sum = lane_cells<IdT>(w, t0, true, len, id, &row0, nullptr);
    uint32_t total;
    (void)jtk_block_excl_prefix<256>(sum, &total);
    if (threadIdx.x == 0) w.tile_bytes[blockIdx.x] = total;
}

template <class IdT>
__global__ void __launch_bounds__(256) k_dr_scatter(JtkDecodeRowsWork w) {
    __shared__ __attribute__((aligned(16))) uint8_t s_out[DSTAGE + 8];
    const int tid = threadIdx.x;
    const int64_t tile = blockIdx.x;
    const int64_t t0 = tile * DT + tid * 8;
    const int64_t obase = w.tile_off[tile];
    const uint32_t total = w.tile_bytes[tile];
    const bool stage = total <= (uint32_t)DSTAGE;
    uint32_t len[8], col0;
    int64_t id[8], row;
    const uint32_t sum = lane_cells<IdT>(w, t0, false, len, id, &row, &col0);
    uint32_t pre = jtk_block_excl_prefix<256>(sum);
    if (tile == 0 && tid == 0) w.byte_off[w.n_rows] = w.tile_off[w.n_tiles];
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const int64_t t = t0 + j;
        if (t < w.n_cells) {
            if (w.cell_byte) w.cell_byte[t] = obase + pre;
            if ((col0 >> j) & 1u) { if (j > 0) row++; w.byte_off[row] = obase + pre; }     // (the row changes at column 0 only)
        }
        if (len[j]) {
            const uint8_t* src = w.tab_blob + w.tab_off[id[j]];
            if (stage) for (uint32_t i = 0; i < len[j]; i++) s_out[pre + i] = src[i];
            else for (uint32_t i = 0; i < len[j]; i++) w.out[obase + pre + i] = src[i];
        }
        pre += len[j];
    }
    if (!stage) return;
    __syncthreads();
    // aligned 4-byte words of the output that the tile's bytes [obase, obase + total) touch (as k_dec_scatter writes them)
    const int64_t a0 = obase & ~(int64_t)3, a1 = (obase + total + 3) & ~(int64_t)3;
    for (int64_t g = a0 + (int64_t)tid * 4; g < a1; g += 1024) {
        const int64_t rel = g - obase;                                 // may be -3..-1 for the first word
        if (rel >= 0 && rel + 4 <= (int64_t)total) {
            const uint32_t v = (uint32_t)s_out[rel] | ((uint32_t)s_out[rel + 1] << 8) | ((uint32_t)s_out[rel + 2] << 16) | ((uint32_t)s_out[rel + 3] << 24);
            *reinterpret_cast<uint32_t*>(w.out + g) = v;
        } else {
            for (int k = 0; k < 4; k++) { const int64_t r = rel + k; if (r >= 0 && r < (int64_t)total) w.out[g + k] = s_out[r]; }
        }
    }
}

}  // namespace

void jtk_launch_decode_rows_count(const JtkDecodeRowsWork& w, hipStream_t s) {
    const dim3 grid((unsigned)w.n_tiles), block(256);
    if (w.id_bytes == 8) {
        if (w.first_stop) hipLaunchKernelGGL(k_dr_row_end<int64_t>, grid, block, 0, s, w);
        hipLaunchKernelGGL(k_dr_count<int64_t>, grid, block, 0, s, w);
    } else {
        if (w.first_stop) hipLaunchKernelGGL(k_dr_row_end<int32_t>, grid, block, 0, s, w);
        hipLaunchKernelGGL(k_dr_count<int32_t>, grid, block, 0, s, w);
    }
    jtk_launch_scan_u32(w.tile_bytes, w.n_tiles, w.tile_off, w.total, s);
}
void jtk_launch_decode_rows_scatter(const JtkDecodeRowsWork& w, hipStream_t s) {
    const dim3 grid((unsigned)w.n_tiles), block(256);
    if (w.id_bytes == 8) hipLaunchKernelGGL(k_dr_scatter<int64_t>, grid, block, 0, s, w);
    else hipLaunchKernelGGL(k_dr_scatter<int32_t>, grid, block, 0, s, w);
}
