// jtk_pack.hip -- packing of the last batch encode into rows of L tokens (jtk_batch_pack in jtk_abi.cpp), by the rule of
// jtk_pack_rules.h: concat (the units one after another, cut every L cells) or whole (next-fit of the units' items), with
// per-cell positions and flash-attention's varlen segments.
//
//   plan, both modes      pk_len          unit length per document -> P, then scan (jtk_launch_scan_i64)   |S| -> hdr[0]
//   plan, concat          pk_cat_count    rows touched by each unit (arithmetic on P), longest segment -> SEG, scan
//   plan, whole           pk_next         nxt(d) per unit (binary search over P) = up[0]; flag = HEAD at the first unit
//                         pk_lift x K-1   up[k][d] = up[k-1][up[k-1][d]]: the head 2^k groups on
//                         pk_mark x K     from k = K-1 down to 0 every head marks up[k][head]: after the K rounds the heads
//                                         h0, up^1(h0), ..., up^(2^K - 1)(h0) are marked, all of the chain (it has at most n
//                                         groups, 2^K > n).  A head newly marked in round k may or may not propagate in the
//                                         same round: its target up[k] is then one that round k marks anyway.
//                         pk_groups       per head: the pad of its group's last row, flag PAD_AFTER on the group's last unit
//                         pk_whole_count  rows per head -> RS, segments per unit -> SEG, longest segment; two scans
//   write                 pk_write        per block a contiguous span of cells, 4 per lane (one int4 store of ids and one of
//                                         positions); each lane keeps a cursor over the heads (whole) and one over the units
//                                         and moves it forward by galloping search (jtk_pack_row / jtk_pack_cell), so the
//                                         search costs ~1 read per step after the first; segment records by the lane that
//                                         holds a segment's first cell.
// Scratch per document: P, SEG, RS (8 B each), flag (1 B), and the lifting table, 4 * K bytes, K = ceil(log2(n + 1)).  Every
// round is a launch of its own: no data passes between workgroups inside one launch.
#include "jtk_device_prims.h"
#include "jtk_kernels.h"

namespace {

constexpr int PK_TILE = 1024;         // cells per workgroup step (256 lanes x 4)
constexpr int PK_MAX_BLOCKS = 4096;   // workgroups of the write; each takes a contiguous run of tiles

// max over the wave, one atomic per wave (all lanes must call it)
__device__ __forceinline__ void pk_max(int64_t* dst, int64_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const int64_t o = __shfl_xor(v, d);
        v = o > v ? o : v;
    }
    if ((threadIdx.x & 63) == 0 && v > 0) atomicMax((unsigned long long*)dst, (unsigned long long)v);
}

__global__ void __launch_bounds__(256) k_pk_len(JtkPackWork w) {
    const int64_t d = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= w.v.n) return;
    w.P[d] = jtk_pack_unit_len(w.v.tok_off[d + 1] - w.v.tok_off[d], w.status[d], w.v.sep_id);
}

__global__ void __launch_bounds__(256) k_pk_cat_count(JtkPackWork w) {
    const int64_t d = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t n = w.v.n, L = w.v.L;
    int64_t m = 0;
    if (d < n) {
        const int64_t K = jtk_pack_concat_rows(w.P[n], L, w.drop_last) * L;
        const int64_t p = w.P[d], q = w.P[d + 1];
        w.SEG[d] = jtk_pack_concat_segs(p, q, L, K);
        m = jtk_pack_concat_max(p, q, L, K);
    }
    pk_max(&w.hdr[3], m);
}

__global__ void __launch_bounds__(256) k_pk_next(JtkPackWork w) {
    const int64_t d = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t n = w.v.n;
    if (d > n) return;
    if (d == n) { w.up[n] = (int32_t)n; return; }
    const int64_t p = w.P[d], l = w.P[d + 1] - p;
    w.up[d] = (int32_t)(l > 0 ? jtk_pack_next_head(w.P, n, d, w.v.L) : n);
    w.flag[d] = (l > 0 && p == 0) ? (uint8_t)JTK_PK_HEAD : (uint8_t)0;
}

__global__ void __launch_bounds__(256) k_pk_lift(const int32_t* prev, int32_t* cur, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i <= n) cur[i] = prev[prev[i]];
}

__global__ void __launch_bounds__(256) k_pk_mark(const int32_t* upk, uint8_t* flag, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !(flag[i] & JTK_PK_HEAD)) return;
    const int64_t t = upk[i];
    if (t < n) flag[t] = (uint8_t)JTK_PK_HEAD;
}

// (flag[last] is written by the head of its group only, and read here by no other lane than that head's)
__global__ void __launch_bounds__(256) k_pk_groups(JtkPackWork w) {
    const int64_t d = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t n = w.v.n;
    int64_t pad = 0;
    if (d < n && (w.flag[d] & JTK_PK_HEAD)) {
        const int64_t nx = w.up[d];
        pad = jtk_pack_group_pad(w.P, d, nx, w.v.L);
        if (pad > 0) {
            const int64_t last = jtk_pack_last_le(w.P, d, nx - 1, w.P[nx] - 1);
            w.flag[last] = (uint8_t)(w.flag[last] | JTK_PK_PAD_AFTER);
        }
    }
    pk_max(&w.hdr[3], pad);
}

__global__ void __launch_bounds__(256) k_pk_whole_count(JtkPackWork w) {
    const int64_t d = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t n = w.v.n, L = w.v.L;
    int64_t m = 0;
    if (d < n) {
        const int64_t l = w.P[d + 1] - w.P[d];
        const uint32_t f = w.flag[d];
        const int64_t rows = (f & JTK_PK_HEAD) ? jtk_pack_unit_rows(l, L) : 0;
        w.RS[d] = rows;
        w.SEG[d] = (l > 0 ? ((f & JTK_PK_HEAD) ? rows : 1) : 0) + ((f & JTK_PK_PAD_AFTER) ? 1 : 0);
        m = l < L ? l : L;
    }
    pk_max(&w.hdr[3], m);
}

__global__ void __launch_bounds__(256) k_pk_write(JtkPackWork w, int32_t pad_id, int32_t* rows, int32_t* positions,
                                                  int32_t* cu_seqlens, int64_t* seg_doc, int64_t total, int64_t tiles_per_block) {
    const JtkPackView& v = w.v;
    const int64_t L = v.L;
    const int64_t n_tiles = (total + PK_TILE - 1) / PK_TILE;
    const int64_t t0 = (int64_t)blockIdx.x * tiles_per_block;
    const int64_t t1 = t0 + tiles_per_block < n_tiles ? t0 + tiles_per_block : n_tiles;
    if (blockIdx.x == 0 && threadIdx.x == 0 && cu_seqlens) cu_seqlens[w.n_seg] = (int32_t)total;
    int64_t h = -1;
    JtkPackUnit u;
    u.d = -1;
    for (int64_t t = t0; t < t1; t++) {
        const int64_t e0 = t * PK_TILE + threadIdx.x * 4;
        if (e0 >= total) break;
        int64_t r = e0 / L, c = e0 - r * L;
        JtkPackRow row = jtk_pack_row(v, r, h);
        int32_t id[4], pos[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            id[j] = pad_id; pos[j] = 0;
            if (e0 + j >= total) continue;
            if (c == L) { r++; c = 0; row = jtk_pack_row(v, r, h); }
            const JtkPackCell cell = jtk_pack_cell(v, row, r, c, pad_id, u);
            id[j] = cell.id; pos[j] = cell.pos;
            if (cell.start) {
                if (cu_seqlens) cu_seqlens[cell.seg] = (int32_t)(e0 + j);
                if (seg_doc) seg_doc[cell.seg] = cell.doc;
            }
            c++;
        }
        const bool full = e0 + 4 <= total;
        int32_t* dr = rows + e0;
        if (full && ((uintptr_t)dr & 15u) == 0) *reinterpret_cast<int4*>(dr) = make_int4(id[0], id[1], id[2], id[3]);
        else for (int j = 0; j < 4; j++) if (e0 + j < total) dr[j] = id[j];
        if (positions) {
            int32_t* dp = positions + e0;
            if (full && ((uintptr_t)dp & 15u) == 0) *reinterpret_cast<int4*>(dp) = make_int4(pos[0], pos[1], pos[2], pos[3]);
            else for (int j = 0; j < 4; j++) if (e0 + j < total) dp[j] = pos[j];
        }
    }
}

}  // namespace

void jtk_launch_pack_plan(const JtkPackWork& w, hipStream_t s) {
    const int64_t n = w.v.n;
    if (n > 0) hipLaunchKernelGGL(k_pk_len, dim3(jtk_blocks_for(n, 256)), dim3(256), 0, s, w);
    jtk_launch_scan_i64(w.P, n, &w.hdr[0], s);
    if (!w.v.whole) {
        if (n > 0) hipLaunchKernelGGL(k_pk_cat_count, dim3(jtk_blocks_for(n, 256)), dim3(256), 0, s, w);
        jtk_launch_scan_i64(w.SEG, n, &w.hdr[1], s);
        return;
    }
    const size_t stride = (size_t)n + 1;
    hipLaunchKernelGGL(k_pk_next, dim3(jtk_blocks_for(n + 1, 256)), dim3(256), 0, s, w);
    if (n > 0) {
        for (int k = 1; k < w.K; k++)
            hipLaunchKernelGGL(k_pk_lift, dim3(jtk_blocks_for(n + 1, 256)), dim3(256), 0, s, (const int32_t*)(w.up + (k - 1) * stride),
                               w.up + k * stride, n);
        for (int k = w.K - 1; k >= 0; k--)
            hipLaunchKernelGGL(k_pk_mark, dim3(jtk_blocks_for(n, 256)), dim3(256), 0, s, (const int32_t*)(w.up + k * stride), w.flag, n);
        hipLaunchKernelGGL(k_pk_groups, dim3(jtk_blocks_for(n, 256)), dim3(256), 0, s, w);
        hipLaunchKernelGGL(k_pk_whole_count, dim3(jtk_blocks_for(n, 256)), dim3(256), 0, s, w);
    }
    jtk_launch_scan_i64(w.RS, n, &w.hdr[2], s);
    jtk_launch_scan_i64(w.SEG, n, &w.hdr[1], s);
}

void jtk_launch_pack_write(const JtkPackWork& w, int32_t pad_id, int32_t* rows, int32_t* positions, int32_t* cu_seqlens,
                           int64_t* seg_doc, hipStream_t s) {
    const int64_t total = w.n_rows * w.v.L;
    if (total <= 0) {
        if (cu_seqlens) (void)hipMemsetAsync(cu_seqlens, 0, 4, s);
        return;
    }
    const int64_t n_tiles = (total + PK_TILE - 1) / PK_TILE;
    const int64_t blocks = n_tiles < PK_MAX_BLOCKS ? n_tiles : PK_MAX_BLOCKS;
    const int64_t per = (n_tiles + blocks - 1) / blocks;
    hipLaunchKernelGGL(k_pk_write, dim3((unsigned)((n_tiles + per - 1) / per)), dim3(256), 0, s, w, pad_id, rows, positions,
                       cu_seqlens, seg_doc, total, per);
}
