// jtk_device_prims.h -- the one home of the small primitives that every post-pass (decode, maxTokens, chunks, allow-special,
// pack, labels) is built on: offset search, token byte length, wave scan / sum, the exclusive prefix of a lane inside its
// workgroup, the token-length prefix of a tile, the one-workgroup array scan, and the grid size of a one-lane-per-item launch.
// The searches and the token length also compile on the host (tests/prims_sim).
//
// Two rules hold for every caller:
//   shuffles   jtk_wave_incl_scan / jtk_wave_sum are called by all 64 lanes, outside any condition;
//   barriers   jtk_block_excl_prefix, jtk_tile_tok_prefix and jtk_block_scan_array contain __syncthreads(): every thread of
//              the workgroup calls them, before any early return.
#ifndef JTK_DEVICE_PRIMS_H
#define JTK_DEVICE_PRIMS_H

#include "jtk_common.h"

// ---- search over a non-decreasing array.  The caller states at the call site what the index means and how it is clamped.
// the first k in [lo, hi) with a[k] > x; hi when there is none
JTK_HD int64_t jtk_first_gt(const int64_t* a, int64_t lo_, int64_t hi_, int64_t x) {
    int64_t hi = hi_, lo = lo_;                  // (declared in this order, find_doc's loop in the hot kernels compiles as it always did)
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (a[mid] > x) hi = mid; else lo = mid + 1;
    }
    return lo;
}
// the first k in [lo, hi) with a[k] >= x; hi when there is none
JTK_HD int64_t jtk_first_ge(const int64_t* a, int64_t lo_, int64_t hi_, int64_t x) {
    int64_t hi = hi_, lo = lo_;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (a[mid] >= x) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// ---- byte length of token id by the decode table's offsets.  An id outside the table (negative ones too) has length
// `unknown`: 1 in the post-passes of an encode (the pseudo ids of bytes a rank map lacks: one byte each; their documents are
// refused), 0 in decode (the id is reported).
JTK_HD uint32_t jtk_tok_len(const uint32_t* tab_off, uint32_t n_ids_table, int32_t id, uint32_t unknown) {
    return ((uint32_t)id < n_ids_table) ? tab_off[id + 1] - tab_off[id] : unknown;
}

// ---- blocks of `per` items that cover n items, at least 1: a launch over nothing is one idle workgroup (every kernel
// launched this way checks its index against n), never the zero-sized grid that the runtime refuses.
inline unsigned jtk_blocks_for(int64_t n, int per) { return (unsigned)((n + per - 1) / per > 0 ? (n + per - 1) / per : 1); }

#if defined(__HIPCC__)

// ---- inclusive prefix sum across the wave
__device__ __forceinline__ uint32_t jtk_wave_incl_scan(uint32_t v) {
    const unsigned lane = threadIdx.x & 63u;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = (uint32_t)__shfl_up((int)v, d);
        if (lane >= (unsigned)d) v += o;
    }
    return v;
}
__device__ __forceinline__ uint64_t jtk_wave_incl_scan(uint64_t v) {
    const unsigned lane = threadIdx.x & 63u;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t o = __shfl_up(v, d);
        if (lane >= (unsigned)d) v += o;
    }
    return v;
}

// ---- inclusive prefix sum over lanes 0..31 of the wave, for values that only those lanes hold (what lanes 32..63 return is
// not a prefix of anything).  In registers: four shifts inside each row of 16 lanes (a lane without a source adds 0), then
// lane 15's sum into row 1 -- no LDS round trip, where the 64-lane scan above makes six.  Called by all 64 lanes.
__device__ __forceinline__ uint32_t jtk_wave_incl_scan32(uint32_t v) {
    constexpr int ROW_SHR = 0x110, ROW_BCAST15 = 0x142;
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, ROW_SHR + 1, 0xF, 0xF, true);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, ROW_SHR + 2, 0xF, 0xF, true);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, ROW_SHR + 4, 0xF, 0xF, true);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, ROW_SHR + 8, 0xF, 0xF, true);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, ROW_BCAST15, 0xA, 0xF, false);   // rows 1 and 3 only
    return v;
}

// ---- sum over the wave; every lane ends with it
__device__ __forceinline__ uint32_t jtk_wave_sum(uint32_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += (uint32_t)__shfl_xor((int)v, d);
    return v;
}
__device__ __forceinline__ uint64_t jtk_wave_sum(uint64_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}
__device__ __forceinline__ int64_t jtk_wave_sum(int64_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

// ---- the sum of v over the lower threads of the workgroup (THREADS threads, whole waves); *total (may be NULL): over all.
// CONTAINS A BARRIER: every thread of the workgroup calls it, before any early return; and its LDS words are one set per
// kernel, so a second call in the same kernel needs a barrier of the caller's in between.
template <int THREADS>
__device__ __forceinline__ uint32_t jtk_block_excl_prefix(uint32_t v, uint32_t* total = nullptr) {
    __shared__ uint32_t s_wsum[THREADS / 64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint32_t inc = jtk_wave_incl_scan(v);
    if (lane == 63) s_wsum[wv] = inc;
    __syncthreads();
    uint32_t pre = inc - v;
    for (int k = 0; k < wv; k++) pre += s_wsum[k];
    if (total) {
        uint32_t t = 0;
#pragma unroll
        for (int k = 0; k < THREADS / 64; k++) t += s_wsum[k];
        *total = t;
    }
    return pre;
}
// the same for a (count, bytes) pair in one pass: one barrier for both
template <int THREADS>
__device__ __forceinline__ void jtk_block_excl_prefix(uint32_t c, int64_t b, uint32_t* c_pre, int64_t* b_pre) {
    __shared__ uint32_t s_csum[THREADS / 64];
    __shared__ int64_t s_bsum[THREADS / 64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint32_t ci = jtk_wave_incl_scan(c);
    const int64_t bi = (int64_t)jtk_wave_incl_scan((uint64_t)b);
    if (lane == 63) { s_csum[wv] = ci; s_bsum[wv] = bi; }
    __syncthreads();
    uint32_t cp = ci - c;
    int64_t bp = bi - b;
    for (int k = 0; k < wv; k++) { cp += s_csum[k]; bp += s_bsum[k]; }
    *c_pre = cp;
    *b_pre = bp;
}

// ---- a tile of 2048 tokens, 256 lanes x 8: the byte lengths len[8] of the lane's tokens t0 .. t0 + 7 (0 past n_tok) and the
// bytes of the tile's tokens before t0; *tile_bytes (may be NULL) = the tile's bytes, id (may be NULL) = the lane's 8 ids.
// CONTAINS A BARRIER (jtk_block_excl_prefix<256>).
__device__ __forceinline__ uint32_t jtk_tile_tok_prefix(const int32_t* tokens, int64_t n_tok, int64_t t0, const uint32_t* tab_off,
                                                        uint32_t n_ids_table, uint32_t unknown, uint32_t (&len)[8],
                                                        uint32_t* tile_bytes = nullptr, int32_t* id = nullptr) {
    uint32_t sum = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const int32_t tk = (t0 + j < n_tok) ? tokens[t0 + j] : -1;
        if (id) id[j] = tk;
        len[j] = (t0 + j < n_tok) ? jtk_tok_len(tab_off, n_ids_table, tk, unknown) : 0u;
        sum += len[j];
    }
    return jtk_block_excl_prefix<256>(sum, tile_bytes);
}

// ---- exclusive scan of load(0 .. n - 1) by ONE workgroup of 1024 threads, 16 items per thread and step: store(i, the sum of
// the items before i) for every i < n; returns the sum of all to every thread.  Sums are 64-bit.
// CONTAINS BARRIERS: all 1024 threads call it; it may be called again in the same kernel.
template <class Load, class Store>
__device__ __forceinline__ uint64_t jtk_block_scan_array(int64_t n, Load load, Store store) {
    constexpr int PER = 16;
    __shared__ uint64_t s_wsum[16];
    __shared__ uint64_t s_base;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    __syncthreads();                                                      // (an earlier call's total has been read)
    if (tid == 0) s_base = 0;
    __syncthreads();
    for (int64_t c0 = 0; c0 < n; c0 += 1024 * PER) {
        const int64_t i0 = c0 + (int64_t)tid * PER;
        uint64_t v[PER];
        uint64_t sum = 0;
#pragma unroll
        for (int j = 0; j < PER; j++) { v[j] = (i0 + j < n) ? (uint64_t)load(i0 + j) : 0u; sum += v[j]; }
        const uint64_t inc = jtk_wave_incl_scan(sum);
        if (lane == 63) s_wsum[wv] = inc;
        __syncthreads();
        uint64_t run = s_base + inc - sum;
        for (int k = 0; k < wv; k++) run += s_wsum[k];
#pragma unroll
        for (int j = 0; j < PER; j++) { if (i0 + j < n) store(i0 + j, run); run += v[j]; }
        __syncthreads();
        if (tid == 1023) s_base = run;
        __syncthreads();
    }
    return s_base;
}

#endif  // __HIPCC__
#endif  // JTK_DEVICE_PRIMS_H
