// jtk_repeat.hip -- repeated token n-grams inside a document (jtk_batch_ngram_repeats in jtk_abi.cpp), by the rule of
// jtk_repeat_rules.h.  Integer only: the results are bit-exact.  No LDS and no barrier in any kernel here; the cross-lane
// operations (__shfl_up, __ballot) are evaluated by all 64 lanes outside any condition.  The partition is
// jtk_ngram.hip's: a workgroup of 4 waves takes 4 consecutive tiles of JTK_NG_TILE tokens of the batch's token array, a lane 8
// consecutive tokens; a launch covers the tiles that touch the token range [lo, hi) of one group of whole documents, and a lane
// takes the positions of its 8 that lie in the range.
//
//   k_rp_preset   n_repeat = n_covered = 0 where asked for, and 0 into the batch's packed top word of every document.
//   k_rp_insert   pass 1.  k of every n-gram of the lane's positions (jtk_rp_lane_keys: the document's key changes with the
//                 document), then per run of equal k among them (jtk_rp_lane_runs) one 64-bit atomicCAS walk to the slot, one
//                 64-bit atomicMin of the run's first position into first[slot] and one atomicAdd of the run's length into
//                 count[slot].  A page of one token repeated costs a lane one pair of atomics, not eight; merging further,
//                 across the lanes of a wave, was not built (DESIGN.md section 4.24 says why).
//   k_rp_flags    pass 2.  The home slots of a lane's up to 8 keys are gathered before any probe goes on, then each probe runs to
//                 its slot and reads first and count; the mode decides the start bit (jtk_rp_is_repeat).  Lanes 33 - n .. 31 look
//                 up the n-gram that starts at position w0 - 32 + lane where that lies in the range (the backward halo).  The
//                 window, the flag bytes -- one 8-byte store where the pointer is 8-byte aligned and all 8 tokens are in the range,
//                 bytes otherwise -- and the per-document counts are k_ng_overlap's.  An n-gram at its own first position offers
//                 (count, position) to its document: one 64-bit atomicMax per document per lane (jtk_rp_lane_top).
//   k_rp_top      top_count and top_first of every document out of the packed word.
#include "jtk_kernels.h"
#include "jtk_repeat_rules.h"

namespace {

constexpr int RP_THREADS = 64 * JTK_NG_BLOCK_TILES;
constexpr int RP_BLOCK_TOKENS = JTK_NG_TILE * JTK_NG_BLOCK_TILES;
constexpr int RP_MAX_BLOCKS = 4096;                              // the one-lane-per-document kernels stride
static_assert(JTK_NG_TILE == 64 * JTK_NG_LANE && JTK_NG_LANE == 8, "a wave's lanes take 8 tokens each: one byte of start bits");

struct DevCas {
    __device__ uint64_t operator()(uint64_t* p, uint64_t k) const {
        return (uint64_t)atomicCAS((unsigned long long*)p, 0ull, (unsigned long long)k);
    }
};

__global__ void __launch_bounds__(256) k_rp_preset(int64_t n_docs, int32_t* __restrict__ n_repeat, int32_t* __restrict__ n_covered,
                                                   uint64_t* __restrict__ top) {
    for (int64_t d = (int64_t)blockIdx.x * 256 + threadIdx.x; d < n_docs; d += (int64_t)gridDim.x * 256) {
        if (n_repeat) n_repeat[d] = 0;
        if (n_covered) n_covered[d] = 0;
        if (top) top[d] = 0;
    }
}

__global__ void __launch_bounds__(256) k_rp_top(int64_t n_docs, const uint64_t* __restrict__ top, int32_t* __restrict__ top_count,
                                                int64_t* __restrict__ top_first) {
    for (int64_t d = (int64_t)blockIdx.x * 256 + threadIdx.x; d < n_docs; d += (int64_t)gridDim.x * 256) {
        const uint64_t packed = top[d];
        if (top_count) top_count[d] = jtk_rp_top_count(packed);
        if (top_first) top_first[d] = jtk_rp_top_first(packed);
    }
}

__global__ void __launch_bounds__(RP_THREADS) k_rp_insert(JtkMhView v, uint64_t key, uint64_t base, uint64_t gn1, JtkRpTable t, int64_t lo, int64_t hi,
                                                          int64_t block0) {
    const int64_t i0 = (block0 + (int64_t)blockIdx.x) * RP_BLOCK_TOKENS + (int64_t)threadIdx.x * JTK_NG_LANE;
    if (i0 >= hi || i0 + JTK_NG_LANE <= lo) return;
    uint64_t ks[JTK_NG_LANE];
    const uint32_t have = jtk_rp_lane_keys(v, key, base, gn1, i0, lo, hi, ks);
    jtk_rp_lane_runs(have, ks, i0, [&](uint64_t k, int64_t at, uint32_t r) {
        const uint64_t slot = jtk_rp_claim(t.key, t.mask, k, DevCas());
        atomicMin((unsigned long long*)t.first + slot, (unsigned long long)at);
        atomicAdd(t.count + slot, r);
    });
}

__global__ void __launch_bounds__(RP_THREADS) k_rp_flags(JtkMhView v, uint64_t key, uint64_t base, uint64_t gn1, uint32_t mode, JtkRpTable t, int64_t lo,
                                                         int64_t hi, int64_t block0, uint8_t* __restrict__ flags, int32_t* __restrict__ n_repeat,
                                                         int32_t* __restrict__ n_covered, uint64_t* __restrict__ top) {
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t w0 = (block0 + (int64_t)blockIdx.x) * RP_BLOCK_TOKENS + (int64_t)wv * JTK_NG_TILE;
    const int64_t i0 = w0 + (int64_t)lane * JTK_NG_LANE;
    const bool live = i0 < hi && i0 + JTK_NG_LANE > lo;

    // the starts at the lane's own tokens
    uint32_t mine = 0, have = 0;
    uint64_t first[JTK_NG_LANE];
    uint32_t count[JTK_NG_LANE];
    if (live) {
        uint64_t ks[JTK_NG_LANE], seen[JTK_NG_LANE];
        have = jtk_rp_lane_keys(v, key, base, gn1, i0, lo, hi, ks);
#pragma unroll
        for (int j = 0; j < JTK_NG_LANE; j++)
            if ((have >> j) & 1u) seen[j] = t.key[ks[j] & t.mask];
#pragma unroll
        for (int j = 0; j < JTK_NG_LANE; j++)
            if ((have >> j) & 1u) {
                const uint64_t slot = jtk_rp_find_on(t.key, t.mask, ks[j] & t.mask, seen[j], ks[j]);
                first[j] = t.first[slot];
                count[j] = t.count[slot];
                if (jtk_rp_is_repeat(mode, i0 + j, first[j], count[j])) mine |= 1u << j;
            }
    }
    // the starts before the tile that reach into it: halo bit q = position w0 - 32 + q, where that lies in the range
    bool before_tile = false;
    const int64_t hp = w0 - 32 + lane;
    if (lane < 32 && lane >= 33 - v.ngram && hp >= lo && hp < hi && w0 < hi) {
        uint64_t k;
        if (jtk_rp_key_at(v, key, base, hp, &k)) {
            const uint64_t slot = jtk_rp_find(t.key, t.mask, k);
            before_tile = jtk_rp_is_repeat(mode, hp, t.first[slot], t.count[slot]);
        }
    }
    const uint32_t halo = (uint32_t)__ballot(before_tile);       // (all 64 lanes, outside any condition: so are the shuffles)
    uint32_t before[4];
#pragma unroll
    for (int k = 1; k <= 4; k++) {
        const uint32_t up = (uint32_t)__shfl_up((int)mine, k);
        before[k - 1] = lane >= k ? up : 0u;
    }
    if (!live) return;
    const uint64_t w = jtk_ng_window(mine, before, halo, lane);

    if (flags) {
        uint64_t bytes = 0;
#pragma unroll
        for (int j = 0; j < JTK_NG_LANE; j++) bytes |= (uint64_t)jtk_ng_flag(w, v.ngram, j) << (8 * j);
        if (((uintptr_t)flags & 7u) == 0 && i0 >= lo && i0 + JTK_NG_LANE <= hi) {
            *(uint64_t*)(flags + i0) = bytes;
        } else {
            for (int j = 0; j < JTK_NG_LANE; j++)
                if (i0 + j >= lo && i0 + j < hi) flags[i0 + j] = (uint8_t)(bytes >> (8 * j));
        }
    }
    if (n_repeat || n_covered) {
        v.total = hi;                                            // (the tokens of the lane before lo have no bit in w: nothing is added for them)
        jtk_ng_lane_docs(v, i0, w, [&](int64_t d, int32_t hit, int32_t cov, int64_t) {
            if (n_repeat && hit) atomicAdd(n_repeat + d, hit);
            if (n_covered && cov) atomicAdd(n_covered + d, cov);
        });
    }
    if (top)
        jtk_rp_lane_top(v, i0, have, first, count, [&](int64_t d, uint64_t packed) {
            atomicMax((unsigned long long*)top + d, (unsigned long long)packed);
        });
}

unsigned strided_blocks(int64_t items) {
    const int64_t nb = (items + 255) / 256;
    return (unsigned)(nb < 1 ? 1 : nb < RP_MAX_BLOCKS ? nb : RP_MAX_BLOCKS);
}

}  // namespace

void jtk_launch_repeat_preset(int64_t n_docs, int32_t* n_repeat, int32_t* n_covered, uint64_t* top, hipStream_t s) {
    if (n_docs <= 0 || !(n_repeat || n_covered || top)) return;
    hipLaunchKernelGGL(k_rp_preset, dim3(strided_blocks(n_docs)), dim3(256), 0, s, n_docs, n_repeat, n_covered, top);
}

void jtk_launch_repeat_group(const JtkMhView& v, uint64_t seed, uint64_t doc_index_base, uint32_t flags, const JtkRpTable& t, int64_t lo, int64_t hi,
                             uint8_t* tok_flags, int32_t* n_repeat, int32_t* n_covered, uint64_t* top, hipStream_t s) {
    if (hi <= lo) return;
    const int64_t block0 = lo / RP_BLOCK_TOKENS;
    const dim3 grid((unsigned)((hi + RP_BLOCK_TOKENS - 1) / RP_BLOCK_TOKENS - block0));
    const uint64_t key = jtk_rp_key(seed, v.ngram), gn1 = jtk_ng_pow(v.ngram);
    hipLaunchKernelGGL(k_rp_insert, grid, dim3(RP_THREADS), 0, s, v, key, doc_index_base, gn1, t, lo, hi, block0);
    hipLaunchKernelGGL(k_rp_flags, grid, dim3(RP_THREADS), 0, s, v, key, doc_index_base, gn1, flags, t, lo, hi, block0, tok_flags, n_repeat, n_covered,
                       top);
}

void jtk_launch_repeat_top(int64_t n_docs, const uint64_t* top, int32_t* top_count, int64_t* top_first, hipStream_t s) {
    if (n_docs <= 0 || !(top_count || top_first)) return;
    hipLaunchKernelGGL(k_rp_top, dim3(strided_blocks(n_docs)), dim3(256), 0, s, n_docs, top, top_count, top_first);
}
