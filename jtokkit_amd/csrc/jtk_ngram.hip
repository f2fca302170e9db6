// jtk_ngram.hip -- token n-gram sets and overlap (jtk_ngram_set_*, jtk_batch_ngram_overlap in jtk_abi.cpp), by the rule of
// jtk_ngram_rules.h.  Integer only: the results are bit-exact.  No LDS and no barrier in any kernel here; the cross-lane
// operations (jtk_wave_sum, __shfl_up, __ballot) are evaluated by all 64 lanes outside any condition.
//
//   k_ng_count        the sum of n_ngrams over the documents: what an add_batch may insert, for the capacity rule.
//   k_ng_insert       a workgroup of 4 waves takes 4 consecutive tiles of JTK_NG_TILE tokens.  A lane takes 8 consecutive tokens,
//                     finds the document of the first by one search over tok_off, and computes k of every n-gram that starts at
//                     one of them -- the first of a run directly, the following rolled (jtk_ng_lane_keys) --; each k claims a slot
//                     with a 64-bit atomicCAS (jtk_ng_insert).  The lanes that turned an empty slot into their key are summed over
//                     the wave and one lane adds the sum to the set's key count.
//   k_ng_insert_keys  one lane per key of an array, the same insert; a 0 is skipped, so the array may be an old table: this is
//                     add_keys (counted) and the rehash after growth (not counted).
//   k_ng_preset       n_hit = n_covered = 0, first_hit = -1 for every document: what the lanes of k_ng_overlap add into.
//   k_ng_overlap      the same walk.  The home slots of a lane's up to 8 keys are gathered before any probe goes on (8 loads in
//                     flight per lane), then each probe runs to its match or empty slot.  Lanes 33 - n .. 31 of a wave look up the
//                     n-gram that starts at position w0 - 32 + lane, before the wave's tile (the backward halo: <= 31 direct
//                     hashes and probes per 512 tokens); a ballot makes them one word.  A lane's window of 39 start bits is its
//                     own 8, the 8 of each of the four lanes before it (shuffles) and, in the tile's first four lanes, the halo.
//                     The 8 flag bytes go out as one 8-byte store where the pointer is 8-byte aligned and the lane has all 8
//                     tokens, as bytes otherwise.  Per document of its 8 tokens a lane adds its counts (atomicAdd) and its first
//                     start (atomicMin on the unsigned pattern: -1 is the largest) -- only where they are not 0, so a corpus
//                     without hits issues no atomic at all.
#include "jtk_kernels.h"
#include "jtk_ngram_rules.h"

namespace {

constexpr int NG_THREADS = 64 * JTK_NG_BLOCK_TILES;
constexpr int NG_BLOCK_TOKENS = JTK_NG_TILE * JTK_NG_BLOCK_TILES;
constexpr int NG_MAX_BLOCKS = 4096;                              // the one-lane-per-item kernels stride
static_assert(JTK_NG_TILE == 64 * JTK_NG_LANE && JTK_NG_LANE == 8, "a wave's lanes take 8 tokens each: one byte of start bits");

struct DevCas {
    __device__ uint64_t operator()(uint64_t* p, uint64_t k) const {
        return (uint64_t)atomicCAS((unsigned long long*)p, 0ull, (unsigned long long)k);
    }
};

__global__ void __launch_bounds__(256) k_ng_count(const int64_t* __restrict__ tok_off, const int32_t* __restrict__ status, int64_t n_docs,
                                                  int32_t ngram, unsigned long long* __restrict__ sum) {
    uint64_t n = 0;
    for (int64_t d = (int64_t)blockIdx.x * 256 + threadIdx.x; d < n_docs; d += (int64_t)gridDim.x * 256)
        if (status[d] >= 0) n += (uint64_t)jtk_ng_n_ngrams(tok_off[d + 1] - tok_off[d], ngram);
    n = jtk_wave_sum(n);                                         // (all 64 lanes, outside any condition)
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(sum, (unsigned long long)n);
}

__global__ void __launch_bounds__(NG_THREADS) k_ng_insert(JtkMhView v, uint64_t key, uint64_t gn1, uint64_t* __restrict__ table, uint64_t mask,
                                                          unsigned long long* __restrict__ count) {
    const int64_t held = v.tok_off[v.n_docs];
    if (held < v.total) v.total = held;                          // (never past what the offsets cover)
    const int64_t i0 = (int64_t)blockIdx.x * NG_BLOCK_TOKENS + (int64_t)threadIdx.x * JTK_NG_LANE;
    uint32_t added = 0;
    if (i0 < v.total) {
        uint64_t ks[JTK_NG_LANE];
        const uint32_t have = jtk_ng_lane_keys(v, key, gn1, i0, ks);
#pragma unroll
        for (int j = 0; j < JTK_NG_LANE; j++)
            if ((have >> j) & 1u) added += (uint32_t)jtk_ng_insert(table, mask, ks[j], DevCas());
    }
    added = jtk_wave_sum(added);                                 // (all 64 lanes, outside any condition)
    if ((threadIdx.x & 63) == 0 && added) atomicAdd(count, (unsigned long long)added);
}

__global__ void __launch_bounds__(256) k_ng_insert_keys(const uint64_t* __restrict__ keys, int64_t n, uint64_t* __restrict__ table, uint64_t mask,
                                                        unsigned long long* __restrict__ count) {
    uint32_t added = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const uint64_t k = keys[i];
        if (k) added += (uint32_t)jtk_ng_insert(table, mask, k, DevCas());
    }
    added = jtk_wave_sum(added);                                 // (all 64 lanes, outside any condition)
    if (count && (threadIdx.x & 63) == 0 && added) atomicAdd(count, (unsigned long long)added);
}

__global__ void __launch_bounds__(256) k_ng_preset(int64_t n_docs, int32_t* __restrict__ n_hit, int32_t* __restrict__ n_covered,
                                                   int64_t* __restrict__ first_hit) {
    for (int64_t d = (int64_t)blockIdx.x * 256 + threadIdx.x; d < n_docs; d += (int64_t)gridDim.x * 256) {
        if (n_hit) n_hit[d] = 0;
        if (n_covered) n_covered[d] = 0;
        if (first_hit) first_hit[d] = -1;
    }
}

__global__ void __launch_bounds__(NG_THREADS) k_ng_overlap(JtkMhView v, uint64_t key, uint64_t gn1, const uint64_t* __restrict__ table, uint64_t mask,
                                                           uint8_t* __restrict__ flags, int32_t* __restrict__ n_hit, int32_t* __restrict__ n_covered,
                                                           int64_t* __restrict__ first_hit) {
    const int64_t held = v.tok_off[v.n_docs];
    if (held < v.total) v.total = held;                          // (never past what the offsets cover)
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t w0 = (int64_t)blockIdx.x * NG_BLOCK_TOKENS + (int64_t)wv * JTK_NG_TILE;
    const int64_t i0 = w0 + (int64_t)lane * JTK_NG_LANE;

    // the starts at the lane's own tokens
    uint32_t mine = 0;
    if (i0 < v.total) {
        uint64_t ks[JTK_NG_LANE], seen[JTK_NG_LANE];
        const uint32_t have = jtk_ng_lane_keys(v, key, gn1, i0, ks);
#pragma unroll
        for (int j = 0; j < JTK_NG_LANE; j++)
            if ((have >> j) & 1u) seen[j] = table[ks[j] & mask];
#pragma unroll
        for (int j = 0; j < JTK_NG_LANE; j++)
            if (((have >> j) & 1u) && jtk_ng_probe_on(table, mask, ks[j] & mask, seen[j], ks[j])) mine |= 1u << j;
    }
    // the starts before the tile that reach into it: halo bit q = position w0 - 32 + q
    bool before_tile = false;
    const int64_t hp = w0 - 32 + lane;
    if (lane < 32 && lane >= 33 - v.ngram && hp >= 0 && w0 < v.total) {
        uint64_t k;
        if (jtk_ng_key_at(v, key, hp, &k)) before_tile = jtk_ng_lookup(table, mask, k);
    }
    const uint32_t halo = (uint32_t)__ballot(before_tile);       // (all 64 lanes, outside any condition: so are the shuffles)
    uint32_t before[4];
#pragma unroll
    for (int k = 1; k <= 4; k++) {
        const uint32_t up = (uint32_t)__shfl_up((int)mine, k);
        before[k - 1] = lane >= k ? up : 0u;
    }
    if (i0 >= v.total) return;
    const uint64_t w = jtk_ng_window(mine, before, halo, lane);

    if (flags) {
        uint64_t bytes = 0;
#pragma unroll
        for (int j = 0; j < JTK_NG_LANE; j++) bytes |= (uint64_t)jtk_ng_flag(w, v.ngram, j) << (8 * j);
        if (((uintptr_t)flags & 7u) == 0 && i0 + JTK_NG_LANE <= v.total) {
            *(uint64_t*)(flags + i0) = bytes;
        } else {
            for (int j = 0; j < JTK_NG_LANE && i0 + j < v.total; j++) flags[i0 + j] = (uint8_t)(bytes >> (8 * j));
        }
    }
    if (n_hit || n_covered || first_hit)
        jtk_ng_lane_docs(v, i0, w, [&](int64_t d, int32_t hit, int32_t cov, int64_t first) {
            if (n_hit && hit) atomicAdd(n_hit + d, hit);
            if (n_covered && cov) atomicAdd(n_covered + d, cov);
            if (first_hit && first >= 0) atomicMin((unsigned long long*)first_hit + d, (unsigned long long)first);
        });
}

unsigned strided_blocks(int64_t items) {
    const int64_t nb = (items + 255) / 256;
    return (unsigned)(nb < 1 ? 1 : nb < NG_MAX_BLOCKS ? nb : NG_MAX_BLOCKS);
}
dim3 tile_grid(int64_t total) { return dim3((unsigned)((total + NG_BLOCK_TOKENS - 1) / NG_BLOCK_TOKENS)); }

}  // namespace

void jtk_launch_ngram_count(const JtkMhView& v, uint64_t* sum, hipStream_t s) {
    if (v.n_docs <= 0) return;
    hipLaunchKernelGGL(k_ng_count, dim3(strided_blocks(v.n_docs)), dim3(256), 0, s, v.tok_off, v.status, v.n_docs, v.ngram, (unsigned long long*)sum);
}

void jtk_launch_ngram_insert(const JtkMhView& v, uint64_t seed, uint64_t* table, int64_t capacity, uint64_t* count, hipStream_t s) {
    if (v.n_docs <= 0 || v.total <= 0) return;
    hipLaunchKernelGGL(k_ng_insert, tile_grid(v.total), dim3(NG_THREADS), 0, s, v, jtk_ng_key(seed, v.ngram), jtk_ng_pow(v.ngram), table,
                       (uint64_t)capacity - 1, (unsigned long long*)count);
}

void jtk_launch_ngram_insert_keys(const uint64_t* keys, int64_t n, uint64_t* table, int64_t capacity, uint64_t* count_or_null, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_ng_insert_keys, dim3(strided_blocks(n)), dim3(256), 0, s, keys, n, table, (uint64_t)capacity - 1,
                       (unsigned long long*)count_or_null);
}

void jtk_launch_ngram_overlap(const JtkMhView& v, uint64_t seed, const uint64_t* table, int64_t capacity, uint8_t* flags, int32_t* n_hit,
                              int32_t* n_covered, int64_t* first_hit, hipStream_t s) {
    if (v.n_docs <= 0) return;
    if (n_hit || n_covered || first_hit)
        hipLaunchKernelGGL(k_ng_preset, dim3(strided_blocks(v.n_docs)), dim3(256), 0, s, v.n_docs, n_hit, n_covered, first_hit);
    if (v.total > 0 && (flags || n_hit || n_covered || first_hit))
        hipLaunchKernelGGL(k_ng_overlap, tile_grid(v.total), dim3(NG_THREADS), 0, s, v, jtk_ng_key(seed, v.ngram), jtk_ng_pow(v.ngram), table,
                           (uint64_t)capacity - 1, flags, n_hit, n_covered, first_hit);
}
