// jtk_minhash.hip -- MinHash signatures, LSH band keys and signature agreement (jtk_batch_minhash, jtk_batch_minhash_agree in
// jtk_abi.cpp), by the rule of jtk_minhash_rules.h.  Integer only: the results are bit-exact.
//
//   k_mh_preset       every word of sig = 0xFFFFFFFF and n_shingles[d]: the rows of documents without shingles are final, the
//                     rows of documents that span tiles are what the tiles' atomic minima start from.  It is a kernel of its
//                     own, queued before k_mh_tiles on the same stream: "the first tile stores, the others combine" would be a
//                     race between workgroups.
//   k_mh_tiles<R>     a workgroup of 4 waves takes 4 consecutive tiles of JTK_MH_TILE tokens, one per wave.
//                     Step 1: a lane takes 8 consecutive tokens of its wave's tile, finds the document of the first by one
//                     search over tok_off (jtk_first_gt), moves forward from there, and writes x of every shingle that starts
//                     at one of them into LDS; the up to n - 1 tokens past the tile's end (the halo) are read from global
//                     memory, where the neighbouring lanes have just read them.
//                     Step 2: lanes own hash functions -- lane L holds a, b and a running minimum of functions L, L + 64, ...
//                     (R = ceil(K / 64) of them, 1..4) in registers -- and the wave walks the documents of its tile
//                     (jtk_mh_segment; everything about a document is the same in all lanes: scalar loads and branches).
//                     For every shingle all lanes read one LDS word, a broadcast, and take R multiply-add-shift values and
//                     minima.  At the end of a document's part the minima are flushed: rows of K consecutive words, stored
//                     when the document lies inside the tile, atomicMin when it spans tiles; then the next document that has
//                     tokens is found -- the next one, or by a search when that one is empty, so a run of empty documents
//                     costs one search.  With K < 64 the lanes above K idle: their share of a tile was not given to other
//                     shingles.
//   k_mh_bands        one lane per (document, band): the fold of the band's r signature words.
//   k_mh_agree<VEC>   one wave per pair: both rows in 16-byte loads (VEC: K a multiple of 4 and sig 16-byte aligned, so every
//                     row is) or word by word, a compare, and a wave sum that all 64 lanes run.  A pair with an index outside
//                     [0, n_sig) gets -1 and reads no row.
#include "jtk_kernels.h"
#include "jtk_minhash_rules.h"

namespace {

constexpr int MH_THREADS = 64 * JTK_MH_BLOCK_TILES;
constexpr int MH_LANE_TOKENS = JTK_MH_TILE / 64;                 // 8
constexpr int MH_BLOCK_TOKENS = JTK_MH_TILE * JTK_MH_BLOCK_TILES;
constexpr int MH_MAX_BLOCKS = 4096;                              // the one-lane-per-item kernels stride

__global__ void __launch_bounds__(256) k_mh_preset(const int64_t* __restrict__ tok_off, const int32_t* __restrict__ status, int64_t n_docs,
                                                   int32_t ngram, int32_t K, uint32_t* __restrict__ sig, int32_t* __restrict__ n_shingles) {
    const int64_t step = (int64_t)gridDim.x * 256, first = (int64_t)blockIdx.x * 256 + threadIdx.x;
    for (int64_t i = first; i < n_docs * K; i += step) sig[i] = JTK_MH_EMPTY;
    if (n_shingles)
        for (int64_t d = first; d < n_docs; d += step)
            n_shingles[d] = (int32_t)jtk_mh_n_shingles(status[d] < 0 ? 0 : tok_off[d + 1] - tok_off[d], ngram);
}

template <int R>
__global__ void __launch_bounds__(MH_THREADS) k_mh_tiles(JtkMhView v, uint64_t key, int32_t K, uint32_t* __restrict__ sig) {
    __shared__ uint32_t s_x[MH_BLOCK_TOKENS];
    const int64_t held = v.tok_off[v.n_docs];
    if (held < v.total) v.total = held;                          // (never past what the offsets cover)
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t tile0 = (int64_t)blockIdx.x * MH_BLOCK_TOKENS;

    // step 1: x of the shingles that start at the lane's tokens
    const int64_t i0 = tile0 + (int64_t)tid * MH_LANE_TOKENS;
    if (i0 < v.total) {
        int64_t d = jtk_mh_doc_of(v, 0, i0);
        for (int j = 0; j < MH_LANE_TOKENS && i0 + j < v.total; j++) {
            const int64_t i = i0 + j;
            if (v.tok_off[d + 1] <= i) d = jtk_mh_next_doc(v, d, i);
            uint32_t x;
            if (jtk_mh_x_at(v, d, i, key, &x)) s_x[tid * MH_LANE_TOKENS + j] = x;
        }
    }
    __syncthreads();

    // step 2: the wave's tile [w0, w1)
    const int64_t w0 = tile0 + (int64_t)wv * JTK_MH_TILE;
    if (w0 >= v.total) return;                                   // (no barrier below)
    const int64_t w1 = w0 + JTK_MH_TILE < v.total ? w0 + JTK_MH_TILE : v.total;
    uint32_t a_lo[R], a_hi[R], mn[R];
    uint64_t b[R];
#pragma unroll
    for (int r = 0; r < R; r++) {
        const int k = lane + 64 * r;                             // (a lane with k >= K computes and never stores)
        const uint64_t a = jtk_mh_a(key, k);
        a_lo[r] = (uint32_t)a; a_hi[r] = (uint32_t)(a >> 32);
        b[r] = jtk_mh_b(key, k);
        mn[r] = JTK_MH_EMPTY;
    }
    int64_t d = jtk_mh_doc_of(v, 0, w0), pos = w0;
    while (pos < w1) {
        const JtkMhSeg seg = jtk_mh_segment(v, d, pos, w0, w1);
        if (seg.live && seg.sh_hi > seg.sh_lo) {
            const uint32_t* xs = s_x + (seg.sh_lo - tile0);
            const int n = (int)(seg.sh_hi - seg.sh_lo);
#pragma unroll 4
            for (int i = 0; i < n; i++) {
                const uint32_t x = xs[i];
#pragma unroll
                for (int r = 0; r < R; r++) {
                    const uint32_t val = jtk_mh_value(a_lo[r], a_hi[r], b[r], x);
                    mn[r] = val < mn[r] ? val : mn[r];
                }
            }
            uint32_t* row = sig + d * K;
#pragma unroll
            for (int r = 0; r < R; r++) {
                const int k = lane + 64 * r;
                if (k < K) {
                    if (seg.whole) row[k] = mn[r];
                    else atomicMin(row + k, mn[r]);
                }
                mn[r] = JTK_MH_EMPTY;
            }
        }
        pos = seg.end;
        if (pos < w1) d = jtk_mh_next_doc(v, d, pos);
    }
}

__global__ void __launch_bounds__(256) k_mh_bands(const uint32_t* __restrict__ sig, int64_t n_docs, uint64_t key, int32_t K, int32_t bands,
                                                  uint64_t* __restrict__ band_keys) {
    const int64_t step = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n_docs * bands; i += step) {
        const int64_t d = i / bands;
        band_keys[i] = jtk_mh_band_key(key, sig + d * K, K, bands, (int32_t)(i - d * bands));
    }
}

template <bool VEC>
__global__ void __launch_bounds__(256) k_mh_agree(const uint32_t* __restrict__ sig, int64_t n_sig, int32_t K, const int64_t* __restrict__ pair_a,
                                                  const int64_t* __restrict__ pair_b, int64_t n_pairs, int32_t* __restrict__ agree) {
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (int64_t p = (int64_t)blockIdx.x * 4 + wv; p < n_pairs; p += (int64_t)gridDim.x * 4) {
        const int64_t ia = pair_a[p], ib = pair_b[p];
        const bool ok = ia >= 0 && ia < n_sig && ib >= 0 && ib < n_sig;        // (the same in all lanes)
        uint32_t n = 0;
        if (ok) {
            const uint32_t* ra = sig + ia * K;
            const uint32_t* rb = sig + ib * K;
            if (VEC) {
                if (4 * lane < K) {                                              // (K <= 256: one load per lane covers the row)
                    const uint4 qa = *(const uint4*)(ra + 4 * lane), qb = *(const uint4*)(rb + 4 * lane);
                    n = (qa.x == qb.x) + (qa.y == qb.y) + (qa.z == qb.z) + (qa.w == qb.w);
                }
            } else {
                for (int k = lane; k < K; k += 64) n += ra[k] == rb[k];
            }
        }
        n = jtk_wave_sum(n);                                                     // (all 64 lanes, outside any condition)
        if (lane == 0) agree[p] = ok ? (int32_t)n : -1;
    }
}

unsigned strided_blocks(int64_t items, int per) {
    const int64_t nb = (items + per - 1) / per;
    return (unsigned)(nb < 1 ? 1 : nb < MH_MAX_BLOCKS ? nb : MH_MAX_BLOCKS);
}

}  // namespace

void jtk_launch_minhash(const JtkMhView& v, uint64_t seed, int32_t num_hashes, int32_t bands, uint32_t* sig, int32_t* n_shingles,
                        uint64_t* band_keys, hipStream_t s) {
    if (v.n_docs <= 0) return;
    const uint64_t key = jtk_mh_key(seed, v.ngram);
    const int32_t K = num_hashes;
    hipLaunchKernelGGL(k_mh_preset, dim3(strided_blocks(v.n_docs * K, 256)), dim3(256), 0, s, v.tok_off, v.status, v.n_docs, v.ngram, K, sig,
                       n_shingles);
    if (v.total > 0) {
        const dim3 grid((unsigned)((v.total + MH_BLOCK_TOKENS - 1) / MH_BLOCK_TOKENS)), block(MH_THREADS);
        switch ((K + 63) / 64) {
            case 1: hipLaunchKernelGGL(k_mh_tiles<1>, grid, block, 0, s, v, key, K, sig); break;
            case 2: hipLaunchKernelGGL(k_mh_tiles<2>, grid, block, 0, s, v, key, K, sig); break;
            case 3: hipLaunchKernelGGL(k_mh_tiles<3>, grid, block, 0, s, v, key, K, sig); break;
            default: hipLaunchKernelGGL(k_mh_tiles<4>, grid, block, 0, s, v, key, K, sig); break;
        }
    }
    if (bands > 0 && band_keys)
        hipLaunchKernelGGL(k_mh_bands, dim3(strided_blocks(v.n_docs * bands, 256)), dim3(256), 0, s, sig, v.n_docs, key, K, bands, band_keys);
}

void jtk_launch_minhash_agree(const uint32_t* sig, int64_t n_sig, int32_t num_hashes, const int64_t* pair_a, const int64_t* pair_b,
                              int64_t n_pairs, int32_t* agree, hipStream_t s) {
    if (n_pairs <= 0) return;
    const dim3 grid(strided_blocks(n_pairs, 4)), block(256);
    if (num_hashes % 4 == 0 && ((uintptr_t)sig & 15u) == 0)
        hipLaunchKernelGGL(k_mh_agree<true>, grid, block, 0, s, sig, n_sig, num_hashes, pair_a, pair_b, n_pairs, agree);
    else
        hipLaunchKernelGGL(k_mh_agree<false>, grid, block, 0, s, sig, n_sig, num_hashes, pair_a, pair_b, n_pairs, agree);
}
