// jtk_compact.hip -- compact token ids (jtk_batch_compact and JTK_ENCODE_COMPACT_IDS in jtk_abi.cpp), by the rule of
// jtk_compact_rules.h: the int32 ids of a token range [t0, t1) become a uint16 plane and a plane of hb high bits per token.
//
//   k_compact<HB, VEC>   one pass, streaming: 4 B read and 2 + HB / 8 B written per token, no LDS.  A lane takes 8 consecutive
//                        tokens: two 16-byte loads, one 16-byte store of the 8 lo entries, and its 8 * HB high bits placed by
//                        jtk_compact_hi_shift.  Those are a quarter word (HB 1), half a word (HB 2), or 1, 2, 4 whole words
//                        (HB 4, 8, 16); quarter and half words are OR-ed across the 4 or 2 neighbouring lanes (__shfl_xor),
//                        and the first lane of the group stores the word: one vector store per word, words of a wave
//                        contiguous; a lane's 2 or 4 whole words (HB 8, 16: custom encodings only) leave in one 8- or 16-byte
//                        store.  (A wave ballot would give the bits lane-major -- bit L of ballot j is token 8 L + j --,
//                        the transpose of the plane's order; with one token per lane it fits, but then lo cannot leave in
//                        16-byte stores.  The ballot form was not built, so the two were not timed against each other.)
//                        The pass starts at jtk_compact_range_start(t0), a multiple of 32 tokens, so every word it stores is
//                        whole and the 16-byte accesses are aligned whenever the buffers are; the ragged end (fewer than 8
//                        tokens in a lane) takes 4-byte loads and 2- and 4-byte stores, and nothing is read or written at or
//                        above t1 except the zero bits of the last hi word.  VEC = false is the same pass for buffers that
//                        are not 16-byte aligned.
//                        d_total != NULL: the range ends at min(t1, *d_total) -- a small job launches it before the host knows
//                        the token count.
#include "jtk_kernels.h"
#include "jtk_compact_rules.h"

namespace {

constexpr int CP_LANE_TOKENS = 8;
constexpr int CP_TILE = 256 * CP_LANE_TOKENS;    // tokens per workgroup step
constexpr int CP_MAX_BLOCKS = 4096;              // a workgroup strides over the tiles

// ids, lo, hi point at token tb = the range's start (a multiple of 32); n tokens from there
template <int HB, bool VEC>
__global__ void __launch_bounds__(256) k_compact(const int32_t* __restrict__ ids, int64_t n, const int64_t* __restrict__ d_total,
                                                 int64_t tb, uint16_t* __restrict__ lo, uint32_t* __restrict__ hi) {
    if (d_total) {
        const int64_t m = *d_total - tb;
        n = m < n ? m : n;
    }
    for (int64_t base = (int64_t)blockIdx.x * CP_TILE; base < n; base += (int64_t)gridDim.x * CP_TILE) {
        const int64_t i = base + (int64_t)threadIdx.x * CP_LANE_TOKENS;
        const int64_t left = n - i;                                 // (<= 0: the lane only takes part in the ORs)
        const bool full = left >= CP_LANE_TOKENS;
        int32_t v[CP_LANE_TOKENS];
        if (VEC && full) {
            const int4 a = *(const int4*)(ids + i), b = *(const int4*)(ids + i + 4);
            v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
        } else {
#pragma unroll
            for (int k = 0; k < CP_LANE_TOKENS; k++) v[k] = k < left ? ids[i + k] : 0;
        }
        if (VEC && full) {
            uint4 p;
            p.x = (uint32_t)jtk_compact_lo(v[0]) | (uint32_t)jtk_compact_lo(v[1]) << 16;
            p.y = (uint32_t)jtk_compact_lo(v[2]) | (uint32_t)jtk_compact_lo(v[3]) << 16;
            p.z = (uint32_t)jtk_compact_lo(v[4]) | (uint32_t)jtk_compact_lo(v[5]) << 16;
            p.w = (uint32_t)jtk_compact_lo(v[6]) | (uint32_t)jtk_compact_lo(v[7]) << 16;
            *(uint4*)(lo + i) = p;
        } else {
#pragma unroll
            for (int k = 0; k < CP_LANE_TOKENS; k++) if (k < left) lo[i + k] = jtk_compact_lo(v[k]);
        }
        if constexpr (HB == 0) continue;
        else if constexpr (HB <= 4) {
            // the lane's 8 * HB bits lie inside one word (i is a multiple of 8); ids past the end are 0 and add nothing
            uint32_t w = jtk_compact_hi_compose(v, i, CP_LANE_TOKENS, HB);
            constexpr int group = 4 / HB;                           // lanes per word: 4, 2, 1
            if (group >= 2) w |= __shfl_xor(w, 1);
            if (group >= 4) w |= __shfl_xor(w, 2);
            if ((threadIdx.x & (group - 1)) == 0 && left > 0) hi[jtk_compact_hi_word(i, HB)] = w;
        } else {
            constexpr int per = 32 / HB;                            // ids per word: 4, 2
            constexpr int nw = CP_LANE_TOKENS / per;                // words per lane: 2, 4 (consecutive, from word i * HB / 32)
            uint32_t w[nw];
#pragma unroll
            for (int k = 0; k < nw; k++) w[k] = jtk_compact_hi_compose(v + k * per, i + k * per, per, HB);
            uint32_t* dst = hi + jtk_compact_hi_word(i, HB);
            if (VEC && full) {
                if constexpr (nw == 2) *(uint2*)dst = make_uint2(w[0], w[1]);
                else *(uint4*)dst = make_uint4(w[0], w[1], w[2], w[3]);
            } else {
#pragma unroll
                for (int k = 0; k < nw; k++) if (k * per < left) dst[k] = w[k];
            }
        }
    }
}

template <int HB>
void launch(bool vec, unsigned blocks, hipStream_t s, const int32_t* ids, int64_t n, const int64_t* d_total, int64_t tb,
            uint16_t* lo, uint32_t* hi) {
    if (vec) hipLaunchKernelGGL((k_compact<HB, true>), dim3(blocks), dim3(256), 0, s, ids, n, d_total, tb, lo, hi);
    else hipLaunchKernelGGL((k_compact<HB, false>), dim3(blocks), dim3(256), 0, s, ids, n, d_total, tb, lo, hi);
}

}  // namespace

void jtk_launch_compact(const int32_t* ids, int64_t t0, int64_t t1, const int64_t* d_total, uint16_t* lo, uint32_t* hi,
                        int64_t origin, int hb, hipStream_t s) {
    if (t1 <= t0) return;
    const int64_t tb = jtk_compact_range_start(t0), n = t1 - tb;
    ids += tb;
    lo += tb - origin;
    if (hb) hi += jtk_compact_hi_word(tb - origin, hb);
    const bool vec = (((uintptr_t)ids | (uintptr_t)lo | (hb >= 8 ? (uintptr_t)hi : 0)) & 15u) == 0;
    const int64_t tiles = (n + CP_TILE - 1) / CP_TILE;
    const unsigned blocks = (unsigned)(tiles < CP_MAX_BLOCKS ? tiles : CP_MAX_BLOCKS);
    switch (hb) {
        case 0: launch<0>(vec, blocks, s, ids, n, d_total, tb, lo, hi); break;
        case 1: launch<1>(vec, blocks, s, ids, n, d_total, tb, lo, hi); break;
        case 2: launch<2>(vec, blocks, s, ids, n, d_total, tb, lo, hi); break;
        case 4: launch<4>(vec, blocks, s, ids, n, d_total, tb, lo, hi); break;
        case 8: launch<8>(vec, blocks, s, ids, n, d_total, tb, lo, hi); break;
        default: launch<16>(vec, blocks, s, ids, n, d_total, tb, lo, hi); break;
    }
}
