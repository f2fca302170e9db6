// jtk_chunk_prefer.hip -- token-budget chunks that end at paragraph, line, sentence and word boundaries
// (jtk_batch_chunk_prefer, jtk_batch_token_cut_levels in jtk_abi.cpp).  The rule is jtk_chunk_prefer_rules.h; the records, the
// byte scan and the rows are those of jtk_chunk.hip.
//
//   cp_levels        the level plane: per token of the last encode the level of the cut before it.  A tile of 2048 tokens per
//                    step: every lane reads 8 ids coalesced, takes the first byte and the last <= 3 bytes of each id's byte
//                    string from the decode table and puts the tail into LDS; after one barrier a cut's lookback x(1..3) is
//                    put together from the tails of the three tokens before it in LDS.  Document edges are ignored here ...
//   cp_doc_heads     ... and set right by one lane per document: 6 for its first token, and the two tokens after it again
//                    with a lookback that stops at the document's start (only they can see across it).
//   cp_count_short   one lane per document of at most JTK_CP_LONG_TOKENS tokens (or of a single chunk): the header's walk on
//                    the plane, its window search reading eight cuts per load, counting; the others are listed for ...
//   cp_long          ... one workgroup each.  Its 256 lanes take a window from the end the rule prefers -- the chunk's end
//                    window from the top, the overlap window from the bottom --, 256 cuts per round, and reduce to
//                    (max level, nearest cut); a round that has seen the highest enabled level ends the search.  Same kernel
//                    counts and writes.
//   scan             chunk_off (jtk_launch_scan_i64), the totals for the host
//   cp_write_short   the records of the short documents (the walk again, writing), then the byte spans (k_ck_bytes)
#include "jtk_chunk_prefer_rules.h"
#include "jtk_device_prims.h"
#include "jtk_kernels.h"

namespace {

constexpr int CT = JTK_DEC_TILE;               // tokens per tile of the level plane
constexpr int CP_PLANE_BLOCKS = 2048;          // persistent workgroups over the tiles (the token count stays on the device)
constexpr int CP_LONG_BLOCKS = 2048;           // persistent workgroups over the long documents
constexpr uint64_t CP_QMAX = ((uint64_t)1 << 40) - 1;
static_assert(CT == 256 * 8, "a tile is 256 lanes x 8 tokens");

__device__ __forceinline__ bool cp_is_long(int64_t n, int64_t N) { return n > N && n > JTK_CP_LONG_TOKENS; }

// The last min(len, 3) bytes of an id's byte string, the last one lowest, and their number in bits 24..25; *y = its first
// byte.  An id outside the table is one byte 0 (its document is refused), an empty string has y = 0 (B holds, as in bnd).
__device__ __forceinline__ uint32_t cp_tail(const uint32_t* tab_off, const uint8_t* blob, uint32_t n_ids, int32_t id, int* y) {
    *y = 0;
    if ((uint32_t)id >= n_ids) return 1u << 24;
    const uint32_t o0 = tab_off[id], o1 = tab_off[id + 1], c = min(o1 - o0, 3u);
    if (c > 0) *y = blob[o0];
    uint32_t tw = c << 24;
    for (uint32_t k = 0; k < c; k++) tw |= (uint32_t)blob[o1 - 1 - k] << (8 * k);
    return tw;
}

// lookback bytes so far (acc: x(1) lowest, c of them) + the tail of the token before them
__device__ __forceinline__ void cp_push(uint32_t& acc, uint32_t& c, uint32_t tw) {
    acc |= (uint32_t)(((uint64_t)(tw & 0xFFFFFFu) << (8 * c)) & 0xFFFFFFu);
    c = min(3u, c + (tw >> 24));
}

__device__ __forceinline__ int cp_level(uint32_t prefer, int y, uint32_t acc, uint32_t c) {
    return jtk_cut_level(prefer, y, c >= 1 ? (int)(acc & 0xFFu) : -1, c >= 2 ? (int)((acc >> 8) & 0xFFu) : -1,
                         c >= 3 ? (int)((acc >> 16) & 0xFFu) : -1);
}

__global__ void __launch_bounds__(256) k_cp_levels(JtkChunkWork w, const uint8_t* blob, uint32_t prefer, uint8_t* plane) {
    __shared__ uint32_t s_tail[CT + 3];                                   // [3 + i]: token i of the tile; [0..2]: the three before it
    const int tid = threadIdx.x;
    const int64_t n_tok = w.tok_off[w.n_docs];
    for (int64_t base = (int64_t)blockIdx.x * CT; base < n_tok; base += (int64_t)gridDim.x * CT) {   // (uniform per workgroup)
        int y[8];
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const int64_t t = base + j * 256 + tid;
            s_tail[3 + j * 256 + tid] = cp_tail(w.tab_off, blob, w.n_ids_table, t < n_tok ? w.tokens[t] : -1, &y[j]);
        }
        if (tid < 3) {
            const int64_t t = base - 3 + tid;
            int y0;
            s_tail[tid] = t >= 0 ? cp_tail(w.tab_off, blob, w.n_ids_table, w.tokens[t], &y0) : 0u;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const int i = j * 256 + tid;
            uint32_t acc = 0, c = 0;
            cp_push(acc, c, s_tail[i + 2]);
            cp_push(acc, c, s_tail[i + 1]);
            cp_push(acc, c, s_tail[i]);
            if (base + i < n_tok) plane[base + i] = (uint8_t)cp_level(prefer, y[j], acc, c);
        }
        __syncthreads();                                                  // (s_tail is rewritten by the next tile)
    }
}

__global__ void __launch_bounds__(256) k_cp_doc_heads(JtkChunkWork w, const uint8_t* blob, uint32_t prefer, uint8_t* plane) {
    const int64_t d = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= w.n_docs) return;
    const int64_t t0 = w.tok_off[d], n = w.tok_off[d + 1] - t0;
    if (n <= 0) return;
    plane[t0] = JTK_LEVEL_DOC_END;
    uint32_t tw[2];
    for (int i = 1; i < 3 && i < n; i++) {
        int y, y0;
        tw[i - 1] = cp_tail(w.tab_off, blob, w.n_ids_table, w.tokens[t0 + i - 1], &y0);
        cp_tail(w.tab_off, blob, w.n_ids_table, w.tokens[t0 + i], &y);
        uint32_t acc = 0, c = 0;
        cp_push(acc, c, tw[i - 1]);
        if (i == 2) cp_push(acc, c, tw[0]);
        plane[t0 + i] = (uint8_t)cp_level(prefer, y, acc, c);
    }
}

// jtk_cut_scan for one lane on the plane: eight cuts per load where the window covers an aligned word, and no further than the
// word that has seen `top`.
__device__ __forceinline__ int cp_scan(const uint8_t* pl, int64_t a, int64_t b, bool last, int64_t* at, int top) {
    int m = 0;
    if (last) {
        for (int64_t i = b; i > a && m < top;) {
            if ((((uintptr_t)(pl + i)) & 7u) == 0 && i - 8 >= a) {
                const uint64_t wd = *reinterpret_cast<const uint64_t*>(pl + i - 8);
#pragma unroll
                for (int k = 7; k >= 0; k--) { const int l = (int)((wd >> (8 * k)) & 0xFFu); if (l > m) { m = l; *at = i - 8 + k; } }
                i -= 8;
            } else {
                i--;
                const int l = pl[i];
                if (l > m) { m = l; *at = i; }
            }
        }
    } else {
        for (int64_t i = a; i < b && m < top;) {
            if ((((uintptr_t)(pl + i)) & 7u) == 0 && i + 8 <= b) {
                const uint64_t wd = *reinterpret_cast<const uint64_t*>(pl + i);
#pragma unroll
                for (int k = 0; k < 8; k++) { const int l = (int)((wd >> (8 * k)) & 0xFFu); if (l > m) { m = l; *at = i + k; } }
                i += 8;
            } else {
                const int l = pl[i];
                if (l > m) { m = l; *at = i; }
                i++;
            }
        }
    }
    return m;
}

__global__ void __launch_bounds__(256) k_cp_count_short(JtkChunkPreferWork p) {
    const JtkChunkWork& w = p.w;
    const int64_t d = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (d == 0) w.hdr[1] = w.tok_off[w.n_docs];
    if (d >= w.n_docs) return;
    const int64_t t0 = w.tok_off[d], n = w.tok_off[d + 1] - t0;
    int64_t cnt = 0;
    if (w.status[d] >= 0 && n > 0) {
        if (cp_is_long(n, w.N)) {
            const unsigned long long i = atomicAdd((unsigned long long*)&w.hdr[2], 1ull);
            w.long_docs[i] = d;
        } else {
            const uint8_t* pl = p.plane + t0;
            const int top = jtk_cut_top_level(p.prefer);
            cnt = jtk_chunk_prefer_walk(n, w.N, w.overlap, p.min_tokens, [&](int64_t i) { return (int)pl[i]; },
                                        [&](int64_t a, int64_t b, bool last, int64_t* at) { return cp_scan(pl, a, b, last, at, top); },
                                        [](int64_t, int64_t, int64_t, bool, int) {});
        }
    }
    w.chunk_off[d] = cnt;
}

__global__ void __launch_bounds__(256) k_cp_write_short(JtkChunkPreferWork p) {
    const JtkChunkWork& w = p.w;
    const int64_t d = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= w.n_docs) return;
    const int64_t t0 = w.tok_off[d], n = w.tok_off[d + 1] - t0;
    if (w.status[d] < 0 || n == 0 || cp_is_long(n, w.N)) return;
    const uint8_t* pl = p.plane + t0;
    const int64_t c0 = w.chunk_off[d];
    const int top = jtk_cut_top_level(p.prefer);
    jtk_chunk_prefer_walk(n, w.N, w.overlap, p.min_tokens, [&](int64_t i) { return (int)pl[i]; },
                          [&](int64_t a, int64_t b, bool last, int64_t* at) { return cp_scan(pl, a, b, last, at, top); },
                          [&](int64_t k, int64_t s, int64_t e, bool split, int end_level) {
                              const int64_t c = c0 + k;
                              w.chunk_doc[c] = d; w.tok_begin[c] = t0 + s; w.n_tok_out[c] = (int32_t)(e - s); w.split[c] = split;
                              p.end_level[c] = (uint8_t)end_level;
                          });
}

// (max level, nearest cut) over the cuts pl[first + q * step], q in [0, cnt), by the whole workgroup: the result's bits 40..
// hold the level, the low bits CP_QMAX - q of the smallest q that has it; level 0: none found.  BND: only B matters (level
// != 0 counts as 1).  Stops after the round that has seen `top`.  All 256 lanes call it with the same arguments; it
// contains barriers, and the shuffles run in all lanes outside any branch.
template <bool BND>
__device__ __forceinline__ uint64_t cp_window(const uint8_t* pl, int64_t first, int64_t step, int64_t cnt, int top, uint64_t* s_red) {
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    uint64_t best = 0;
    for (int64_t q0 = 0; q0 < cnt; q0 += 256) {
        const int64_t q = q0 + tid;
        uint64_t key = 0;
        if (q < cnt) {
            uint32_t v = pl[first + q * step];
            if (BND) v = v != 0 ? 1u : 0u;
            key = ((uint64_t)v << 40) | (CP_QMAX - (uint64_t)q);
        }
#pragma unroll
        for (int dd = 32; dd >= 1; dd >>= 1) {
            const uint64_t o = __shfl_xor(key, dd);
            key = o > key ? o : key;
        }
        if (lane == 0) s_red[wv] = key;
        __syncthreads();
        const uint64_t a = s_red[0] > s_red[1] ? s_red[0] : s_red[1], b = s_red[2] > s_red[3] ? s_red[2] : s_red[3];
        const uint64_t r = a > b ? a : b;
        __syncthreads();                                                   // (s_red is rewritten next round)
        if (r > best) best = r;                                            // (an earlier round wins a tie: its q is smaller)
        if ((int)(best >> 40) >= top) break;                               // (the same in every lane)
    }
    return best;
}

// One workgroup per long document (persistent over the list).  All lanes run the loop in step: every value that decides it
// comes out of cp_window, the same in every lane.
template <bool WRITE>
__global__ void __launch_bounds__(256) k_cp_long(JtkChunkPreferWork p) {
    __shared__ uint64_t s_red[4];
    const JtkChunkWork& w = p.w;
    const int tid = threadIdx.x;
    const int64_t n_long = w.hdr[2];
    const int64_t N = w.N, ov = w.overlap, mt = p.min_tokens;
    const int top = jtk_cut_top_level(p.prefer);
    for (int64_t li = blockIdx.x; li < n_long; li += gridDim.x) {
        const int64_t d = w.long_docs[li];
        const int64_t t0 = w.tok_off[d], n = w.tok_off[d + 1] - t0;
        const uint8_t* pl = p.plane + t0;
        const int64_t c0 = WRITE ? w.chunk_off[d] : 0;
        int64_t s = 0, c = 0;
        for (;;) {
            const bool last = n - s <= N;
            int64_t e = n;
            if (!last) {
                const int64_t hi = s + N, lo = mt < N ? s + mt : hi;
                const uint64_t r = cp_window<false>(pl, hi, -1, hi - lo + 1, top, s_red);
                if ((r >> 40) >= 1) {
                    e = hi - (int64_t)(CP_QMAX - (r & CP_QMAX));
                } else {                                                   // the back-off of jtk_chunk_end: B below the window
                    const uint64_t r2 = cp_window<true>(pl, lo - 1, -1, lo - 1 - s, 1, s_red);
                    e = (r2 >> 40) ? lo - 1 - (int64_t)(CP_QMAX - (r2 & CP_QMAX)) : hi;
                }
            }
            if (WRITE && tid == 0) {
                const int64_t cc = c0 + c;
                w.chunk_doc[cc] = d; w.tok_begin[cc] = t0 + s; w.n_tok_out[cc] = (int32_t)(e - s);
                w.split[cc] = !((s == 0 || pl[s] != 0) && (last || pl[e] != 0));
                p.end_level[cc] = last ? (uint8_t)JTK_LEVEL_DOC_END : pl[e];
            }
            c++;
            if (last) break;
            const int64_t a = e - ov > s + 1 ? e - ov : s + 1;
            const uint64_t r = cp_window<false>(pl, a, 1, e - a, top, s_red);
            s = (r >> 40) >= 1 ? a + (int64_t)(CP_QMAX - (r & CP_QMAX)) : e;
        }
        if (!WRITE && tid == 0) w.chunk_off[d] = c;
    }
}

}  // namespace

void jtk_launch_cut_levels(const JtkChunkWork& w, const uint8_t* tab_blob, uint32_t prefer, uint8_t* plane, hipStream_t s) {
    hipLaunchKernelGGL(k_cp_levels, dim3(CP_PLANE_BLOCKS), dim3(256), 0, s, w, tab_blob, prefer, plane);
    hipLaunchKernelGGL(k_cp_doc_heads, dim3(jtk_blocks_for(w.n_docs, 256)), dim3(256), 0, s, w, tab_blob, prefer, plane);
}

void jtk_launch_chunk_prefer_count(const JtkChunkPreferWork& p, hipStream_t s) {
    hipLaunchKernelGGL(k_cp_count_short, dim3(jtk_blocks_for(p.w.n_docs, 256)), dim3(256), 0, s, p);
    hipLaunchKernelGGL(k_cp_long<false>, dim3(CP_LONG_BLOCKS), dim3(256), 0, s, p);
    jtk_launch_scan_i64(p.w.chunk_off, p.w.n_docs, &p.w.hdr[0], s);
}

void jtk_launch_chunk_prefer_write(const JtkChunkPreferWork& p, hipStream_t s) {
    if (p.w.n_chunks <= 0) return;
    hipLaunchKernelGGL(k_cp_write_short, dim3(jtk_blocks_for(p.w.n_docs, 256)), dim3(256), 0, s, p);
    hipLaunchKernelGGL(k_cp_long<true>, dim3(CP_LONG_BLOCKS), dim3(256), 0, s, p);
    jtk_launch_chunk_bytes(p.w, s);
}
