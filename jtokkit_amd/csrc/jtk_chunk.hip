// jtk_chunk.hip -- token-budget chunking of the last batch encode (jtk_batch_chunk in jtk_abi.cpp): every document with
// status OK cut into chunks of at most N tokens by the rule of jtk_chunk_rules.h, with the byte span of every chunk, rows
// [n_chunks, N] for a model and, on request, the byte position of every token ("offset mapping").
//
//   ck_count_short   one lane per document with few chunks: the header's walk, counting; documents with many chunks are
//                    listed for ...
//   ck_long          ... one workgroup each: 256 lanes guess the next 256 ends s + N, s + 2N, ... (with overlap: stride
//                    N - overlap), check B at each, and take the leading run of hits; the first miss goes through the
//                    header's back-off on one lane.  Equal to the walk cut for cut.  Same kernel counts and writes.
//   scan             exclusive scan of the per-document counts (one workgroup) -> chunk_off, and the totals for the host
//   ck_tiles         per tile of 2048 tokens: byte sum (-> tile_bytes) and, per group of 16 tokens, the tile's bytes before
//                    it (sub16): the segmented scan of token byte lengths, as k_dec_count / k_dec_scatter do
//   scan             tile_off = exclusive scan of tile_bytes
//   ck_dbase         per document: doc_off[d] - G(tok_off[d])
//   ck_write_short   the records of the short documents (the walk again, writing)
//   ck_bytes         per chunk: byte_begin / byte_end from G at its two ends
//   ck_rows          the ids of every chunk, then pad_id: [n_chunks, N] int32, coalesced along the row
//   ck_tokpos        byte position of every token (tile scan + document base)
// G(t) = bytes of the batch's tokens before token t = tile_off[t / 2048] + sub16[t / 16] + the lengths of < 16 tokens.
#include "jtk_chunk_rules.h"
#include "jtk_device_prims.h"
#include "jtk_kernels.h"

namespace {

constexpr int CT = JTK_DEC_TILE;               // tokens per tile
constexpr int CK_LONG_CHUNKS = 32;             // documents with more chunks than this get a workgroup
constexpr int CK_LONG_BLOCKS = 2048;           // persistent workgroups over the long documents
static_assert(CT == 256 * 8 && CT % 16 == 0, "a tile is 256 lanes x 8 tokens");

__device__ __forceinline__ bool ck_bnd(const JtkChunkWork& w, int32_t id) {
    return (uint32_t)id >= w.n_ids_table || ((w.bnd[(uint32_t)id >> 5] >> ((uint32_t)id & 31)) & 1u);
}

__device__ __forceinline__ bool ck_is_long(int64_t n, int64_t N, int64_t ov) {
    if (n <= N) return false;
    const int64_t stride = N - ov;
    return (n - N + stride - 1) / stride >= CK_LONG_CHUNKS;
}

// G(x) for 0 <= x <= n_tok
__device__ __forceinline__ int64_t ck_G(const JtkChunkWork& w, int64_t x) {
    if (x >= w.n_tok) return w.tile_off[w.n_tiles];
    int64_t v = w.tile_off[x / CT] + w.sub16[x >> 4];
    for (int64_t y = x & ~(int64_t)15; y < x; y++) v += jtk_tok_len(w.tab_off, w.n_ids_table, w.tokens[y], 1u);
    return v;
}

__global__ void __launch_bounds__(256) k_ck_count_short(JtkChunkWork w) {
    const int64_t d = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= w.n_docs) return;
    const int64_t t0 = w.tok_off[d], n = w.tok_off[d + 1] - t0;
    int64_t cnt = 0;
    if (w.status[d] >= 0 && n > 0) {
        if (ck_is_long(n, w.N, w.overlap)) {
            const unsigned long long i = atomicAdd((unsigned long long*)&w.hdr[2], 1ull);
            w.long_docs[i] = d;
        } else {
            const int32_t* tk = w.tokens + t0;
            cnt = jtk_chunk_walk(n, w.N, w.overlap, [&](int64_t i) { return ck_bnd(w, tk[i]); },
                                 [](int64_t, int64_t, int64_t, bool) {});
        }
    }
    w.chunk_off[d] = cnt;
}

__global__ void __launch_bounds__(256) k_ck_write_short(JtkChunkWork w) {
    const int64_t d = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= w.n_docs) return;
    const int64_t t0 = w.tok_off[d], n = w.tok_off[d + 1] - t0;
    if (w.status[d] < 0 || n == 0 || ck_is_long(n, w.N, w.overlap)) return;
    const int32_t* tk = w.tokens + t0;
    const int64_t c0 = w.chunk_off[d];
    jtk_chunk_walk(n, w.N, w.overlap, [&](int64_t i) { return ck_bnd(w, tk[i]); },
                   [&](int64_t k, int64_t s, int64_t e, bool split) {
                       const int64_t c = c0 + k;
                       w.chunk_doc[c] = d; w.tok_begin[c] = t0 + s; w.n_tok_out[c] = (int32_t)(e - s); w.split[c] = split;
                   });
}

// One workgroup per document with many chunks (persistent over the list).  All lanes run the loop in step: every value that
// decides it comes from LDS after a barrier.
template <bool WRITE>
__global__ void __launch_bounds__(256) k_ck_long(JtkChunkWork w) {
    __shared__ int s_miss[4];
    __shared__ int64_t s_next;
    __shared__ int s_done;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t n_long = w.hdr[2];
    const int64_t N = w.N, ov = w.overlap, stride = N - ov;
    for (int64_t li = blockIdx.x; li < n_long; li += gridDim.x) {
        const int64_t d = w.long_docs[li];
        const int64_t t0 = w.tok_off[d], n = w.tok_off[d + 1] - t0;
        const int32_t* tk = w.tokens + t0;
        auto bnd = [&](int64_t i) { return ck_bnd(w, tk[i]); };
        const int64_t c0 = WRITE ? w.chunk_off[d] : 0;
        int64_t s = 0, c = 0;
        for (;;) {
            // guess k: the chunk [s_k, s_k + N) with s_k = s + k * stride; the chain goes on past it on the grid when its end
            // is inside the document and both the end and the next start are boundaries
            const int64_t sk = s + (int64_t)tid * stride;
            const int64_t ek = (n - sk < N) ? n : sk + N;
            const bool cont = ek < n && bnd(ek) && (ov == 0 || bnd(ek - ov));
            const uint64_t miss = __ballot(!cont);                         // (all lanes, outside any branch)
            if (lane == 0) s_miss[wv] = miss ? wv * 64 + __ffsll((unsigned long long)miss) - 1 : 256;
            __syncthreads();
            const int m = min(min(s_miss[0], s_miss[1]), min(s_miss[2], s_miss[3]));
            if (WRITE && tid < m) {
                const int64_t cc = c0 + c + tid;
                w.chunk_doc[cc] = d; w.tok_begin[cc] = t0 + sk; w.n_tok_out[cc] = (int32_t)N;
                w.split[cc] = jtk_chunk_split(sk, ek, n, bnd);
            }
            c += m;
            if (m == 256) {
                s += 256 * stride;
                __syncthreads();                                           // (s_miss is rewritten next round)
                continue;
            }
            if (tid == 0) {                                                // the miss: the header's rule
                const int64_t sm = s + (int64_t)m * stride;
                const int64_t e = jtk_chunk_end(sm, n, N, bnd);
                if (WRITE) {
                    const int64_t cc = c0 + c;
                    w.chunk_doc[cc] = d; w.tok_begin[cc] = t0 + sm; w.n_tok_out[cc] = (int32_t)(e - sm);
                    w.split[cc] = jtk_chunk_split(sm, e, n, bnd);
                }
                s_done = e == n;
                s_next = e == n ? n : jtk_chunk_next_start(sm, e, ov, n, bnd);
            }
            __syncthreads();
            c += 1;
            const bool done = s_done != 0;
            s = s_next;
            __syncthreads();
            if (done) break;
        }
        if (!WRITE && tid == 0) w.chunk_off[d] = c;
    }
}

// Exclusive scan of in[0, n) into out[0, n] (in may be out), out[n] = the sum, and *total (may be NULL); one workgroup
// (jtk_block_scan_array).  hdr != NULL: the chunk count's epilogue, hdr[1] = tok_off[n_docs].
template <class T>
__global__ void __launch_bounds__(1024) k_ck_scan(const T* in, int64_t n, int64_t* out, int64_t* total, const int64_t* tok_off,
                                                  int64_t n_docs, int64_t* hdr) {
    const int64_t sum = (int64_t)jtk_block_scan_array(n, [&](int64_t i) { return in[i]; },
                                                      [&](int64_t i, uint64_t v) { out[i] = (int64_t)v; });
    if (threadIdx.x == 0) {
        out[n] = sum;
        if (total) *total = sum;
        if (hdr) hdr[1] = tok_off[n_docs];
    }
}

__global__ void __launch_bounds__(256) k_ck_tiles(JtkChunkWork w) {
    const int tid = threadIdx.x;
    const int64_t t0 = (int64_t)blockIdx.x * CT + tid * 8;
    uint32_t len[8], tile_bytes;
    const uint32_t pre = jtk_tile_tok_prefix(w.tokens, w.n_tok, t0, w.tab_off, w.n_ids_table, 1u, len, &tile_bytes);
    if ((tid & 1) == 0 && t0 < w.n_tok) w.sub16[t0 >> 4] = pre;           // (t0 of an even lane is a multiple of 16)
    if (tid == 0) w.tile_bytes[blockIdx.x] = tile_bytes;
}

__global__ void __launch_bounds__(256) k_ck_dbase(JtkChunkWork w) {
    const int64_t d = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= w.n_docs) return;
    w.dbase[d] = w.doc_off[d] - ck_G(w, w.tok_off[d]);
}

__global__ void __launch_bounds__(256) k_ck_bytes(JtkChunkWork w) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= w.n_chunks) return;
    const int64_t base = w.dbase[w.chunk_doc[c]], s = w.tok_begin[c], e = s + w.n_tok_out[c];
    w.byte_begin[c] = base + ck_G(w, s);
    w.byte_end[c] = base + ck_G(w, e);
}

// rows[c * N + col] = tokens[tok_begin[c] + col] for col < n_tok[c], else pad_id: 4 consecutive cells per lane
__global__ void __launch_bounds__(256) k_ck_rows(JtkChunkWork w, int32_t pad_id, int32_t* rows, int64_t total) {
    const int64_t blk0 = (int64_t)blockIdx.x * 1024;
    const int64_t e0 = blk0 + threadIdx.x * 4;
    if (e0 >= total) return;
    const int64_t N = w.N;
    const int64_t r0 = blk0 / N;                                         // (the same for the whole block)
    const int64_t rel = e0 - r0 * N;
    int64_t row = r0 + rel / N, col = rel % N;
    int64_t tb = w.tok_begin[row];
    int32_t nt = w.n_tok_out[row];
    int32_t v[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        if (col >= N) {
            do { col -= N; row++; } while (col >= N);
            if (row < w.n_chunks) { tb = w.tok_begin[row]; nt = w.n_tok_out[row]; }
        }
        v[j] = (e0 + j < total && col < nt) ? w.tokens[tb + col] : pad_id;
        col++;
    }
    int32_t* dst = rows + e0;
    if (e0 + 4 <= total && ((uintptr_t)dst & 15u) == 0) {
        *reinterpret_cast<int4*>(dst) = make_int4(v[0], v[1], v[2], v[3]);
    } else {
        for (int j = 0; j < 4; j++) if (e0 + j < total) dst[j] = v[j];
    }
}

// the document that holds token t: the last d in [0, n_docs) with tok_off[d] <= t (tok_off[0] <= t; the empty documents
// before it share its offset and are passed over)
__device__ __forceinline__ int64_t ck_doc_of(const JtkChunkWork& w, int64_t t) {
    return jtk_first_gt(w.tok_off, 1, w.n_docs, t) - 1;
}

__global__ void __launch_bounds__(256) k_ck_tokpos(JtkChunkWork w, int64_t* byte_pos) {
    const int64_t t0 = (int64_t)blockIdx.x * CT + threadIdx.x * 8;
    uint32_t len[8];
    const uint32_t pre = jtk_tile_tok_prefix(w.tokens, w.n_tok, t0, w.tab_off, w.n_ids_table, 1u, len);
    if (t0 >= w.n_tok) return;                                            // (behind the prefix: it holds a barrier)
    int64_t pos = w.tile_off[blockIdx.x] + pre;
    int64_t d = ck_doc_of(w, t0);
    for (int j = 0; j < 8 && t0 + j < w.n_tok; j++) {
        const int64_t t = t0 + j;
        if (w.tok_off[d + 1] <= t) d = ck_doc_of(w, t);
        byte_pos[t] = w.dbase[d] + pos;
        pos += len[j];
    }
}

}  // namespace

void jtk_launch_chunk_count(const JtkChunkWork& w, hipStream_t s) {
    hipLaunchKernelGGL(k_ck_count_short, dim3(jtk_blocks_for(w.n_docs, 256)), dim3(256), 0, s, w);
    hipLaunchKernelGGL(k_ck_long<false>, dim3(CK_LONG_BLOCKS), dim3(256), 0, s, w);
    hipLaunchKernelGGL(k_ck_scan<int64_t>, dim3(1), dim3(1024), 0, s, (const int64_t*)w.chunk_off, w.n_docs, w.chunk_off, &w.hdr[0],
                       w.tok_off, w.n_docs, w.hdr);
}

void jtk_launch_chunk_tiles(const JtkChunkWork& w, hipStream_t s) {
    if (w.n_tok > 0) hipLaunchKernelGGL(k_ck_tiles, dim3((unsigned)w.n_tiles), dim3(256), 0, s, w);
    jtk_launch_scan_u32(w.tile_bytes, w.n_tok > 0 ? w.n_tiles : (int64_t)0, w.tile_off, nullptr, s);
    if (w.n_docs > 0) hipLaunchKernelGGL(k_ck_dbase, dim3(jtk_blocks_for(w.n_docs, 256)), dim3(256), 0, s, w);
}

void jtk_launch_chunk_write(const JtkChunkWork& w, hipStream_t s) {
    if (w.n_chunks <= 0) return;
    hipLaunchKernelGGL(k_ck_write_short, dim3(jtk_blocks_for(w.n_docs, 256)), dim3(256), 0, s, w);
    hipLaunchKernelGGL(k_ck_long<true>, dim3(CK_LONG_BLOCKS), dim3(256), 0, s, w);
    hipLaunchKernelGGL(k_ck_bytes, dim3(jtk_blocks_for(w.n_chunks, 256)), dim3(256), 0, s, w);
}

void jtk_launch_chunk_bytes(const JtkChunkWork& w, hipStream_t s) {
    if (w.n_chunks > 0) hipLaunchKernelGGL(k_ck_bytes, dim3(jtk_blocks_for(w.n_chunks, 256)), dim3(256), 0, s, w);
}

void jtk_launch_chunk_rows(const JtkChunkWork& w, int32_t pad_id, int32_t* rows, hipStream_t s) {
    const int64_t total = w.n_chunks * w.N;
    if (total > 0) hipLaunchKernelGGL(k_ck_rows, dim3(jtk_blocks_for(total, 1024)), dim3(256), 0, s, w, pad_id, rows, total);
}

void jtk_launch_token_offsets(const JtkChunkWork& w, int64_t* byte_pos, hipStream_t s) {
    if (w.n_tok > 0) hipLaunchKernelGGL(k_ck_tokpos, dim3((unsigned)w.n_tiles), dim3(256), 0, s, w, byte_pos);
}

void jtk_launch_scan_i64(int64_t* inout, int64_t n, int64_t* total, hipStream_t s) {
    hipLaunchKernelGGL(k_ck_scan<int64_t>, dim3(1), dim3(1024), 0, s, (const int64_t*)inout, n, inout, total, (const int64_t*)nullptr,
                       (int64_t)0, (int64_t*)nullptr);
}
void jtk_launch_scan_u32(const uint32_t* in, int64_t n, int64_t* out, int64_t* total, hipStream_t s) {
    hipLaunchKernelGGL(k_ck_scan<uint32_t>, dim3(1), dim3(1024), 0, s, in, n, out, total, (const int64_t*)nullptr, (int64_t)0,
                       (int64_t*)nullptr);
}
