// jtk_decode.hip -- batch decode on the device: Encoding.decodeBytes(List<Integer>)
// (GptBytePairEncoding.java:137-151: for every token id, append its byte string; unknown id ->
// IllegalArgumentException, :302-314 incl. special tokens :308-311) for many token lists at once.
//
//   dec_mark     one bit per sequence start (token index), like mark_docs
//   dec_count    bytes per tile of 2048 tokens (lengths from the offset table); unknown ids -> status of their sequence
//   scan         exclusive scan of the tile sizes (the one-workgroup scan, jtk_launch_scan_u32; tiles are few)
//   dec_scatter  per tile: byte offset of every token (block scan), the tile's bytes assembled in LDS and
//                written in aligned 4-byte words; leaves the byte offset at sequence starts
//   dec_offsets  byte_off[q] per sequence
// Integer / byte gather work; bound by the random reads of the token byte strings (L2-resident blob).
#include "jtk_device_prims.h"
#include "jtk_kernels.h"
#include "jtk_maxtok_rules.h"

namespace {

constexpr int DT = JTK_DEC_TILE;           // tokens per tile
constexpr int DSTAGE = 16384;              // bytes of a tile assembled in LDS (ordinary text: ~7 KB)

__global__ void __launch_bounds__(256) k_dec_mark(JtkDecodeWork w) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q > w.n_seqs) return;
    const int64_t p = w.seq_off[q];
    if (p < 0 || p > w.n_tok) return;
    atomicOr((unsigned long long*)&w.seqmask[p >> 6], 1ull << (p & 63));
}

__global__ void __launch_bounds__(256) k_dec_count(JtkDecodeWork w) {
    const int64_t t0 = (int64_t)blockIdx.x * DT + threadIdx.x * 8;
    uint32_t sum = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const int64_t t = t0 + j;
        if (t < w.n_tok) {
            const uint32_t l = jtk_tok_len(w.tab_off, w.n_ids_table, w.ids[t], 0u);
            if (l == 0) {                                              // GptBytePairEncoding.java:313
                // the sequence that holds token t: the one before the first whose start is past t (none: t is before all)
                const int64_t q = jtk_first_gt(w.seq_off, 0, w.n_seqs, t) - 1;
                if (q >= 0) atomicMin(&w.status[q], -3 /* JTK_ERR_UNKNOWN_TOKEN */);
            }
            sum += l;
        }
    }
    uint32_t total;
    (void)jtk_block_excl_prefix<256>(sum, &total);
    if (threadIdx.x == 0) w.tile_bytes[blockIdx.x] = total;
}

__global__ void __launch_bounds__(256) k_dec_scatter(JtkDecodeWork w) {
    __shared__ __attribute__((aligned(16))) uint8_t s_out[DSTAGE + 8];
    const int tid = threadIdx.x;
    const int64_t tile = blockIdx.x;
    const int64_t t0 = tile * DT + tid * 8;
    const int64_t obase = w.tile_off[tile];
    const uint32_t total = w.tile_bytes[tile];
    const bool stage = total <= (uint32_t)DSTAGE && w.out != nullptr;
    int32_t id[8];
    uint32_t len[8];
    uint32_t pre = jtk_tile_tok_prefix(w.ids, w.n_tok, t0, w.tab_off, w.n_ids_table, 0u, len, nullptr, id);
    const uint64_t mword = w.seqmask[t0 >> 6];                        // (t0 is a multiple of 8: one word covers the 8 tokens)
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const int64_t t = t0 + j;
        if (t < w.n_tok && ((mword >> (t & 63)) & 1ull)) w.seqpre[t] = pre;
        if (len[j] && w.out != nullptr) {
            const uint8_t* src = w.tab_blob + w.tab_off[id[j]];
            if (stage) for (uint32_t i = 0; i < len[j]; i++) s_out[pre + i] = src[i];
            else for (uint32_t i = 0; i < len[j]; i++) w.out[obase + pre + i] = src[i];
        }
        pre += len[j];
    }
    if (!stage) return;
    __syncthreads();
    // aligned 4-byte words of the output that the tile's bytes [obase, obase + total) touch
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

__global__ void __launch_bounds__(256) k_dec_offsets(JtkDecodeWork w) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q > w.n_seqs) return;
    const int64_t p = w.seq_off[q];
    w.byte_off[q] = (p >= w.n_tok) ? w.tile_off[w.n_tiles] : w.tile_off[p / DT] + w.seqpre[p];
    if (q < w.n_seqs) {
        const int32_t st = w.status[q];
        if (st < 0) atomicMin(w.worst_status, st);
    }
}

// ---------------------------------------------------------------------------------------------------
// truncate: Encoding.encode(text, maxTokens) for every document of the last batch encode
// (GptBytePairEncoding.java:43-45, 79, 90-100, 110-119).  Pieces encode independently, so the list before
// the back-off is the first min(maxTokens, total) tokens of the full result; the back-off (:90-100) drops
// trailing tokens until decode(tokens) is a prefix of the text, i.e. until their bytes end on a code-point
// boundary -- or in the middle of a U+FFFD of the text, which new String(bytes, UTF_8) turns into the
// same U+FFFD.  truncated (:97) = text.length() > decoded.length().  One thread per document.
// ---------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_truncate(JtkTruncWork w) {
    const int64_t d = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= w.n_docs) return;
    const int64_t t0 = w.tok_off[d], cnt = w.tok_off[d + 1] - t0;
    int64_t keep = cnt < w.max_tokens ? cnt : w.max_tokens;
    uint8_t trunc = 0;
    if (cnt > w.max_tokens) {
        const uint8_t* tx = w.text + w.doc_off[d];
        const int64_t len = w.doc_off[d + 1] - w.doc_off[d];
        int64_t nb = 0;
        for (int64_t k = 0; k < keep; k++) { const int32_t id = w.tokens[t0 + k]; nb += w.tab_off[id + 1] - w.tab_off[id]; }
        const JtkBackoff r = jtk_maxtok_backoff(tx, len, keep, nb, [&](int64_t k) {
            const int32_t id = w.tokens[t0 + k];
            return (int64_t)(w.tab_off[id + 1] - w.tab_off[id]);
        });
        keep = r.keep;
        trunc = r.ok && (r.units == 0 ? r.from < len : r.from + 3 < len);
    }
    w.kept[d] = keep;
    w.truncated[d] = trunc;
}

}  // namespace

void jtk_launch_truncate(const JtkTruncWork& w, hipStream_t s) {
    if (w.n_docs > 0) hipLaunchKernelGGL(k_truncate, dim3((unsigned)((w.n_docs + 255) / 256)), dim3(256), 0, s, w);
}

void jtk_launch_decode_count(const JtkDecodeWork& w, hipStream_t s) {
    const int64_t n = w.n_seqs + 1;
    hipLaunchKernelGGL(k_dec_mark, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, w);
    hipLaunchKernelGGL(k_dec_count, dim3((unsigned)w.n_tiles), dim3(256), 0, s, w);
    jtk_launch_scan_u32(w.tile_bytes, w.n_tiles, w.tile_off, w.total, s);
}
void jtk_launch_decode_scatter(const JtkDecodeWork& w, hipStream_t s) {
    const int64_t n = w.n_seqs + 1;
    hipLaunchKernelGGL(k_dec_scatter, dim3((unsigned)w.n_tiles), dim3(256), 0, s, w);
    hipLaunchKernelGGL(k_dec_offsets, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, w);
}
