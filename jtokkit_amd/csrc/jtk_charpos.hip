// jtk_charpos.hip -- character positions of the batch text (jtk_batch_char_index / _char_positions / _byte_positions /
// _token_char_offsets in jtk_abi.cpp): a rank / select index over the text of the last encode and the query passes over it.  The
// rule, the layout of the index and the rank and select walks are jtk_charpos_rules.h (shared with tests/charpos_sim).
//
//   cp_build     one WAVE per superblock of 4096 bytes, four per workgroup: four coalesced 16-byte loads per lane (lane l of load
//                j holds bytes j * 1024 + l * 16 ..), the units of each by bit tricks on its four words and __popc, one wave scan
//                of the four counts packed into 16-bit fields -- no LDS, no barrier.  Every fourth lane stores a block's sub entry, lane 0 the superblock's total.
//   scan         sup = exclusive scan of the superblock totals (jtk_launch_scan_u32: one workgroup over n / 4096 items)
//   cp_dunit     dunit[d] = rank(doc_off[d]), d = 0 .. n_docs; doc_units[d] = dunit[d + 1] - dunit[d] on request
//   cp_rank      one lane per position: document (given or searched), snap, rank, minus dunit[d]
//   cp_select    one lane per (d, k): jtk_cp_byte_pos
//   cp_tokpos    tile form of k_ck_tokpos (2048 tokens, 8 per lane, jtk_tile_tok_prefix): FLOOR of every token's first byte and
//                CEIL of its end, straight from the tile's byte prefix; a token that begins where the one before it ended, on a
//                boundary, takes that token's end
#include "jtk_charpos_rules.h"
#include "jtk_device_prims.h"
#include "jtk_kernels.h"

namespace {

constexpr int CT = JTK_DEC_TILE;
static_assert(CT == 256 * 8, "a tile is 256 lanes x 8 tokens");
static_assert(JTK_CP_SUPER == 4 * 64 * 16 && JTK_CP_BLOCK == 4 * 16, "a wave covers a superblock in four loads; four lanes a block");

__global__ void __launch_bounds__(256) k_cp_build(const uint8_t* text, int64_t n_bytes, int64_t n_sup, int unit, uint32_t* sup_cnt,
                                                  uint16_t* sub) {
    const int lane = threadIdx.x & 63;
    const int64_t sb = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);      // (wave-uniform)
    const bool live = sb < n_sup;
    const int64_t base = sb * JTK_CP_SUPER;
    uint32_t c[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int64_t off = base + j * 1024 + lane * 16;
        c[j] = 0;
        if (live && off < n_bytes) c[j] = jtk_cp_quad_units(jtk_cp_load_quad(text, off), n_bytes - off, unit);
    }
    // one scan for the four loads: their counts in the 16-bit fields of one word (a granule has at most 32 units, a load's wave
    // sum at most 2048: no field carries into the next).  The shuffles: all 64 lanes, outside any condition.
    const uint64_t pk = (uint64_t)c[0] | (uint64_t)c[1] << 16 | (uint64_t)c[2] << 32 | (uint64_t)c[3] << 48;
    const uint64_t inc = jtk_wave_incl_scan(pk);
    const uint64_t tot = __shfl(inc, 63);
    uint32_t run = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const uint32_t before = (uint32_t)(inc >> (16 * j) & 0xFFFFu) - c[j];
        if (live && (lane & 3) == 0) sub[sb * JTK_CP_BLOCKS_PER_SUPER + j * 16 + (lane >> 2)] = (uint16_t)(run + before);
        run += (uint32_t)(tot >> (16 * j) & 0xFFFFu);
    }
    if (live && lane == 0) sup_cnt[sb] = run;
}

struct CpDocs {
    const int64_t* doc_off;     // [n_docs + 1]
    const int64_t* dunit;       // [n_docs + 1]
    int64_t n_docs;
};

__global__ void __launch_bounds__(256) k_cp_dunit(JtkCharIndex ix, const int64_t* doc_off, int64_t n_docs, int64_t* dunit) {
    const int64_t d = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (d > n_docs) return;
    dunit[d] = jtk_cp_rank(ix, jtk_cp_clamp(doc_off[d], ix.n_bytes));
}

__global__ void __launch_bounds__(256) k_cp_doc_units(CpDocs dc, int64_t* doc_units) {
    const int64_t d = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= dc.n_docs) return;
    const int64_t u = dc.dunit[d + 1] - dc.dunit[d];
    doc_units[d] = u < 0 ? 0 : u;
}

__global__ void __launch_bounds__(256) k_cp_rank(JtkCharIndex ix, CpDocs dc, int round, const int64_t* doc, const int64_t* byte_pos,
                                                 int64_t n, int64_t* char_pos) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t p = byte_pos[i];
    const int64_t d = doc ? doc[i] : jtk_cp_doc_of(dc.doc_off, dc.n_docs, ix.n_bytes, p);
    char_pos[i] = jtk_cp_char_index(ix, dc.doc_off, dc.dunit, dc.n_docs, d, p, round);
}

__global__ void __launch_bounds__(256) k_cp_select(JtkCharIndex ix, CpDocs dc, const int64_t* doc, const int64_t* char_pos, int64_t n,
                                                   int64_t* byte_pos) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    byte_pos[i] = jtk_cp_byte_pos(ix, dc.doc_off, dc.dunit, dc.n_docs, doc[i], char_pos[i]);
}

// (as ck_doc_of of jtk_chunk.hip)
__device__ __forceinline__ int64_t cp_doc_of_tok(const JtkChunkWork& w, int64_t t) { return jtk_first_gt(w.tok_off, 1, w.n_docs, t) - 1; }

__global__ void __launch_bounds__(256) k_cp_tokpos(JtkChunkWork w, JtkCharIndex ix, const int64_t* dunit, int64_t* begin, int64_t* end) {
    const int64_t t0 = (int64_t)blockIdx.x * CT + threadIdx.x * 8;
    uint32_t len[8];
    const uint32_t pre = jtk_tile_tok_prefix(w.tokens, w.n_tok, t0, w.tab_off, w.n_ids_table, 1u, len);
    if (t0 >= w.n_tok) return;                                            // (behind the prefix: it holds a barrier)
    int64_t pos = w.tile_off[blockIdx.x] + pre;
    int64_t d = -1, a = 0, e = 0, base = 0, du = 0;
    int64_t carry_pos = -1, carry_val = 0;                                // the previous token's end, when it is a boundary of d
    for (int j = 0; j < 8 && t0 + j < w.n_tok; j++) {
        const int64_t t = t0 + j;
        if (d < 0 || w.tok_off[d + 1] <= t) {
            d = cp_doc_of_tok(w, t);
            jtk_cp_doc_range(w.doc_off, d, ix.n_bytes, &a, &e);
            base = w.dbase[d];
            du = dunit[d];
            carry_pos = -1;
        }
        const int64_t p = base + pos, q = p + len[j];
        pos += len[j];
        int64_t vb = -1, ve = -1;
        if (p >= a && q <= e) {                                           // (a position outside its document touches no memory)
            vb = p == carry_pos ? carry_val : jtk_cp_rank(ix, jtk_cp_snap(ix.text, a, e, p, JTK_CP_FLOOR)) - du;
            const int64_t qs = jtk_cp_snap(ix.text, a, e, q, JTK_CP_CEIL);
            ve = jtk_cp_rank(ix, qs) - du;
            carry_pos = (qs == q && jtk_cp_is_boundary(ix.text, a, e, q)) ? q : -1;
            carry_val = ve;
        } else {
            carry_pos = -1;
        }
        begin[t] = vb;
        if (end) end[t] = ve;
    }
}

}  // namespace

void jtk_launch_charpos_build(const JtkCharIndex& ix, uint32_t* sup_cnt, int64_t* sup, uint16_t* sub, const int64_t* doc_off,
                              int64_t n_docs, int64_t* dunit, hipStream_t s) {
    if (ix.n_sup > 0)
        hipLaunchKernelGGL(k_cp_build, dim3(jtk_blocks_for(ix.n_sup, 4)), dim3(256), 0, s, ix.text, ix.n_bytes, ix.n_sup, ix.unit, sup_cnt, sub);
    jtk_launch_scan_u32(sup_cnt, ix.n_sup, sup, nullptr, s);
    hipLaunchKernelGGL(k_cp_dunit, dim3(jtk_blocks_for(n_docs + 1, 256)), dim3(256), 0, s, ix, doc_off, n_docs, dunit);
}

void jtk_launch_charpos_doc_units(const int64_t* doc_off, const int64_t* dunit, int64_t n_docs, int64_t* doc_units, hipStream_t s) {
    if (n_docs <= 0) return;
    const CpDocs dc{doc_off, dunit, n_docs};
    hipLaunchKernelGGL(k_cp_doc_units, dim3(jtk_blocks_for(n_docs, 256)), dim3(256), 0, s, dc, doc_units);
}

void jtk_launch_charpos_rank(const JtkCharIndex& ix, const int64_t* doc_off, const int64_t* dunit, int64_t n_docs, int round,
                             const int64_t* doc, const int64_t* byte_pos, int64_t n, int64_t* char_pos, hipStream_t s) {
    if (n <= 0) return;
    const CpDocs dc{doc_off, dunit, n_docs};
    hipLaunchKernelGGL(k_cp_rank, dim3(jtk_blocks_for(n, 256)), dim3(256), 0, s, ix, dc, round, doc, byte_pos, n, char_pos);
}

void jtk_launch_charpos_select(const JtkCharIndex& ix, const int64_t* doc_off, const int64_t* dunit, int64_t n_docs, const int64_t* doc,
                               const int64_t* char_pos, int64_t n, int64_t* byte_pos, hipStream_t s) {
    if (n <= 0) return;
    const CpDocs dc{doc_off, dunit, n_docs};
    hipLaunchKernelGGL(k_cp_select, dim3(jtk_blocks_for(n, 256)), dim3(256), 0, s, ix, dc, doc, char_pos, n, byte_pos);
}

void jtk_launch_charpos_tokens(const JtkChunkWork& w, const JtkCharIndex& ix, const int64_t* dunit, int64_t* begin, int64_t* end,
                               hipStream_t s) {
    if (w.n_tok > 0) hipLaunchKernelGGL(k_cp_tokpos, dim3((unsigned)w.n_tiles), dim3(256), 0, s, w, ix, dunit, begin, end);
}
