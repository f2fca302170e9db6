// jtk_special.hip -- allow-special encode (JTK_ENCODE_ALLOW_SPECIAL, orchestrated by jtk_abi.cpp): allowed special-token
// literals become their ids, the text between them is encoded as encodeOrdinary() of each segment.  The rule is
// jtk_special_rules.h; the four-kernel encode pipeline itself is untouched and runs on the sub-documents.
//
//   sp_check     one lane per offset: doc_off non-decreasing within [0, n_bytes], doc_off[0] == 0 -> hdr[1]
//   sp_find      one lane per 16 bytes (a workgroup per JTK_SPECIAL_BLOCK): candidate bytes from the first-byte bitmap, a
//                ballot skips the waves without one; per candidate the longest allowed literal that ends inside its document,
//                and (encode()) whether a literal outside the allowed set matches there (atomicMin of the document's status)
//   scan         exclusive scan of the per-workgroup counts (jtk_launch_scan_i64) -> hdr[0] = candidates, read by the host
//   sp_find      again, writing the candidates in position order (workgroup base + lane scan)
//   sp_resolve   one lane per candidate: kept for certain, or part of a chain
//   sp_walk      one lane per chain: the greedy walk from the certain candidate before it
//   sp_docs      one lane per document: its first sub-document (a segment)
//   sp_subs      one lane per candidate: its two sub-documents (literal, segment after it; empty when not kept)
//   ... the encode pipeline on the sub-documents (encodeOrdinary), then the stitch:
//   sp_status    one lane per sub-document: segment statuses (and a literal's JTK_ERR_BAD_UTF8) into the document's status
//   sp_count     one lane per sub-document: its tokens in the result (1 for a kept literal, 0 in a refused document)
//   scan         exclusive scan of the counts
//   sp_offsets   one lane per document: tok_off, worst status, token total
//   sp_gather    16 output tokens per lane: segment ids copied, special ids written
#include "jtk_device_prims.h"
#include "jtk_kernels.h"
#include "jtk_special_rules.h"

namespace {

constexpr int FT = 256;                    // find: lanes per workgroup, 16 bytes each
static_assert(FT * 16 == JTK_SPECIAL_BLOCK, "a find workgroup covers JTK_SPECIAL_BLOCK bytes");
constexpr int GT = 256, GPER = 16;         // gather: lanes per workgroup, output tokens per lane
constexpr int GATHER_BLOCKS_MAX = 65536;

// the document that holds byte p (empty documents skipped); clamped to a valid index, so that bad offsets are never followed
// out of range (the call then discards the find pass)
__device__ __forceinline__ int64_t sp_find_doc(const JtkSpecialWork& w, int64_t p) {
    int64_t d = jtk_first_gt(w.doc_off, 0, w.n_docs + 1, p) - 1;      // the one before the first k with doc_off[k] > p
    if (d < 0) d = 0;
    if (d > w.n_docs - 1) d = w.n_docs - 1;
    return d;
}

__global__ void __launch_bounds__(256) k_sp_check(JtkSpecialWork w) {
    const int64_t d = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (d > w.n_docs) return;
    const int64_t q = w.doc_off[d];
    const bool bad = q < 0 || q > w.n_bytes || (d > 0 && w.doc_off[d - 1] > q) || (d == 0 && q != 0) || (d == w.n_docs && q != w.n_bytes);
    if (bad) atomicMax((unsigned long long*)&w.hdr[1], 1ull);
}

// One candidate position: the longest allowed literal at p that ends inside its document (*len, *lit; 0 / -1: none), its
// document, and whether a literal outside the allowed set matches there.  The first look is bounded by the batch's end only,
// so that the document is looked up only where some literal matches.
__device__ __forceinline__ bool sp_at(const JtkSpecialWork& w, int64_t p, int* len, int* lit, int64_t* doc) {
    auto at = [&](int64_t q) -> uint32_t { return w.text[q]; };
    bool dis = jtk_special_scan_at(p, w.n_bytes, at, w.n_lits, w.lit_off, w.lit_blob, w.allowed, len, lit);
    *doc = -1;
    if (*len == 0 && !(dis && w.check_dis)) return false;
    const int64_t d = sp_find_doc(w, p);
    const int64_t end = w.doc_off[d + 1] < w.n_bytes ? w.doc_off[d + 1] : w.n_bytes;
    dis = jtk_special_scan_at(p, end, at, w.n_lits, w.lit_off, w.lit_blob, w.allowed, len, lit);
    *doc = d;
    return dis && w.check_dis;
}

template <bool WRITE>
__global__ void __launch_bounds__(FT) k_sp_find(JtkSpecialWork w) {
    __shared__ uint32_t s_first[8];
    const int tid = threadIdx.x;
    if (tid < 8) s_first[tid] = w.first[tid];
    __syncthreads();
    const int64_t p0 = (int64_t)blockIdx.x * JTK_SPECIAL_BLOCK + (int64_t)tid * 16;
    uint32_t cand = 0;                     // bit j: byte p0 + j starts some literal the pass looks for
    if (p0 < w.n_bytes) {
        const uint4 v = *reinterpret_cast<const uint4*>(w.text + p0);     // (readable up to the next multiple of 16)
        const uint32_t d4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 16; j++) {
            const uint32_t b = (d4[j >> 2] >> (8 * (j & 3))) & 0xFFu;
            cand |= ((s_first[b >> 5] >> (b & 31)) & 1u) << j;
        }
        const int64_t left = w.n_bytes - p0;
        if (left < 16) cand &= (1u << left) - 1u;
    }
    uint32_t found = 0, n_here = 0;        // bit j: a candidate (an allowed literal ends inside the document) at p0 + j
    int first_j = -1, first_len = 0, first_lit = -1;
    int64_t first_doc = 0;
    if (__ballot(cand != 0) != 0ull) {     // (most waves of ordinary text hold no byte that starts a literal)
        for (uint32_t m = cand; m;) {
            const int j = __builtin_ctz(m);
            m &= m - 1;
            int len, lit;
            int64_t d;
            const bool dis = sp_at(w, p0 + j, &len, &lit, &d);
            if (!WRITE && dis) {
                atomicMin(&w.status[d], -2 /* JTK_ERR_UNSUPPORTED_SPECIAL */);
                atomicMax((unsigned long long*)&w.hdr[2], 1ull);
            }
            if (len > 0) {
                if (first_j < 0) { first_j = j; first_len = len; first_lit = lit; first_doc = d; }
                found |= 1u << j;
                n_here++;
            }
        }
    }
    uint32_t n_blk_here;
    const uint32_t pre = jtk_block_excl_prefix<FT>(n_here, &n_blk_here);
    if (!WRITE) {
        if (tid == 0) w.blk[blockIdx.x] = (int64_t)n_blk_here;
        return;
    }
    int64_t idx = w.blk[blockIdx.x] + (int64_t)pre;
    for (uint32_t m = found; m; idx++) {
        const int j = __builtin_ctz(m);
        m &= m - 1;
        int len, lit;
        int64_t d;
        if (j == first_j) { len = first_len; lit = first_lit; d = first_doc; }   // (the lane's first candidate: kept from above)
        else (void)sp_at(w, p0 + j, &len, &lit, &d);
        if (idx >= w.n_cand) break;
        w.cand_pos[idx] = p0 + j;
        w.cand_len[idx] = len;
        w.cand_id[idx] = w.lit_id[lit];
        w.cand_doc[idx] = d;
    }
}

__global__ void __launch_bounds__(256) k_sp_resolve(JtkSpecialWork w) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= w.n_cand) return;
    auto s = [&](int64_t k) { return w.cand_pos[k]; };
    auto e = [&](int64_t k) { return w.cand_pos[k] + w.cand_len[k]; };
    w.cand_keep[i] = jtk_special_certain(i, w.maxlen, s, e) ? 1 : 2;
}

__global__ void __launch_bounds__(256) k_sp_walk(JtkSpecialWork w) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i + 1 >= w.n_cand || w.cand_keep[i] != 1 || w.cand_keep[i + 1] == 1) return;
    // (chains are disjoint and a certain mark is never changed: each lane reads and writes its own chain only)
    auto s = [&](int64_t k) { return w.cand_pos[k]; };
    auto e = [&](int64_t k) { return w.cand_pos[k] + w.cand_len[k]; };
    jtk_special_walk(i, w.n_cand, s, e, [&](int64_t k) { return w.cand_keep[k] == 1; },
                     [&](int64_t k, bool kept) { w.cand_keep[k] = kept ? 3 : 0; });
}

__device__ __forceinline__ bool sp_kept(const JtkSpecialWork& w, int64_t i) { return w.cand_keep[i] == 1 || w.cand_keep[i] == 3; }

__global__ void __launch_bounds__(256) k_sp_docs(JtkSpecialWork w) {
    const int64_t d = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (d > w.n_docs) return;
    if (d == w.n_docs) { w.sub_off[w.n_sub] = w.doc_off[w.n_docs]; return; }
    const int64_t q = w.doc_off[d];
    const int64_t f = d + 2 * jtk_first_ge(w.cand_pos, 0, w.n_cand, q);   // (the candidates before the document: two slots each)
    w.doc_first[d] = f;
    w.sub_off[f] = q;
    w.sub_lit[f] = -1;
    w.sub_doc[f] = d;
}

__global__ void __launch_bounds__(256) k_sp_subs(JtkSpecialWork w) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= w.n_cand) return;
    const int64_t d = w.cand_doc[i], a = d + 2 * i + 1;
    w.sub_doc[a] = d;
    w.sub_doc[a + 1] = d;
    if (sp_kept(w, i)) {
        w.sub_off[a] = w.cand_pos[i];
        w.sub_off[a + 1] = w.cand_pos[i] + w.cand_len[i];
        w.sub_lit[a] = w.cand_id[i];
        w.sub_lit[a + 1] = -1;
        return;
    }
    // not kept (inside a chain): two empty slots where the segment it sits in ends -- the next kept match, or the document's end
    int64_t j = i + 1;
    while (j < w.n_cand && w.cand_doc[j] == d && !sp_kept(w, j)) j++;
    const int64_t v = (j < w.n_cand && w.cand_doc[j] == d) ? w.cand_pos[j] : w.doc_off[d + 1];
    w.sub_off[a] = v;
    w.sub_off[a + 1] = v;
    w.sub_lit[a] = -2;
    w.sub_lit[a + 1] = -2;
}

__global__ void __launch_bounds__(256) k_sp_status(JtkSpecialWork w) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= w.n_sub) return;
    const int32_t st = w.sub_status[j];
    // a literal's own status counts only for UTF-8 validation (its bytes are part of the document); an encodeOrdinary of it
    // is not part of the result
    if (st < 0 && (w.sub_lit[j] == -1 || st == -6 /* JTK_ERR_BAD_UTF8 */)) atomicMin(&w.status[w.sub_doc[j]], st);
}

__global__ void __launch_bounds__(256) k_sp_count(JtkSpecialWork w) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= w.n_sub) return;
    const int32_t lit = w.sub_lit[j];
    int64_t c = 0;
    if (w.status[w.sub_doc[j]] >= 0) c = lit >= 0 ? 1 : (lit == -2 ? 0 : w.sub_tok_off[j + 1] - w.sub_tok_off[j]);
    w.cnt[j] = c;
}

__global__ void __launch_bounds__(256) k_sp_offsets(JtkSpecialWork w) {
    const int64_t d = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (d > w.n_docs) return;
    if (d == w.n_docs) {
        w.tok_off[d] = w.cnt[w.n_sub];
        w.result->n_tokens = w.cnt[w.n_sub];
        return;
    }
    w.tok_off[d] = w.cnt[w.doc_first[d]];
    if (w.status[d] < 0) atomicMin(&w.result->worst_status, w.status[d]);
}

// (lanes take consecutive tokens -- coalesced -- and keep the sub-document of their last one: a search only where a lane's
// next token lies past it.  16 consecutive tokens per lane with a search each took 6.4 ms on the headline corpus, this 2.9)
__global__ void __launch_bounds__(GT) k_sp_gather(JtkSpecialWork w) {
    const int64_t total = w.cnt[w.n_sub];
    // the sub-document that holds output token t, searched from lo: last k in [lo - 1, n_sub) with cnt[k] <= t, the one before
    // the first k with cnt[k] > t (cnt[n_sub] = total > t)
    auto locate = [&](int64_t lo, int64_t t) { return jtk_first_gt(w.cnt, lo, w.n_sub, t) - 1; };
    for (int64_t base = (int64_t)blockIdx.x * GT * GPER; base < total; base += (int64_t)gridDim.x * GT * GPER) {
        int64_t j = -1;
        for (int k = 0; k < GPER; k++) {
            const int64_t t = base + (int64_t)k * GT + threadIdx.x;
            if (t >= total) break;
            if (j < 0 || w.cnt[j + 1] <= t) j = locate(j < 0 ? 0 : j + 1, t);
            const int32_t lit = w.sub_lit[j];
            w.tokens[t] = lit >= 0 ? lit : w.sub_tokens[w.sub_tok_off[j] + (t - w.cnt[j])];
        }
    }
}

}  // namespace

void jtk_launch_special_find(const JtkSpecialWork& w, hipStream_t s) {
    hipLaunchKernelGGL(k_sp_check, dim3(jtk_blocks_for(w.n_docs + 1, 256)), dim3(256), 0, s, w);
    if (w.n_blk > 0 && w.n_docs > 0) hipLaunchKernelGGL(k_sp_find<false>, dim3((unsigned)w.n_blk), dim3(FT), 0, s, w);
    else if (w.n_blk > 0) (void)hipMemsetAsync(w.blk, 0, (size_t)w.n_blk * 8, s);
    jtk_launch_scan_i64(w.blk, w.n_blk, &w.hdr[0], s);
}

void jtk_launch_special_write(const JtkSpecialWork& w, hipStream_t s) {
    hipLaunchKernelGGL(k_sp_find<true>, dim3((unsigned)w.n_blk), dim3(FT), 0, s, w);
    hipLaunchKernelGGL(k_sp_resolve, dim3(jtk_blocks_for(w.n_cand, 256)), dim3(256), 0, s, w);
    hipLaunchKernelGGL(k_sp_walk, dim3(jtk_blocks_for(w.n_cand, 256)), dim3(256), 0, s, w);
    hipLaunchKernelGGL(k_sp_docs, dim3(jtk_blocks_for(w.n_docs + 1, 256)), dim3(256), 0, s, w);
    hipLaunchKernelGGL(k_sp_subs, dim3(jtk_blocks_for(w.n_cand, 256)), dim3(256), 0, s, w);
}

void jtk_launch_special_stitch(const JtkSpecialWork& w, hipStream_t s) {
    hipLaunchKernelGGL(k_sp_status, dim3(jtk_blocks_for(w.n_sub, 256)), dim3(256), 0, s, w);
    hipLaunchKernelGGL(k_sp_count, dim3(jtk_blocks_for(w.n_sub, 256)), dim3(256), 0, s, w);
    jtk_launch_scan_i64(w.cnt, w.n_sub, nullptr, s);
    hipLaunchKernelGGL(k_sp_offsets, dim3(jtk_blocks_for(w.n_docs + 1, 256)), dim3(256), 0, s, w);
    if (!w.count_only) {
        int64_t g = w.n_bytes / (4 * GT * GPER) + 1;       // (about one token per 4 bytes; the loop takes any total)
        if (g > GATHER_BLOCKS_MAX) g = GATHER_BLOCKS_MAX;
        hipLaunchKernelGGL(k_sp_gather, dim3((unsigned)g), dim3(GT), 0, s, w);
    }
}
