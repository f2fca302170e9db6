// jtk_maxtok.hip -- Encoding.encode(text, maxTokens) / encodeOrdinary(text, maxTokens) (GptBytePairEncoding.java:43-45,
// 66-69, 79-100) for a device-resident batch, with the early exit of jtk_batch_encode_max_tokens run as kernels
// (jtk_batch_encode_device_max_tokens in jtk_abi.cpp drives the rounds):
//
//   maxtok_check     the caller's offsets are non-decreasing within [0, n_bytes] (else nothing is written)
//   maxtok_special   encode(): text.contains(literal) over the WHOLE caller text (:52-56), one lane per 16-byte block
//   maxtok_finish    round 1: the rows of documents that need no encode (special, empty, maxTokens 0)
//   maxtok_plan      count / scan / place: the open documents of the round, in document order, and their prefixes'
//                    offsets in the gather buffer; the totals go to a 16-byte word the host reads
//   maxtok_gather    the prefixes, back to back, from the caller text at any alignment (wide loads, byte shifts in registers)
//   maxtok_decide    per chunk, behind run_job's doc_offsets: the last safe piece start from the chunk's piece mask, the
//                    token bytes before it, the back-off (jtk_maxtok_rules.h), the row; undecided documents go round again
#include "jtk_device_prims.h"
#include "jtk_kernels.h"
#include "jtk_maxtok_rules.h"

namespace {

constexpr int MT_ITEMS = 4;                   // plan items per thread
constexpr int MT_BLOCK = 256;
constexpr int MT_PER_BLOCK = MT_ITEMS * MT_BLOCK;

__global__ void __launch_bounds__(256) k_mt_check(JtkMaxTokWork m) {
    const int64_t d = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (d > m.n_docs) return;
    const int64_t o = m.doc_off[d];
    if (o < 0 || o > m.n_bytes || (d > 0 && m.doc_off[d - 1] > o)) atomicOr(m.bad, 1u);
}

// the document holding [p, p + len) whole, or -1 (a literal across two documents flags neither)
__device__ int64_t mt_doc_of(const JtkMaxTokWork& m, int64_t p, int64_t len) {
    const int64_t d = jtk_first_gt(m.doc_off, 0, m.n_docs, p) - 1;       // the one before the first d with doc_off[d] > p
    return (d >= 0 && p + len <= m.doc_off[d + 1]) ? d : -1;
}

// One lane per 16-byte block of the caller text (blocks aligned in memory): every byte that some literal starts with is
// tested as special_check_at does it.
__global__ void __launch_bounds__(256) k_mt_special(JtkMaxTokWork m, JtkDeviceTables t) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uintptr_t base = (uintptr_t)m.text & ~(uintptr_t)15;
    const int64_t p0 = (int64_t)(base - (uintptr_t)m.text) + 16 * i;     // text position of the block's first byte (may be < 0)
    if (p0 >= m.n_bytes) return;
    const uint4 v = *reinterpret_cast<const uint4*>(base + 16 * (uintptr_t)i);
    const uint32_t dw[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < 16; j++) {
        const uint32_t c = (dw[j >> 2] >> (8 * (j & 3))) & 0xFFu;
        const int64_t p = p0 + j;
        if (p < 0 || p >= m.n_bytes || !((t.special_first[c >> 5] >> (c & 31)) & 1u)) continue;
        for (int s = 0; s < t.n_specials; s++) {
            const uint32_t o = t.special_off[s];
            const int len = (int)(t.special_off[s + 1] - o);
            if (p + len > m.n_bytes) continue;
            bool eq = true;
            for (int k = 0; k < len && eq; k++) eq = (m.text[p + k] == t.special_blob[o + k]);
            if (!eq) continue;
            const int64_t d = mt_doc_of(m, p, len);
            if (d >= 0) m.special[d] = 1;
        }
    }
}

__device__ __forceinline__ void mt_write_row(const JtkMaxTokWork& m, int64_t d, int64_t keep, const int32_t* ids, int lane) {
    int32_t* row = m.out_tokens + d * m.max_tokens;
    for (int64_t j = lane; j < m.max_tokens; j += 64) row[j] = j < keep ? ids[j] : m.pad_id;
}

// Round 1, one wave per document: the rows of the documents the rounds never take -- those encode() refuses (status
// JTK_ERR_UNSUPPORTED_SPECIAL), empty ones and all of them at maxTokens 0 (kept 0; truncated = the text is not empty, by the
// back-off rule).  Nothing is written when the offsets are bad.
__global__ void __launch_bounds__(256) k_mt_finish_closed(JtkMaxTokWork m) {
    const int64_t d = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (d >= m.n_docs || *m.bad) return;
    const int64_t off = m.doc_off[d], len = m.doc_off[d + 1] - off;
    const bool special = m.special[d] != 0;
    if (!special && len > 0 && m.max_tokens > 0) return;
    mt_write_row(m, d, 0, nullptr, lane);
    if (lane == 0) {
        bool tr = false;
        if (!special) {
            const uint8_t* tx = m.text + off;
            const JtkBackoff r = jtk_maxtok_backoff(tx, len, 0, 0, [](int64_t) { return (int64_t)0; });
            tr = r.ok && jtk_more_units_than(tx, r.from, len, r.units);
        }
        m.out_kept[d] = 0;
        m.out_truncated[d] = tr ? 1 : 0;
        m.out_status[d] = special ? -2 /* JTK_ERR_UNSUPPORTED_SPECIAL */ : 0;
    }
}

// plan item j: is it open in this round, which document, how many leading bytes
__device__ __forceinline__ bool mt_item(const JtkMaxTokWork& m, int64_t j, int64_t* doc, int64_t* bytes) {
    if (j >= m.n_in) return false;
    int64_t d;
    if (m.round == 1) {
        d = j;
        if (*m.bad || m.special[d]) return false;
    } else {
        d = m.act_in[j];
        if (!m.again_in[j]) return false;
    }
    const int64_t len = m.doc_off[d + 1] - m.doc_off[d];
    if (len <= 0 || m.max_tokens <= 0) return false;
    *doc = d;
    *bytes = jtk_maxtok_prefix_bytes(len, m.P, m.cb);
    return true;
}

__global__ void __launch_bounds__(MT_BLOCK) k_mt_count(JtkMaxTokWork m) {
    __shared__ uint32_t s_cnt[MT_BLOCK / 64];
    __shared__ int64_t s_bytes[MT_BLOCK / 64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    uint32_t cnt = 0;
    int64_t bytes = 0;
    for (int k = 0; k < MT_ITEMS; k++) {
        int64_t d, p;
        if (mt_item(m, (int64_t)blockIdx.x * MT_PER_BLOCK + (int64_t)k * MT_BLOCK + tid, &d, &p)) { cnt++; bytes += p; }
    }
    cnt = jtk_wave_sum(cnt);
    bytes = jtk_wave_sum(bytes);
    if (lane == 0) { s_cnt[wv] = cnt; s_bytes[wv] = bytes; }
    __syncthreads();
    if (tid == 0) {
        uint32_t c = 0; int64_t b = 0;
        for (int k = 0; k < MT_BLOCK / 64; k++) { c += s_cnt[k]; b += s_bytes[k]; }
        m.blk_cnt[blockIdx.x] = c;
        m.blk_bytes[blockIdx.x] = b;
    }
}

// one workgroup: exclusive scans of the block totals, counts then bytes, into the interleaved blk_base; the round's totals to
// hdr (and the end of the gather offsets)
__global__ void __launch_bounds__(1024) k_mt_scan(JtkMaxTokWork m) {
    const int64_t n_act = (int64_t)jtk_block_scan_array(m.n_blk, [&](int64_t i) { return m.blk_cnt[i]; },
                                                        [&](int64_t i, uint64_t v) { m.blk_base[2 * i] = (int64_t)v; });
    const int64_t n_bytes = (int64_t)jtk_block_scan_array(m.n_blk, [&](int64_t i) { return m.blk_bytes[i]; },
                                                          [&](int64_t i, uint64_t v) { m.blk_base[2 * i + 1] = (int64_t)v; });
    if (threadIdx.x == 0) {
        m.hdr[0] = *m.bad ? -1 : n_act;
        m.hdr[1] = n_bytes;
        m.goff[n_act] = n_bytes;
    }
}

__global__ void __launch_bounds__(MT_BLOCK) k_mt_place(JtkMaxTokWork m) {
    const int tid = threadIdx.x;
    // thread tid owns items [tid * MT_ITEMS, tid * MT_ITEMS + MT_ITEMS) of the block: slots stay in item order
    const int64_t j0 = (int64_t)blockIdx.x * MT_PER_BLOCK + (int64_t)tid * MT_ITEMS;
    int64_t doc[MT_ITEMS], pb[MT_ITEMS];
    bool on[MT_ITEMS];
    uint32_t cnt = 0;
    int64_t bytes = 0;
#pragma unroll
    for (int k = 0; k < MT_ITEMS; k++) {
        on[k] = mt_item(m, j0 + k, &doc[k], &pb[k]);
        if (on[k]) { cnt++; bytes += pb[k]; }
    }
    uint32_t c_pre;
    int64_t b_pre;
    jtk_block_excl_prefix<MT_BLOCK>(cnt, bytes, &c_pre, &b_pre);
    int64_t slot = m.blk_base[2 * blockIdx.x] + c_pre;
    int64_t off = m.blk_base[2 * blockIdx.x + 1] + b_pre;
#pragma unroll
    for (int k = 0; k < MT_ITEMS; k++) {
        if (!on[k]) continue;
        m.act[slot] = doc[k];
        m.goff[slot] = off;
        slot++;
        off += pb[k];
    }
}

// 16 bytes of the caller text from `src` (any alignment), for `n` of them; only the aligned blocks holding
// src[0, n) are read.  Byte k of the result (little-endian in 4 dwords) is src[k].
__device__ __forceinline__ void mt_load16(const uint8_t* src, int n, uint32_t out[4]) {
    const uintptr_t a = (uintptr_t)src & ~(uintptr_t)15;
    const int sh = (int)((uintptr_t)src - a);
    const uint4 v0 = *reinterpret_cast<const uint4*>(a);
    uint4 v1 = make_uint4(0, 0, 0, 0);
    if (sh + n > 16) v1 = *reinterpret_cast<const uint4*>(a + 16);
    const uint32_t x[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
    const int dw = sh >> 2;
    const uint32_t bs = (uint32_t)(sh & 3);
    uint32_t y[5];
#pragma unroll
    for (int k = 0; k < 5; k++) y[k] = dw == 0 ? x[k] : dw == 1 ? x[k + 1] : dw == 2 ? x[k + 2] : x[k + 3 < 8 ? k + 3 : 7];
#pragma unroll
    for (int k = 0; k < 4; k++) out[k] = __builtin_amdgcn_alignbyte(y[k + 1], y[k], bs);
}

// One wave per open document: its prefix to gather[goff[i], goff[i + 1]).  Lanes take the aligned 16-byte words of the
// destination; a word wholly inside the prefix is one 16-byte store, the (at most two) words shared with the neighbours
// are written byte by byte so that no lane touches another document's bytes.
__global__ void __launch_bounds__(256) k_mt_gather(JtkMaxTokWork m, int64_t n_act) {
    const int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (i >= n_act) return;
    const int64_t g0 = m.goff[i], g1 = m.goff[i + 1];
    if (g1 <= g0) return;
    const uint8_t* src = m.text + m.doc_off[m.act[i]];
    const int64_t w0 = g0 >> 4, w1 = (g1 + 15) >> 4;
    for (int64_t wd = w0 + lane; wd < w1; wd += 64) {
        const int64_t lo = wd * 16 > g0 ? wd * 16 : g0;
        const int64_t hi = wd * 16 + 16 < g1 ? wd * 16 + 16 : g1;
        const int n = (int)(hi - lo);
        uint32_t v[4];
        mt_load16(src + (lo - g0), n, v);
        if (n == 16) {
            *reinterpret_cast<uint4*>(m.gather + lo) = make_uint4(v[0], v[1], v[2], v[3]);
        } else {
#pragma unroll
            for (int k = 0; k < 16; k++)
                if (k < n) m.gather[lo + k] = (uint8_t)(v[k >> 2] >> (8 * (k & 3)));
        }
    }
}

// Per chunk, one wave per document of the chunk (slot0 + i of the round): the decision of jtk_batch_encode_max_tokens.
__global__ void __launch_bounds__(256) k_mt_decide(JtkWork w, JtkMaxTokWork m, int64_t slot0) {
    const int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (i >= w.n_docs) return;
    const int64_t slot = slot0 + i;
    const int64_t d = m.act[slot];
    const int64_t len = m.doc_off[d + 1] - m.doc_off[d];
    const int64_t g0 = m.goff[slot], p = m.goff[slot + 1] - g0;
    const uint8_t* t = m.gather + g0;
    const int32_t st = w.status[i];
    const int64_t t0 = w.tok_off[i], n = w.tok_off[i + 1] - t0;
    const int32_t* ids = w.tokens + t0;
    const int64_t mx = m.max_tokens;
    // (ids past the decode table are the pseudo ids of bytes a rank map lacks: one byte each; their documents are refused)
    auto tok_len = [&](int64_t j) { return jtk_tok_len(m.tab_off, m.n_ids_table, ids[j], 1u); };
    if (st != 0) {                                        // (the pipeline's status: no tokens, as on the host)
        mt_write_row(m, d, 0, nullptr, lane);
        if (lane == 0) { m.out_kept[d] = 0; m.out_truncated[d] = 0; m.out_status[d] = st; m.again[slot] = 0; }
        return;
    }
    int64_t k = -1, nb = 0;
    if (p == len) {
        k = n < mx ? n : mx;
        for (int64_t b = 0; b < k; b += 64) nb += jtk_wave_sum(b + lane < k ? tok_len(b + lane) : 0u);
    } else {
        // the last safe piece start q at or before p - JTK_MAXTOK_MARGIN: 64 mask words per step, backwards
        const int64_t base = g0 - w.text_base;            // the prefix in the chunk's piece mask
        const int64_t top = base + p - JTK_MAXTOK_MARGIN;
        int64_t q = 0;
        if (top > base) {
            const int64_t wl = (base + 1) >> 6;
            for (int64_t wh = top >> 6; wh >= wl && q == 0; wh -= 64) {
                const int64_t wi = wh - lane;
                int64_t best = 0;
                if (wi >= wl) {
                    uint64_t bits = w.piecemask[wi];
                    if (wi == (top >> 6) && (top & 63) != 63) bits &= (2ull << (top & 63)) - 1;   // bits 0..top
                    if (wi == (base >> 6)) bits &= ~((2ull << (base & 63)) - 1);                  // bits above base
                    while (bits) {
                        const int bit = 63 - __builtin_clzll(bits);
                        const int64_t cand = wi * 64 + bit - base;
                        if (jtk_maxtok_safe_start(t[cand], t[cand + 1])) { best = cand; break; }
                        bits &= ~(1ull << bit);
                    }
                }
                const uint64_t found = __ballot(best > 0);
                if (found) q = __shfl(best, __ffsll((unsigned long long)found) - 1);   // the lowest lane holds the highest word
            }
        }
        if (q > 0 && n >= mx) {
            int64_t cum = 0;
            for (int64_t b = 0; b < mx && cum <= q; b += 64) cum += jtk_wave_sum(b + lane < mx ? tok_len(b + lane) : 0u);
            if (jtk_maxtok_decided(n, mx, cum, q)) { k = mx; nb = cum; }
        }
    }
    if (k < 0) {
        if (lane == 0) m.again[slot] = 1;
        return;
    }
    // the back-off reads the text around the cut from the prefix (every lane the same: uniform loads)
    const JtkBackoff r = jtk_maxtok_backoff(t, len, k, nb, [&](int64_t j) { return (int64_t)tok_len(j); });
    const int64_t avail = m.gbytes - g0;                 // (the gathered bytes from here on)
    const bool tr = r.ok && jtk_more_units_than(t, r.from, len < avail ? len : avail, r.units);
    mt_write_row(m, d, r.keep, ids, lane);
    if (lane == 0) { m.out_kept[d] = r.keep; m.out_truncated[d] = tr ? 1 : 0; m.out_status[d] = 0; m.again[slot] = 0; }
}

}  // namespace

void jtk_launch_maxtok_check(const JtkMaxTokWork& m, hipStream_t s) {
    const int64_t n = m.n_docs + 1;
    hipLaunchKernelGGL(k_mt_check, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, m);
}
void jtk_launch_maxtok_special(const JtkMaxTokWork& m, const JtkDeviceTables& t, hipStream_t s) {
    if (m.n_bytes <= 0 || t.n_specials <= 0) return;
    const uintptr_t a = (uintptr_t)m.text & ~(uintptr_t)15, e = ((uintptr_t)m.text + (uintptr_t)m.n_bytes + 15) & ~(uintptr_t)15;
    const int64_t blocks = (int64_t)((e - a) / 16);
    hipLaunchKernelGGL(k_mt_special, dim3((unsigned)((blocks + 255) / 256)), dim3(256), 0, s, m, t);
}
void jtk_launch_maxtok_finish_closed(const JtkMaxTokWork& m, hipStream_t s) {
    if (m.n_docs <= 0) return;
    hipLaunchKernelGGL(k_mt_finish_closed, dim3((unsigned)((m.n_docs + 3) / 4)), dim3(256), 0, s, m);
}
void jtk_launch_maxtok_plan(const JtkMaxTokWork& m, hipStream_t s) {
    const unsigned nb = (unsigned)(m.n_blk > 0 ? m.n_blk : 1);
    hipLaunchKernelGGL(k_mt_count, dim3(nb), dim3(MT_BLOCK), 0, s, m);
    hipLaunchKernelGGL(k_mt_scan, dim3(1), dim3(1024), 0, s, m);
    hipLaunchKernelGGL(k_mt_place, dim3(nb), dim3(MT_BLOCK), 0, s, m);
}
void jtk_launch_maxtok_gather(const JtkMaxTokWork& m, int64_t n_act, hipStream_t s) {
    if (n_act > 0) hipLaunchKernelGGL(k_mt_gather, dim3((unsigned)((n_act + 3) / 4)), dim3(256), 0, s, m, n_act);
}
void jtk_launch_maxtok_decide(const JtkWork& w, const JtkMaxTokWork& m, int64_t slot0, hipStream_t s) {
    if (w.n_docs > 0) hipLaunchKernelGGL(k_mt_decide, dim3((unsigned)((w.n_docs + 3) / 4)), dim3(256), 0, s, w, m, slot0);
}
