// jtk_words.hip -- word-level quality signals of a document (jtk_batch_word_stats in jtk_abi.cpp), by the rule of
// jtk_words_rules.h.  A pass over the TEXT of the last encode.  Integer only: the results are exact.  No output needs a list of
// words: every signal is a per-document sum of events that a byte decides from its granule, at most 8 bytes before it, 4 behind it
// and a carry of one or two bits.  A lane's work is bounded by its granule of 16 bytes, whatever the length of a word; the carries
// compose across lanes by ballots and bit scans, across waves in LDS, across workgroups through kernel boundaries only.  Every
// barrier is reached by all threads of its workgroup, and the shuffles and ballots are evaluated by all 64 lanes outside any
// condition.
//
//   k_wd_mark     one lane per document: the EDGE and REF planes (as k_ln_mark of jtk_lines.hip).
//   k_wd_tile<0>  pass A.  A workgroup takes a tile of 4096 bytes, a lane a granule: three loads (the granule, the 4 bytes before
//                 and behind it), the masks, the four transforms of the granule, their composition over the wave by ballots.  Out:
//                 the tile's summary word.
//   k_wd_scan     pass B.  ONE workgroup of 1024: the tiles' carries forward (the L-or-N state, the dot carry) in ascending
//                 steps of 1024 tiles, backward (L-or-N, L) in descending steps.
//   k_wd_tile<1>  pass C.  Pass A's work again with the carries: the event masks, the stop words at the word ends, and the sums:
//                 packed counters summed over the wave; a wave without a document edge adds them once, from lane 0; in a wave
//                 with one every lane adds the segments of its granule.
//   k_wd_preset   one lane per document: 0 into every output that is asked for; n_lines.
//   k_wd_lines    one lane per unit of the held line list: 3 bytes at each end and its chars; summed as k_ln_flags does.
#include "jtk_device_prims.h"
#include "jtk_kernels.h"
#include "jtk_lines_rules.h"
#include "jtk_words_rules.h"

namespace {

constexpr int WD_THREADS = JTK_WD_TILE_GRANULES;
constexpr int WD_MAX_BLOCKS = 4096;
constexpr int SCAN_THREADS = JTK_WD_SCAN_STEP;
static_assert(WD_THREADS == 256 && JTK_WD_GRANULE == 16 && SCAN_THREADS == 1024, "a lane a granule, four waves a tile, a step of pass B one tile per thread");
static_assert(JTK_WD_GRANULE == JTK_LN_GRANULE && JTK_WD_TILE == JTK_LN_TILE, "the planes are laid out as jtk_lines.hip has them");

__device__ __forceinline__ int64_t wd_clamp(int64_t v, int64_t n) { return v < 0 ? 0 : v > n ? n : v; }

__global__ void __launch_bounds__(256) k_wd_mark(const int64_t* __restrict__ doc_off, const int32_t* __restrict__ status, int64_t n_docs, int64_t n_bytes,
                                                 uint32_t* __restrict__ edge, uint32_t* __restrict__ ref) {
    for (int64_t d = (int64_t)blockIdx.x * 256 + threadIdx.x; d <= n_docs; d += (int64_t)gridDim.x * 256) {
        const int64_t q = wd_clamp(doc_off[d], n_bytes);
        bool mark = true, refused = true;                        // (d == n_docs: what lies behind the last document is no document's)
        if (d < n_docs) {
            mark = wd_clamp(doc_off[d + 1], n_bytes) > q;
            refused = status[d] < 0;
        }
        if (!mark) continue;
        atomicOr(edge + (q >> 5), 1u << (q & 31));
        if (refused) atomicOr(ref + (q >> 5), 1u << (q & 31));
    }
}

__device__ __forceinline__ uint32_t wd_wave_or(uint32_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v |= (uint32_t)__shfl_xor((int)v, d);
    return v;
}

// a wave's four transforms in one word of LDS, and back
__device__ __forceinline__ uint32_t wd_pack_t(uint32_t f_ln, uint32_t b_ln, uint32_t b_l, uint32_t dot) { return f_ln | (b_ln << 2) | (b_l << 4) | (dot << 6); }
__device__ __forceinline__ uint32_t wd_f_ln(uint32_t t) { return t & 3u; }
__device__ __forceinline__ uint32_t wd_b_ln(uint32_t t) { return (t >> 2) & 3u; }
__device__ __forceinline__ uint32_t wd_b_l(uint32_t t) { return (t >> 4) & 3u; }
__device__ __forceinline__ uint32_t wd_dot(uint32_t t) { return (t >> 6) & 7u; }

// the sums of one segment (the bytes `seg` of a granule, all of one document) into document d
struct WdEvents {
    uint32_t starts, wchars, alpha, sym, symch, hash, ell, hits;
};
__device__ __forceinline__ void wd_add(const JtkWdOut& o, int64_t d, uint32_t n_words, uint32_t wchars, uint32_t alpha, uint32_t sym, uint32_t symch,
                                       uint32_t hash, uint32_t ell, uint32_t hits, uint32_t smask) {
    if (o.n_words && n_words) atomicAdd(o.n_words + d, (int32_t)n_words);
    if (o.word_chars && wchars) atomicAdd((unsigned long long*)o.word_chars + d, (unsigned long long)wchars);
    if (o.n_alpha_words && alpha) atomicAdd(o.n_alpha_words + d, (int32_t)alpha);
    if (o.n_symbol_words && sym) atomicAdd(o.n_symbol_words + d, (int32_t)sym);
    if (o.symbol_word_chars && symch) atomicAdd((unsigned long long*)o.symbol_word_chars + d, (unsigned long long)symch);
    if (o.n_hash && hash) atomicAdd((unsigned long long*)o.n_hash + d, (unsigned long long)hash);
    if (o.n_ellipsis && ell) atomicAdd(o.n_ellipsis + d, (int32_t)ell);
    if (o.n_stop_hits && hits) atomicAdd(o.n_stop_hits + d, (int32_t)hits);
    if (o.stop_mask && smask) atomicOr(o.stop_mask + d, smask);
}

template <bool WRITE>
__global__ void __launch_bounds__(WD_THREADS) k_wd_tile(JtkWdWork w, JtkWdStops stops) {
    __shared__ uint32_t s_ref[4], s_t[4], s_trail[4], s_rin;
    __shared__ uint64_t s_key[JTK_WD_MAX_STOP];
    __shared__ uint8_t s_idx[JTK_WD_MAX_STOP], s_first[JTK_WD_MAX_STOP_LEN + 2];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t tile = blockIdx.x;
    const int64_t g = tile * JTK_WD_TILE_GRANULES + tid, g0 = g * JTK_WD_GRANULE;
    const int64_t left = w.n_bytes - g0;
    const int valid = left >= JTK_WD_GRANULE ? JTK_WD_GRANULE : left > 0 ? (int)left : 0;

    // the granule, the 4 bytes before it and the 4 behind it (the text is readable up to the next multiple of 16)
    uint32_t w6[6] = {0, 0, 0, 0, 0, 0};
    uint64_t p23 = 0;
    if (valid > 0) {
        const uint4 q = *reinterpret_cast<const uint4*>(w.text + g0);
        w6[1] = q.x; w6[2] = q.y; w6[3] = q.z; w6[4] = q.w;
        if (g0 > 0) {
            const uint2 p = *reinterpret_cast<const uint2*>(w.text + g0 - 8);
            p23 = (uint64_t)p.x | ((uint64_t)p.y << 32);
            w6[0] = p.y;
        }
        if (left > JTK_WD_GRANULE) w6[5] = *reinterpret_cast<const uint32_t*>(w.text + g0 + JTK_WD_GRANULE);
    }
    const uint16_t* const e16 = (const uint16_t*)w.edge;
    const uint32_t e32 = (uint32_t)e16[g] | ((uint32_t)e16[g + 1] << 16);
    const uint32_t vmask = (1u << valid) - 1u;
    const uint32_t edge = e32 & vmask, eend = (e32 >> 1) & vmask, ref = ((const uint16_t*)w.ref)[g] & vmask;

    // who is refused: the last edge before a byte decides
    const uint32_t last_ref = edge ? (ref >> (31 - __builtin_clz(edge))) & 1u : 0u;
    const uint64_t has_b = __ballot(edge != 0), ref_b = __ballot(last_ref != 0);
    if (tid == 0) {
        const int64_t d = jtk_ln_doc_at(w.doc_off, w.n_docs, tile * JTK_WD_TILE);
        s_rin = (d < 0 || d >= w.n_docs || w.status[d] < 0) ? 1u : 0u;
    }
    if (WRITE) {
        if (tid < JTK_WD_MAX_STOP) { s_key[tid] = stops.key[tid]; s_idx[tid] = stops.idx[tid]; }
        if (tid < JTK_WD_MAX_STOP_LEN + 2) s_first[tid] = stops.first[tid];
    }
    if (lane == 0) s_ref[wv] = has_b ? 2u | (uint32_t)((ref_b >> (63 - __builtin_clzll(has_b))) & 1u) : 0u;
    __syncthreads();
    uint32_t r_in = s_rin;
    for (int k = 0; k < wv; k++)
        if (s_ref[k] & 2u) r_in = s_ref[k] & 1u;
    const uint64_t below = has_b & ((1ull << lane) - 1ull);
    if (below) r_in = (uint32_t)((ref_b >> (63 - __builtin_clzll(below))) & 1u);
    const JtkWdGran gr = jtk_wd_classify(w.uc, w6, valid, jtk_wd_refused_mask(edge, ref, r_in));

    // the granule's transforms and the wave's
    const uint32_t blk_f = ~gr.nw | edge, blk_b = ~gr.nw | eend;
    const uint32_t t_fln = jtk_wd_t_fwd(gr.LN, blk_f), t_bln = jtk_wd_t_bwd(gr.LN, blk_b), t_bl = jtk_wd_t_bwd(gr.L, blk_b);
    const uint32_t t_dot = valid == JTK_WD_GRANULE ? jtk_wd_dot_t(gr.dot, edge) : JTK_WD_DOT_FIX;
    const uint32_t trail = jtk_wd_trail(gr, edge);
    const uint64_t fln_set = __ballot(t_fln == JTK_WD_T_SET), fln_non = __ballot(t_fln != JTK_WD_T_ID);
    const uint64_t bln_set = __ballot(t_bln == JTK_WD_T_SET), bln_non = __ballot(t_bln != JTK_WD_T_ID);
    const uint64_t bl_set = __ballot(t_bl == JTK_WD_T_SET), bl_non = __ballot(t_bl != JTK_WD_T_ID);
    const uint64_t dot_fix = __ballot((t_dot & JTK_WD_DOT_FIX) != 0);
    const int dot_src = jtk_wd_dot_src(dot_fix, lane);
    const uint32_t r_src = (uint32_t)__shfl((int)(t_dot & 3u), dot_src < 0 ? 0 : dot_src);
    const uint32_t r_last = (uint32_t)__shfl((int)(t_dot & 3u), dot_fix ? 63 - __builtin_clzll(dot_fix) : 0);
    const uint32_t trail_up = (uint32_t)__shfl_up((int)trail, 1);
    if (lane == 0)
        s_t[wv] = wd_pack_t(jtk_wd_wave_fwd(fln_set, fln_non), jtk_wd_wave_bwd(bln_set, bln_non), jtk_wd_wave_bwd(bl_set, bl_non),
                            jtk_wd_dot_wave(dot_fix, r_last));
    if (lane == 63) s_trail[wv] = trail;
    __syncthreads();

    if (!WRITE) {
        if (tid == 0) {
            uint32_t f = JTK_WD_T_ID, bn = JTK_WD_T_ID, bl = JTK_WD_T_ID, dt = 0;
            for (int k = 0; k < 4; k++) {
                f = jtk_wd_then(f, wd_f_ln(s_t[k]));
                bn = jtk_wd_then(bn, wd_b_ln(s_t[3 - k]));
                bl = jtk_wd_then(bl, wd_b_l(s_t[3 - k]));
                dt = jtk_wd_dot_then(dt, wd_dot(s_t[k]));
            }
            w.sum_word[tile] = jtk_wd_tile_word(f, bn, bl, dt, s_trail[3]);
        }
        return;
    }

    // the carries into this granule
    const uint32_t cf = w.tile_cf[tile], cb = w.tile_cb[tile];
    uint32_t c_fln = cf & 1u, c_dot = (cf >> 3) & 3u, c_bln = cb & 1u, c_bl = (cb >> 1) & 1u;
    for (int k = 0; k < wv; k++) { c_fln = jtk_wd_apply(wd_f_ln(s_t[k]), c_fln); c_dot = jtk_wd_dot_apply(wd_dot(s_t[k]), c_dot); }
    for (int k = 3; k > wv; k--) { c_bln = jtk_wd_apply(wd_b_ln(s_t[k]), c_bln); c_bl = jtk_wd_apply(wd_b_l(s_t[k]), c_bl); }
    c_fln = jtk_wd_carry_before(fln_set, fln_non, lane, c_fln);
    c_bln = jtk_wd_carry_behind(bln_set, bln_non, lane, c_bln);
    c_bl = jtk_wd_carry_behind(bl_set, bl_non, lane, c_bl);
    c_dot = jtk_wd_dot_before(dot_src, r_src, lane, c_dot);
    uint32_t prev_trail = lane > 0 ? trail_up : wv > 0 ? s_trail[wv - 1] : tile > 0 ? jtk_wd_word_trail(w.sum_word[tile - 1]) : 0u;
    if (edge & 1u) prev_trail = 0;

    // the events
    WdEvents ev;
    ev.starts = jtk_wd_starts(gr, edge, prev_trail ? 1u : 0u);
    const uint32_t ends = jtk_wd_ends(gr, eend);
    const uint32_t ln_f = jtk_wd_seen_fwd(gr.LN, blk_f, c_fln), ln_b = jtk_wd_seen_bwd(gr.LN, blk_b, c_bln), l_b = jtk_wd_seen_bwd(gr.L, blk_b, c_bl);
    ev.wchars = gr.nw & gr.lead;
    ev.alpha = ev.starts & l_b;
    ev.sym = ev.starts & ~ln_b;
    ev.symch = ev.wchars & ~ln_f & ~ln_b;
    ev.hash = gr.hash;
    ev.ell = jtk_wd_ellipses(gr.dot, edge, c_dot) | gr.u2026;
    ev.hits = 0;
    uint32_t smask = 0;
    const uint64_t x01 = (uint64_t)w6[1] | ((uint64_t)w6[2] << 32), x23 = (uint64_t)w6[3] | ((uint64_t)w6[4] << 32);
    if (s_first[JTK_WD_MAX_STOP_LEN + 1]) {
        for (uint32_t e = ends; e; e &= e - 1u) {
            const int i = __ffs((int)e) - 1;
            uint64_t key;
            const uint32_t len = jtk_wd_word_at_end(ev.starts, prev_trail, p23, x01, x23, i, stops.fold, &key);
            const uint32_t bits = len ? jtk_wd_stop_bits(s_key, s_idx, s_first, len, key) : 0u;
            if (bits) { ev.hits |= 1u << i; smask |= bits; }
        }
    }

    // the sums: packed counters over the wave
    const uint64_t pa = (uint64_t)__popc(ev.starts) | ((uint64_t)__popc(ev.wchars) << 12) | ((uint64_t)__popc(ev.alpha) << 24) |
                        ((uint64_t)__popc(ev.sym) << 36) | ((uint64_t)__popc(ev.symch) << 48);
    const uint32_t pb = (uint32_t)__popc(ev.hash) | ((uint32_t)__popc(ev.ell) << 11) | ((uint32_t)__popc(ev.hits) << 21);
    const uint64_t sa = jtk_wave_sum(pa);
    const uint32_t sb = jtk_wave_sum(pb), sm = wd_wave_or(smask);
    if (has_b == 0ull) {                                         // the wave lies inside one document (or outside all)
        if (lane != 0 || !(sa | sb)) return;
        const int64_t d = jtk_ln_doc_at(w.doc_off, w.n_docs, g0);
        if (d < 0 || d >= w.n_docs) return;
        wd_add(w.out, d, (uint32_t)(sa & 0xFFFu), (uint32_t)((sa >> 12) & 0xFFFu), (uint32_t)((sa >> 24) & 0xFFFu), (uint32_t)((sa >> 36) & 0xFFFu),
               (uint32_t)((sa >> 48) & 0xFFFu), sb & 0x7FFu, (sb >> 11) & 0x3FFu, sb >> 21, sm);
        return;
    }
    if (!(pa | pb)) return;
    // a wave with a document edge: every lane adds the segments of its granule
    uint32_t em = edge & ~1u;
    for (int s = 0;;) {
        const int e = em ? __ffs((int)em) - 1 : JTK_WD_GRANULE;
        const uint32_t seg = ((1u << e) - 1u) & ~((1u << s) - 1u);
        if ((ev.starts | ev.wchars | ev.hash | ev.ell | ev.hits) & seg) {
            const int64_t d = jtk_ln_doc_at(w.doc_off, w.n_docs, g0 + s);
            uint32_t seg_mask = smask;
            if (edge & ~1u) {                                    // (a granule of several documents: the hits of this one)
                seg_mask = 0;
                for (uint32_t h = ev.hits & seg; h; h &= h - 1u) {
                    uint64_t key = 0;
                    const uint32_t len = jtk_wd_word_at_end(ev.starts, prev_trail, p23, x01, x23, __ffs((int)h) - 1, stops.fold, &key);
                    seg_mask |= jtk_wd_stop_bits(s_key, s_idx, s_first, len, key);
                }
            }
            if (d >= 0 && d < w.n_docs)
                wd_add(w.out, d, (uint32_t)__popc(ev.starts & seg), (uint32_t)__popc(ev.wchars & seg), (uint32_t)__popc(ev.alpha & seg),
                       (uint32_t)__popc(ev.sym & seg), (uint32_t)__popc(ev.symch & seg), (uint32_t)__popc(ev.hash & seg),
                       (uint32_t)__popc(ev.ell & seg), (uint32_t)__popc(ev.hits & seg), (ev.hits & seg) ? seg_mask : 0u);
        }
        if (!em) break;
        s = e;
        em &= em - 1u;
    }
}

// pass B: one workgroup; a step takes JTK_WD_SCAN_STEP tiles, one per thread
__global__ void __launch_bounds__(SCAN_THREADS) k_wd_scan(JtkWdWork w, int64_t n_tiles) {
    __shared__ uint32_t s_a[SCAN_THREADS / 64], s_b[SCAN_THREADS / 64], s_state[2];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t n_steps = (n_tiles + JTK_WD_SCAN_STEP - 1) / JTK_WD_SCAN_STEP;
    if (tid == 0) s_state[0] = s_state[1] = 0;
    __syncthreads();
    for (int64_t step = 0; step < n_steps; step++) {            // forward: the L-or-N state (s_state[0]) and the dot carry ([1])
        const int64_t t = step * JTK_WD_SCAN_STEP + tid;
        const bool live = t < n_tiles;
        const uint32_t word = live ? w.sum_word[t] : 0u;
        const uint32_t tf = wd_f_ln(word), td = wd_dot(word);
        const uint64_t set = __ballot(tf == JTK_WD_T_SET), non = __ballot(tf != JTK_WD_T_ID), fix = __ballot((td & JTK_WD_DOT_FIX) != 0);
        const int src = jtk_wd_dot_src(fix, lane);
        const uint32_t r_src = (uint32_t)__shfl((int)(td & 3u), src < 0 ? 0 : src);
        const uint32_t r_last = (uint32_t)__shfl((int)(td & 3u), fix ? 63 - __builtin_clzll(fix) : 0);
        if (lane == 0) { s_a[wv] = jtk_wd_wave_fwd(set, non); s_b[wv] = jtk_wd_dot_wave(fix, r_last); }
        __syncthreads();
        uint32_t c = s_state[0], cd = s_state[1];
        for (int k = 0; k < wv; k++) { c = jtk_wd_apply(s_a[k], c); cd = jtk_wd_dot_apply(s_b[k], cd); }
        c = jtk_wd_carry_before(set, non, lane, c);
        cd = jtk_wd_dot_before(src, r_src, lane, cd);
        if (live) w.tile_cf[t] = c | (cd << 3);
        __syncthreads();
        if (tid == SCAN_THREADS - 1) { s_state[0] = jtk_wd_apply(tf, c); s_state[1] = jtk_wd_dot_apply(td, cd); }
        __syncthreads();
    }
    if (tid == 0) s_state[0] = s_state[1] = 0;
    __syncthreads();
    for (int64_t step = n_steps - 1; step >= 0; step--) {        // backward: thread tid takes the step's tile 1023 - tid
        const int64_t t = step * JTK_WD_SCAN_STEP + (SCAN_THREADS - 1 - tid);
        const bool live = t < n_tiles;
        const uint32_t word = live ? w.sum_word[t] : 0u;
        const uint32_t tn = wd_b_ln(word), tl = wd_b_l(word);
        const uint64_t n_set = __ballot(tn == JTK_WD_T_SET), n_non = __ballot(tn != JTK_WD_T_ID);
        const uint64_t l_set = __ballot(tl == JTK_WD_T_SET), l_non = __ballot(tl != JTK_WD_T_ID);
        if (lane == 0) { s_a[wv] = jtk_wd_wave_fwd(n_set, n_non); s_b[wv] = jtk_wd_wave_fwd(l_set, l_non); }     // (forward in thread order)
        __syncthreads();
        uint32_t cn = s_state[0], cl = s_state[1];
        for (int k = 0; k < wv; k++) { cn = jtk_wd_apply(s_a[k], cn); cl = jtk_wd_apply(s_b[k], cl); }
        cn = jtk_wd_carry_before(n_set, n_non, lane, cn);
        cl = jtk_wd_carry_before(l_set, l_non, lane, cl);
        if (live) w.tile_cb[t] = cn | (cl << 1);
        __syncthreads();
        if (tid == SCAN_THREADS - 1) { s_state[0] = jtk_wd_apply(tn, cn); s_state[1] = jtk_wd_apply(tl, cl); }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(256) k_wd_preset(int64_t n_docs, JtkWdOut o, const int64_t* __restrict__ unit_off) {
    for (int64_t d = (int64_t)blockIdx.x * 256 + threadIdx.x; d < n_docs; d += (int64_t)gridDim.x * 256) {
        if (o.n_words) o.n_words[d] = 0;
        if (o.word_chars) o.word_chars[d] = 0;
        if (o.n_alpha_words) o.n_alpha_words[d] = 0;
        if (o.n_symbol_words) o.n_symbol_words[d] = 0;
        if (o.symbol_word_chars) o.symbol_word_chars[d] = 0;
        if (o.n_hash) o.n_hash[d] = 0;
        if (o.n_ellipsis) o.n_ellipsis[d] = 0;
        if (o.stop_mask) o.stop_mask[d] = 0;
        if (o.n_stop_hits) o.n_stop_hits[d] = 0;
        if (o.n_lines) o.n_lines[d] = unit_off ? (int32_t)(unit_off[d + 1] - unit_off[d]) : 0;
        if (o.n_bullet_lines) o.n_bullet_lines[d] = 0;
        if (o.n_ellipsis_lines) o.n_ellipsis_lines[d] = 0;
        if (o.n_terminal_lines) o.n_terminal_lines[d] = 0;
        if (o.n_short_lines) o.n_short_lines[d] = 0;
    }
}

// A wave whose units are all one document's adds its sums once, from lane 0; a wave that holds several documents adds per lane.
__global__ void __launch_bounds__(256) k_wd_lines(JtkLnWork ln, JtkWdOut o, int32_t short_line_chars) {
    const int lane = threadIdx.x & 63;
    const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool live = u < ln.n_units;
    int64_t d = -1;
    uint32_t f = 0, is_short = 0;
    if (live) {
        const int64_t b = ln.u_begin[u], e = ln.u_end[u], len = e - b;
        d = jtk_ln_doc_of_unit(ln.unit_off, ln.n_docs, u);
        if (len > 0 && b >= 0 && e <= ln.n_bytes) {
            const uint32_t h0 = ln.text[b], h1 = len >= 3 ? ln.text[b + 1] : 0u, h2 = len >= 3 ? ln.text[b + 2] : 0u;
            const uint32_t t2 = ln.text[e - 1], t1 = len >= 3 ? ln.text[e - 2] : 0u, t0 = len >= 3 ? ln.text[e - 3] : 0u;
            f = jtk_wd_line_flags(h0, h1, h2, t0, t1, t2, len);
            is_short = short_line_chars > 0 && ln.u_chars[u] < (int64_t)short_line_chars ? 1u : 0u;
        }
    }
    const int64_t d0 = __shfl(d, 0);
    const bool uniform = __ballot(live && d != d0) == 0ull;
    const uint32_t mine = ((f & JTK_WD_LINE_BULLET) ? 1u : 0u) | ((f & JTK_WD_LINE_ELLIPSIS) ? 1u << 8 : 0u) |
                          ((f & JTK_WD_LINE_TERMINAL) ? 1u << 16 : 0u) | (is_short << 24);
    const uint32_t all = jtk_wave_sum(mine);                     // (four counts of at most 64 each)
    if (!live || d < 0 || d >= ln.n_docs || (uniform && lane != 0)) return;
    const uint32_t v = uniform ? all : mine;
    if (o.n_bullet_lines && (v & 0xFFu)) atomicAdd(o.n_bullet_lines + d, (int32_t)(v & 0xFFu));
    if (o.n_ellipsis_lines && ((v >> 8) & 0xFFu)) atomicAdd(o.n_ellipsis_lines + d, (int32_t)((v >> 8) & 0xFFu));
    if (o.n_terminal_lines && ((v >> 16) & 0xFFu)) atomicAdd(o.n_terminal_lines + d, (int32_t)((v >> 16) & 0xFFu));
    if (o.n_short_lines && (v >> 24)) atomicAdd(o.n_short_lines + d, (int32_t)(v >> 24));
}

unsigned strided_blocks(int64_t items) {
    const int64_t nb = (items + 255) / 256;
    return (unsigned)(nb < 1 ? 1 : nb < WD_MAX_BLOCKS ? nb : WD_MAX_BLOCKS);
}

}  // namespace

int64_t jtk_words_tiles(int64_t n_bytes) { return (n_bytes + JTK_WD_TILE - 1) / JTK_WD_TILE; }

void jtk_launch_words_preset(const JtkWdWork& w, const int64_t* unit_off, hipStream_t s) {
    if (w.n_docs > 0) hipLaunchKernelGGL(k_wd_preset, dim3(strided_blocks(w.n_docs)), dim3(256), 0, s, w.n_docs, w.out, unit_off);
}

void jtk_launch_words_text(const JtkWdWork& w, const JtkWdStops& stops, hipStream_t s) {
    const int64_t n_tiles = jtk_words_tiles(w.n_bytes);
    if (n_tiles <= 0) return;
    hipLaunchKernelGGL(k_wd_mark, dim3(strided_blocks(w.n_docs + 1)), dim3(256), 0, s, w.doc_off, w.status, w.n_docs, w.n_bytes, w.edge, w.ref);
    hipLaunchKernelGGL(k_wd_tile<false>, dim3((unsigned)n_tiles), dim3(WD_THREADS), 0, s, w, stops);
    hipLaunchKernelGGL(k_wd_scan, dim3(1), dim3(SCAN_THREADS), 0, s, w, n_tiles);
    hipLaunchKernelGGL(k_wd_tile<true>, dim3((unsigned)n_tiles), dim3(WD_THREADS), 0, s, w, stops);
}

void jtk_launch_words_lines(const JtkWdWork& w, const JtkLnWork& ln, int32_t short_line_chars, hipStream_t s) {
    if (ln.n_units > 0) hipLaunchKernelGGL(k_wd_lines, dim3(jtk_blocks_for(ln.n_units, 256)), dim3(256), 0, s, ln, w.out, short_line_chars);
}
