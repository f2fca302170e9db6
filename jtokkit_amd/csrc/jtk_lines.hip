// jtk_lines.hip -- duplicate lines and paragraphs inside a document (jtk_batch_line_units / jtk_batch_line_repeats in
// jtk_abi.cpp), by the rule of jtk_lines_rules.h.  A pass over the TEXT of the last encode.  Integer only: the results are
// bit-exact.  A lane's work is bounded by its granule of 16 bytes, whatever the length of a line; no workgroup waits for
// another: every carry crosses a kernel boundary.  Every barrier is reached by all threads of its workgroup, and the shuffles
// and ballots are evaluated by all 64 lanes outside any condition.
//
//   k_ln_mark     one lane per document: its bit in the EDGE plane where it starts (non-empty documents; and the bit at the last
//                 document's end), its bit in the REF plane when it is refused.  atomicOr on 32-bit words of planes preset to 0.
//   k_ln_tile<0>  pass A.  A workgroup takes a tile of 4096 bytes, a lane a granule: one 16-byte load, the masks, the refusal from
//                 ballots of the planes' bits (the tile's first byte: one offset search by one lane), the granule's two
//                 transforms, one wave scan of each (forward by __shfl_up, backward by __shfl_down), the hash of the granule and
//                 its wave scan with constant multipliers G^(16 d), the starts the tile decides alone.  Out: the tile's word,
//                 starts, chars and hash.
//   k_ln_scan     pass B.  ONE workgroup of 1024: the tiles' carries forward (ascending steps of 1024 tiles) -- state, units,
//                 chars, P -- and backward (descending steps).
//   k_ln_tile<1>  pass C.  Pass A's work again with the carries; every start byte writes begin, P, chars of its unit, every end
//                 byte end, P, chars; every edge bit the units and chars before its document.
//   k_ln_docs     one lane per d <= n_docs: unit_off and the chars before it, from the entry of the document that starts there.
//   k_ln_keys     one lane per unit: k from the two prefixes (G^length by squaring), chars.
//   k_ln_preset / k_ln_insert / k_ln_flags / k_ln_doc_out   the repeats: jtk_repeat.hip's two passes with unit indices for
//                 token positions, one lane per unit of the group; k_rp_top unpacks the top words.
#include "jtk_device_prims.h"
#include "jtk_kernels.h"
#include "jtk_lines_rules.h"

namespace {

constexpr int LN_THREADS = JTK_LN_TILE_GRANULES;
constexpr int LN_MAX_BLOCKS = 4096;
constexpr uint64_t POW_WAVE = jtk_ln_pow(JTK_LN_WAVE_BYTES), POW_TILE = jtk_ln_pow(JTK_LN_TILE), POW_TILE64 = jtk_ln_pow((uint64_t)JTK_LN_TILE * 64);
constexpr int SCAN_THREADS = JTK_LN_SCAN_STEP;
static_assert(LN_THREADS == 256 && JTK_LN_GRANULE == 16 && SCAN_THREADS == 1024, "a lane a granule, four waves a tile, a step of pass B one tile per thread");

struct DevCas {
    __device__ uint64_t operator()(uint64_t* p, uint64_t k) const {
        return (uint64_t)atomicCAS((unsigned long long*)p, 0ull, (unsigned long long)k);
    }
};

__device__ __forceinline__ int64_t ln_clamp(int64_t v, int64_t n) { return v < 0 ? 0 : v > n ? n : v; }

__global__ void __launch_bounds__(256) k_ln_mark(const int64_t* __restrict__ doc_off, const int32_t* __restrict__ status, int64_t n_docs, int64_t n_bytes,
                                                 uint32_t* __restrict__ edge, uint32_t* __restrict__ ref) {
    for (int64_t d = (int64_t)blockIdx.x * 256 + threadIdx.x; d <= n_docs; d += (int64_t)gridDim.x * 256) {
        const int64_t q = ln_clamp(doc_off[d], n_bytes);
        bool mark = true, refused = true;                        // (d == n_docs: what lies behind the last document is no document's)
        if (d < n_docs) {
            mark = ln_clamp(doc_off[d + 1], n_bytes) > q;
            refused = status[d] < 0;
        }
        if (!mark) continue;
        atomicOr(edge + (q >> 5), 1u << (q & 31));
        if (refused) atomicOr(ref + (q >> 5), 1u << (q & 31));
    }
}

// inclusive scans of transforms across the wave: forward (lane l: granules 0 .. l) and backward (granules 63 .. l)
__device__ __forceinline__ uint32_t ln_wave_scan_fwd(uint32_t t, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = (uint32_t)__shfl_up((int)t, d);
        if (lane >= d) t = jtk_ln_then(o, t);
    }
    return t;
}
__device__ __forceinline__ uint32_t ln_wave_scan_bwd(uint32_t t, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = (uint32_t)__shfl_down((int)t, d);
        if (lane + d < 64) t = jtk_ln_then(o, t);
    }
    return t;
}
// inclusive scan of hashes of `span` bytes each: lane l holds H of the items 0 .. l
template <uint64_t SPAN>
__device__ __forceinline__ uint64_t ln_wave_scan_hash(uint64_t h, int lane) {
    constexpr uint64_t M1 = jtk_ln_pow(SPAN), M2 = jtk_ln_pow(SPAN * 2), M4 = jtk_ln_pow(SPAN * 4), M8 = jtk_ln_pow(SPAN * 8),
                       M16 = jtk_ln_pow(SPAN * 16), M32 = jtk_ln_pow(SPAN * 32);
    { const uint64_t o = __shfl_up(h, 1);  if (lane >= 1)  h += o * M1; }
    { const uint64_t o = __shfl_up(h, 2);  if (lane >= 2)  h += o * M2; }
    { const uint64_t o = __shfl_up(h, 4);  if (lane >= 4)  h += o * M4; }
    { const uint64_t o = __shfl_up(h, 8);  if (lane >= 8)  h += o * M8; }
    { const uint64_t o = __shfl_up(h, 16); if (lane >= 16) h += o * M16; }
    { const uint64_t o = __shfl_up(h, 32); if (lane >= 32) h += o * M32; }
    return h;
}

template <bool WRITE>
__global__ void __launch_bounds__(LN_THREADS) k_ln_tile(JtkLnWork w) {
    __shared__ uint32_t s_ref[4], s_tf[4], s_tb[4], s_open, s_rin;
    __shared__ uint64_t s_h[4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t tile = blockIdx.x;
    const int64_t g = tile * JTK_LN_TILE_GRANULES + tid, g0 = g * JTK_LN_GRANULE;
    const int64_t left = w.n_bytes - g0;
    const int valid = left >= JTK_LN_GRANULE ? JTK_LN_GRANULE : left > 0 ? (int)left : 0;
    const uint32_t thr = jtk_ln_threshold(w.unit);

    uint32_t x[4] = {0, 0, 0, 0};
    if (valid > 0) {                                             // (the text is readable up to the next multiple of 16)
        const uint4 q = *reinterpret_cast<const uint4*>(w.text + g0);
        x[0] = q.x; x[1] = q.y; x[2] = q.z; x[3] = q.w;
    }
    const uint16_t* const e16 = (const uint16_t*)w.edge;
    const uint32_t e32 = (uint32_t)e16[g] | ((uint32_t)e16[g + 1] << 16);
    const uint32_t vmask = (1u << valid) - 1u;
    const uint32_t edge = e32 & vmask, eend = (e32 >> 1) & vmask, ref = ((const uint16_t*)w.ref)[g] & vmask;

    // who is refused: the last edge before a byte decides
    const uint32_t last_ref = edge ? (ref >> (31 - __builtin_clz(edge))) & 1u : 0u;
    const uint64_t has_b = __ballot(edge != 0), ref_b = __ballot(last_ref != 0);
    if (tid == 0) {
        const int64_t d = jtk_ln_doc_at(w.doc_off, w.n_docs, tile * JTK_LN_TILE);
        s_rin = (d < 0 || d >= w.n_docs || w.status[d] < 0) ? 1u : 0u;
        s_open = 0;
    }
    if (lane == 0) s_ref[wv] = has_b ? 2u | (uint32_t)((ref_b >> (63 - __builtin_clzll(has_b))) & 1u) : 0u;
    __syncthreads();
    uint32_t r_in = s_rin;
    for (int k = 0; k < wv; k++)
        if (s_ref[k] & 2u) r_in = s_ref[k] & 1u;
    const uint64_t below = has_b & ((1ull << lane) - 1ull);
    if (below) r_in = (uint32_t)((ref_b >> (63 - __builtin_clzll(below))) & 1u);
    uint32_t r_out;
    const uint32_t refused = jtk_ln_refused_mask(edge, ref, r_in, &r_out);
    const JtkLnGran gr = jtk_ln_classify(x, valid, w.flags, refused);

    // the carries inside the tile
    const uint32_t tf_i = ln_wave_scan_fwd(jtk_ln_gran_fwd(gr, edge), lane);
    const uint32_t tb_i = ln_wave_scan_bwd(jtk_ln_gran_bwd(gr, eend), lane);
    const uint32_t tf_up = (uint32_t)__shfl_up((int)tf_i, 1), tb_dn = (uint32_t)__shfl_down((int)tb_i, 1);
    const uint64_t h_i = ln_wave_scan_hash<JTK_LN_GRANULE>(jtk_ln_gran_hash(x), lane);
    const uint64_t h_up = __shfl_up(h_i, 1);
    if (lane == 63) { s_tf[wv] = tf_i; s_h[wv] = h_i; }
    if (lane == 0) s_tb[wv] = tb_i;
    __syncthreads();
    uint32_t t_in = WRITE ? jtk_ln_fix(w.tile_cf[tile]) : JTK_LN_T_ID;
    for (int k = 0; k < wv; k++) t_in = jtk_ln_then(t_in, s_tf[k]);
    if (lane > 0) t_in = jtk_ln_then(t_in, tf_up);
    uint32_t open = 0;
    const uint32_t starts = jtk_ln_starts(gr, edge, t_in, thr, &open);
    uint32_t c_pre;
    int64_t ch_pre;
    jtk_block_excl_prefix<LN_THREADS>((uint32_t)__popc(starts), (int64_t)__popc(gr.nonc), &c_pre, &ch_pre);     // (a barrier)

    if (!WRITE) {
        if (open) s_open = open;                                 // (at most one byte of a tile is open)
        __syncthreads();
        if (tid == LN_THREADS - 1) {
            uint32_t tf = JTK_LN_T_ID, tb = JTK_LN_T_ID;
            uint64_t h = 0;
            for (int k = 0; k < 4; k++) {
                tf = jtk_ln_then(tf, s_tf[k]);
                tb = jtk_ln_then(tb, s_tb[3 - k]);
                h = h * POW_WAVE + s_h[k];
            }
            w.sum_word[tile] = jtk_ln_tile_word(tf, tb, s_open);
            w.sum_units[tile] = c_pre + (uint32_t)__popc(starts);
            w.sum_chars[tile] = (uint32_t)ch_pre + (uint32_t)__popc(gr.nonc);
            w.sum_hash[tile] = h;
        }
        return;
    }

    uint32_t s_b = w.tile_cb[tile];
    for (int k = 3; k > wv; k--) s_b = jtk_ln_apply(s_tb[k], s_b);
    if (lane < 63) s_b = jtk_ln_apply(tb_dn, s_b);
    const uint32_t ends = jtk_ln_ends(gr, eend, s_b, thr);
    uint64_t H = w.tile_hash[tile];
    for (int k = 0; k < wv; k++) H = H * POW_WAVE + s_h[k];
    H = H * jtk_ln_pow((uint64_t)lane * JTK_LN_GRANULE) + (lane > 0 ? h_up : 0ull);
    int64_t u = w.tile_units[tile] + c_pre, ch = w.tile_chars[tile] + ch_pre;
    if (!(starts | ends | edge)) return;
#pragma unroll
    for (int i = 0; i < JTK_LN_GRANULE; i++) {
        const int64_t p = g0 + i;                                // (bits at or behind `valid` are 0 in all three masks)
        if ((edge >> i) & 1u) {
            const int64_t d = jtk_ln_doc_at(w.doc_off, w.n_docs, p);
            if (d >= 0 && d < w.n_docs) { w.doc_units[d] = u; w.doc_chars[d] = ch; }
        }
        if (((starts >> i) & 1u) && u < w.n_units) { w.u_begin[u] = p; w.u_k[u] = H; w.u_chars[u] = ch; }
        u += (starts >> i) & 1u;
        ch += (gr.nonc >> i) & 1u;
        H = jtk_ln_step(H, (x[i >> 2] >> (8 * (i & 3))) & 0xFFu);
        if (((ends >> i) & 1u) && u >= 1 && u <= w.n_units) { w.u_end[u - 1] = p + 1; w.u_pe[u - 1] = H; w.u_ce[u - 1] = ch; }
    }
}

// pass B: one workgroup; a step takes JTK_LN_SCAN_STEP tiles, one per thread
__global__ void __launch_bounds__(SCAN_THREADS) k_ln_scan(JtkLnWork w, int64_t n_tiles) {
    __shared__ uint32_t s_t[SCAN_THREADS / 64], s_state;
    __shared__ uint64_t s_u[SCAN_THREADS / 64], s_c[SCAN_THREADS / 64], s_h[SCAN_THREADS / 64], s_base[3];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const uint32_t thr = jtk_ln_threshold(w.unit);
    const int64_t n_steps = (n_tiles + JTK_LN_SCAN_STEP - 1) / JTK_LN_SCAN_STEP;
    if (tid == 0) { s_state = JTK_LN_NOINK; s_base[0] = s_base[1] = s_base[2] = 0; }
    __syncthreads();
    for (int64_t step = 0; step < n_steps; step++) {
        const int64_t t = step * JTK_LN_SCAN_STEP + tid;
        const bool live = t < n_tiles;
        const uint32_t word = live ? w.sum_word[t] : 0u;
        const uint32_t tf_i = ln_wave_scan_fwd(jtk_ln_word_fwd(word), lane);
        const uint32_t tf_up = (uint32_t)__shfl_up((int)tf_i, 1);
        if (lane == 63) s_t[wv] = tf_i;
        __syncthreads();
        uint32_t s = s_state;
        for (int k = 0; k < wv; k++) s = jtk_ln_apply(s_t[k], s);
        if (lane > 0) s = jtk_ln_apply(tf_up, s);                // the state before tile t
        const uint64_t un = live ? (uint64_t)w.sum_units[t] + jtk_ln_open_starts(jtk_ln_word_open(word), s, thr) : 0ull;
        const uint64_t cn = live ? (uint64_t)w.sum_chars[t] : 0ull;
        const uint64_t u_i = jtk_wave_incl_scan(un), c_i = jtk_wave_incl_scan(cn);
        const uint64_t h_i = ln_wave_scan_hash<JTK_LN_TILE>(live ? w.sum_hash[t] : 0ull, lane);
        const uint64_t h_up = __shfl_up(h_i, 1);
        if (lane == 63) { s_u[wv] = u_i; s_c[wv] = c_i; s_h[wv] = h_i; }
        __syncthreads();
        uint64_t ub = s_base[0], cb = s_base[1], hb = s_base[2];
        for (int k = 0; k < wv; k++) { ub += s_u[k]; cb += s_c[k]; hb = hb * POW_TILE64 + s_h[k]; }
        hb = hb * jtk_ln_pow((uint64_t)lane * JTK_LN_TILE) + (lane > 0 ? h_up : 0ull);
        if (live) {
            w.tile_cf[t] = s;
            w.tile_units[t] = (int64_t)(ub + u_i - un);
            w.tile_chars[t] = (int64_t)(cb + c_i - cn);
            w.tile_hash[t] = hb;
        }
        __syncthreads();
        if (tid == SCAN_THREADS - 1) {                             // the carries behind the step's last tile
            s_state = jtk_ln_apply(jtk_ln_word_fwd(word), s);
            s_base[0] = ub + u_i;
            s_base[1] = cb + c_i;
            s_base[2] = hb * POW_TILE + (live ? w.sum_hash[t] : 0ull);
        }
        __syncthreads();
    }
    if (tid == 0) {
        w.hdr[0] = (int64_t)s_base[0];
        w.doc_units[w.n_docs] = (int64_t)s_base[0];              // the entry of the text's end
        w.doc_chars[w.n_docs] = (int64_t)s_base[1];
        s_state = JTK_LN_NOINK;
    }
    __syncthreads();
    for (int64_t step = n_steps - 1; step >= 0; step--) {        // backward: thread tid takes the step's tile 1023 - tid
        const int64_t t = step * JTK_LN_SCAN_STEP + (SCAN_THREADS - 1 - tid);
        const bool live = t < n_tiles;
        const uint32_t tb = live ? jtk_ln_word_bwd(w.sum_word[t]) : JTK_LN_T_ID;
        const uint32_t tb_i = ln_wave_scan_fwd(tb, lane);
        const uint32_t tb_up = (uint32_t)__shfl_up((int)tb_i, 1);
        if (lane == 63) s_t[wv] = tb_i;
        __syncthreads();
        uint32_t s = s_state;
        for (int k = 0; k < wv; k++) s = jtk_ln_apply(s_t[k], s);
        if (lane > 0) s = jtk_ln_apply(tb_up, s);                // the state behind tile t
        if (live) w.tile_cb[t] = s;
        __syncthreads();
        if (tid == SCAN_THREADS - 1) s_state = jtk_ln_apply(tb, s);
        __syncthreads();
    }
}

__global__ void __launch_bounds__(256) k_ln_docs(JtkLnWork w) {
    for (int64_t d = (int64_t)blockIdx.x * 256 + threadIdx.x; d <= w.n_docs; d += (int64_t)gridDim.x * 256) {
        // the entry that holds the counts before doc_off[d]: of the non-empty document that starts there, or of the text's end
        const int64_t q = ln_clamp(w.doc_off[d], w.n_bytes);
        int64_t at = jtk_ln_doc_at(w.doc_off, w.n_docs, q);
        if (at < 0) at = 0;                                      // (offsets that the encode refused: nothing is read outside the arrays)
        if (d == w.n_docs) at = w.n_docs;
        w.unit_off[d] = w.doc_units[at];
        w.char_off[d] = w.doc_chars[at];
    }
}

__global__ void __launch_bounds__(256) k_ln_keys(JtkLnWork w, uint64_t key, uint64_t base) {
    const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (u >= w.n_units) return;
    const int64_t b = w.u_begin[u], e = w.u_end[u];
    const int64_t d = jtk_ln_doc_of_unit(w.unit_off, w.n_docs, u);
    const uint64_t h = jtk_ln_range_hash(w.u_k[u], w.u_pe[u], e - b);
    w.u_k[u] = jtk_ln_finish(h, jtk_rp_doc_key(key, base, d));
    w.u_chars[u] = w.u_ce[u] - w.u_chars[u];
}

__global__ void __launch_bounds__(256) k_ln_preset(int64_t n_docs, JtkLnOut o, uint64_t* __restrict__ top) {
    for (int64_t d = (int64_t)blockIdx.x * 256 + threadIdx.x; d < n_docs; d += (int64_t)gridDim.x * 256) {
        if (o.n_dup) o.n_dup[d] = 0;
        if (o.dup_bytes) o.dup_bytes[d] = 0;
        if (o.dup_chars) o.dup_chars[d] = 0;
        if (o.unit_bytes) o.unit_bytes[d] = 0;
        if (o.unit_chars) o.unit_chars[d] = 0;
        if (top) top[d] = 0;
    }
}

__global__ void __launch_bounds__(256) k_ln_doc_out(int64_t n_docs, const int64_t* __restrict__ unit_off, const int64_t* __restrict__ char_off,
                                                    int64_t* __restrict__ o_unit_off, int64_t* __restrict__ o_doc_chars) {
    for (int64_t d = (int64_t)blockIdx.x * 256 + threadIdx.x; d <= n_docs; d += (int64_t)gridDim.x * 256) {
        if (o_unit_off) o_unit_off[d] = unit_off[d];
        if (o_doc_chars && d < n_docs) o_doc_chars[d] = char_off[d + 1] - char_off[d];
    }
}

// pass 1.  Equal k at consecutive units of a wave (a line repeated back to back: consecutive units with one k are one document's)
// become one (min, +r) pair at the run's first lane, as jtk_rp_lane_runs does inside a lane.  The shuffle and the ballots: all
// 64 lanes, outside any condition.
__global__ void __launch_bounds__(256) k_ln_insert(const uint64_t* __restrict__ u_k, JtkRpTable t, int64_t lo, int64_t hi) {
    const int lane = threadIdx.x & 63;
    const int64_t u = lo + (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool live = u < hi;
    const uint64_t k = live ? u_k[u] : 0ull;                     // (no unit's k is 0)
    const uint64_t up = __shfl_up(k, 1);
    const bool head = live && (lane == 0 || up != k);
    const uint64_t heads = __ballot(head), lives = __ballot(live);
    if (!head) return;
    const uint64_t above = lane == 63 ? 0ull : (heads >> (lane + 1)) << (lane + 1);
    const int end = above ? __ffsll((unsigned long long)above) - 1 : __popcll(lives);       // (the live lanes of a wave are its first ones)
    const uint64_t slot = jtk_rp_claim(t.key, t.mask, k, DevCas());
    atomicMin((unsigned long long*)t.first + slot, (unsigned long long)u);
    atomicAdd(t.count + slot, (uint32_t)(end - lane));
}

// pass 2.  A wave whose units are all one document's (a page of many lines) adds its sums once, from lane 0; a wave that holds
// several documents adds per lane.
__global__ void __launch_bounds__(256) k_ln_flags(JtkLnWork w, uint32_t mode, JtkRpTable t, int64_t lo, int64_t hi, JtkLnOut o,
                                                  uint64_t* __restrict__ top) {
    const int lane = threadIdx.x & 63;
    const int64_t u = lo + (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool live = u < hi;
    bool rep = false;
    int64_t d = -1, bytes = 0, chars = 0;
    if (live) {
        const uint64_t slot = jtk_rp_find(t.key, t.mask, w.u_k[u]);
        const uint64_t first = t.first[slot];
        const uint32_t count = t.count[slot];
        rep = jtk_rp_is_repeat(mode, u, first, count);
        if (o.unit_flags) o.unit_flags[u] = rep ? 1 : 0;
        d = jtk_ln_doc_of_unit(w.unit_off, w.n_docs, u);
        bytes = w.u_end[u] - w.u_begin[u];
        chars = w.u_chars[u];
        if (top && first == (uint64_t)u)
            atomicMax((unsigned long long*)top + d, (unsigned long long)jtk_rp_top_pack(count, u - w.unit_off[d]));
    }
    const int64_t d0 = __shfl(d, 0);
    const bool uniform = __ballot(live && d != d0) == 0ull;
    const int64_t all_bytes = jtk_wave_sum(bytes), all_chars = jtk_wave_sum(chars);
    const int64_t rep_bytes = jtk_wave_sum(rep ? bytes : (int64_t)0), rep_chars = jtk_wave_sum(rep ? chars : (int64_t)0);
    const uint32_t reps = jtk_wave_sum(rep ? 1u : 0u);
    if (!live || (uniform && lane != 0)) return;
    const int64_t ub = uniform ? all_bytes : bytes, uc = uniform ? all_chars : chars;
    const int64_t db = uniform ? rep_bytes : (rep ? bytes : 0), dc = uniform ? rep_chars : (rep ? chars : 0);
    const uint32_t nr = uniform ? reps : (rep ? 1u : 0u);
    if (o.unit_bytes && ub) atomicAdd((unsigned long long*)o.unit_bytes + d, (unsigned long long)ub);
    if (o.unit_chars && uc) atomicAdd((unsigned long long*)o.unit_chars + d, (unsigned long long)uc);
    if (nr) {
        if (o.n_dup) atomicAdd(o.n_dup + d, (int32_t)nr);
        if (o.dup_bytes && db) atomicAdd((unsigned long long*)o.dup_bytes + d, (unsigned long long)db);
        if (o.dup_chars && dc) atomicAdd((unsigned long long*)o.dup_chars + d, (unsigned long long)dc);
    }
}

unsigned strided_blocks(int64_t items) {
    const int64_t nb = (items + 255) / 256;
    return (unsigned)(nb < 1 ? 1 : nb < LN_MAX_BLOCKS ? nb : LN_MAX_BLOCKS);
}

}  // namespace

int64_t jtk_lines_tiles(int64_t n_bytes) { return (n_bytes + JTK_LN_TILE - 1) / JTK_LN_TILE; }

void jtk_launch_lines_count(const JtkLnWork& w, hipStream_t s) {
    const int64_t n_tiles = jtk_lines_tiles(w.n_bytes);
    hipLaunchKernelGGL(k_ln_mark, dim3(strided_blocks(w.n_docs + 1)), dim3(256), 0, s, w.doc_off, w.status, w.n_docs, w.n_bytes, w.edge, w.ref);
    if (n_tiles > 0) hipLaunchKernelGGL(k_ln_tile<false>, dim3((unsigned)n_tiles), dim3(LN_THREADS), 0, s, w);
    hipLaunchKernelGGL(k_ln_scan, dim3(1), dim3(SCAN_THREADS), 0, s, w, n_tiles);
}

void jtk_launch_lines_write(const JtkLnWork& w, uint64_t seed, uint64_t doc_index_base, hipStream_t s) {
    const int64_t n_tiles = jtk_lines_tiles(w.n_bytes);
    if (n_tiles > 0) hipLaunchKernelGGL(k_ln_tile<true>, dim3((unsigned)n_tiles), dim3(LN_THREADS), 0, s, w);
    hipLaunchKernelGGL(k_ln_docs, dim3(strided_blocks(w.n_docs + 1)), dim3(256), 0, s, w);
    if (w.n_units > 0)
        hipLaunchKernelGGL(k_ln_keys, dim3(jtk_blocks_for(w.n_units, 256)), dim3(256), 0, s, w, jtk_ln_key(seed, w.unit), doc_index_base);
}

void jtk_launch_lines_preset(const JtkLnWork& w, const JtkLnOut& o, uint64_t* top, hipStream_t s) {
    if (w.n_docs > 0 && (o.n_dup || o.dup_bytes || o.dup_chars || o.unit_bytes || o.unit_chars || top))
        hipLaunchKernelGGL(k_ln_preset, dim3(strided_blocks(w.n_docs)), dim3(256), 0, s, w.n_docs, o, top);
    if (o.unit_off || o.doc_chars)
        hipLaunchKernelGGL(k_ln_doc_out, dim3(strided_blocks(w.n_docs + 1)), dim3(256), 0, s, w.n_docs, w.unit_off, w.char_off, o.unit_off, o.doc_chars);
}

void jtk_launch_lines_group(const JtkLnWork& w, uint32_t flags, const JtkRpTable& t, int64_t lo, int64_t hi, const JtkLnOut& o, uint64_t* top,
                            hipStream_t s) {
    if (hi <= lo) return;
    const dim3 grid(jtk_blocks_for(hi - lo, 256));
    hipLaunchKernelGGL(k_ln_insert, grid, dim3(256), 0, s, (const uint64_t*)w.u_k, t, lo, hi);
    hipLaunchKernelGGL(k_ln_flags, grid, dim3(256), 0, s, w, flags & JTK_LINES_MARK_FIRST, t, lo, hi, o, top);
}
