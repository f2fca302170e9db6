// jtk_phrase.hip -- phrase hits of the last encode's text against a phrase set (jtk_batch_phrase_hits in jtk_abi.cpp), by the rule
// and the tables of jtk_phrase_rules.h.  Failureless Aho-Corasick: every start byte walks the trie on its own, and nearly every walk
// ends at its first test, a bit of LDS.  There is no failure link and no state that crosses a lane, hence no scan and no second pass.
//
//   k_ph_clear    0 into the masks and counts, "no hit" into the scratch of the first hits.
//   k_ph_scan     A workgroup of 256 lanes stages the two first-byte bitmaps and -- when it has at most JTK_PH_LDS_SLOTS slots -- the
//                 edge table into LDS ONCE and then takes tiles of 4096 bytes in a grid-stride loop (the tables are 12 times a tile:
//                 staged per tile they would be the pass).  Per tile: the tile with 16 bytes before and 80 behind it into LDS with
//                 16-byte loads, folded while stored when the set asks for it and zero behind the text, so that the walk and both
//                 boundary characters of every start byte of the tile are read from LDS and nowhere else.  A lane owns a granule of
//                 16 start positions and tests each against the bitmaps; the survivors are compacted in position order into the
//                 wave's queue in LDS (one wave scan of the counts), and the wave then walks one candidate per lane and round: text
//                 from LDS, edges by the probe of the rules header in LDS or L2.  At a terminal state the lane reads the state's 16
//                 bytes, tests the boundaries and the unit.  A lane keeps the sums of its current document and the mask of its
//                 current unit in registers and sends them when either changes; at the end of a tile a wave whose lanes all hold
//                 the same document reduces over the wave and sends one set of atomics: a text of "aaaa..." against {"a"} costs
//                 four sets of atomics per tile, not 4096.
//   k_ph_docs     the scratch into n_hits (saturated), first_hit and first_which.
//   k_ph_units    one lane per unit of the held list: n_hit_units, summed as k_wd_lines of jtk_words.hip does.
// Every barrier is reached by all threads of its workgroup (the tile loop's trip count is the workgroup's), and the shuffles and
// ballots are evaluated by all 64 lanes outside any condition.
#include "jtk_device_prims.h"
#include "jtk_kernels.h"
#include "jtk_lines_rules.h"
#include "jtk_phrase_rules.h"

namespace {

constexpr int PH_THREADS = JTK_PH_TILE / JTK_PH_GRANULE;
constexpr int PH_MAX_BLOCKS = 1024;
static_assert(PH_THREADS == 256 && JTK_PH_GRANULE == 16 && JTK_PH_WINDOW % 16 == 0, "a lane a granule, four waves a tile, the window in 16-byte loads");

__device__ __forceinline__ int64_t ph_clamp(int64_t v, int64_t n) { return v < 0 ? 0 : v > n ? n : v; }

struct PhWindow {                  // the staged bytes by batch position
    const uint8_t* s;
    int64_t base;
    __device__ __forceinline__ uint32_t operator[](int64_t i) const { return s[i - base]; }
};
struct PhFind {
    const JtkPhEdge* edges;
    uint32_t n_slots;
    __device__ __forceinline__ uint32_t operator()(uint32_t state, uint32_t byte) const { return jtk_ph_find(edges, n_slots, state, byte); }
};

__device__ __forceinline__ uint32_t ph_wave_or(uint32_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v |= (uint32_t)__shfl_xor((int)v, d);
    return v;
}
__device__ __forceinline__ uint64_t ph_wave_min(uint64_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint64_t o = __shfl_xor(v, d);
        v = o < v ? o : v;
    }
    return v;
}

__device__ __forceinline__ void ph_send(const JtkPhWork& w, int64_t d, uint32_t mask, uint32_t cnt, uint64_t first) {
    if (w.out.group_mask) atomicOr(w.out.group_mask + d, mask);
    atomicAdd((unsigned long long*)w.count + d, (unsigned long long)cnt);
    atomicMin((unsigned long long*)w.first + d, (unsigned long long)first);
}

__global__ void __launch_bounds__(256) k_ph_clear(JtkPhWork w) {
    const int64_t n = w.n_docs > w.n_units ? w.n_docs : w.n_units;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        if (i < w.n_docs) {
            w.first[i] = JTK_PH_NO_HIT;
            w.count[i] = 0;
            if (w.out.group_mask) w.out.group_mask[i] = 0;
            if (w.out.n_hit_units) w.out.n_hit_units[i] = 0;
        }
        if (w.umask && i < w.n_units) w.umask[i] = 0;
    }
}

template <bool LDS_TABLE>
__global__ void __launch_bounds__(PH_THREADS) k_ph_scan(JtkPhWork w, JtkPhSet set, int64_t n_tiles) {
    __shared__ __attribute__((aligned(16))) uint8_t s_text[JTK_PH_WINDOW];
    __shared__ __attribute__((aligned(16))) uint32_t s_first2[65536 / 32];
    __shared__ uint32_t s_first1[256 / 32];
    __shared__ uint16_t s_queue[PH_THREADS / 64][64 * JTK_PH_GRANULE];
    __shared__ __attribute__((aligned(16))) JtkPhEdge s_edge[LDS_TABLE ? JTK_PH_LDS_SLOTS : 1];
    __shared__ int64_t s_d[2];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;

    // the tables, once per workgroup
    for (int i = tid; i < 65536 / 32 / 4; i += PH_THREADS) reinterpret_cast<uint4*>(s_first2)[i] = reinterpret_cast<const uint4*>(set.first2)[i];
    if (tid < 256 / 32) s_first1[tid] = set.first1[tid];
    if (LDS_TABLE)
        for (uint32_t i = tid; i < set.n_slots; i += PH_THREADS) s_edge[i] = set.edges[i];
    const PhFind find{LDS_TABLE ? s_edge : set.edges, set.n_slots};
    const bool fold = set.flags & JTK_PHRASE_FOLD_ASCII, bounds = set.flags & JTK_PHRASE_WORD_BOUNDS;

    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t tile0 = tile * JTK_PH_TILE;
        __syncthreads();                                         // (the walks of the tile before are done with the window)
        for (int i = tid; i < JTK_PH_WINDOW / 16; i += PH_THREADS) {
            const int64_t pos = tile0 - JTK_PH_LEAD + (int64_t)i * 16, left = w.n_bytes - pos;
            uint32_t v[4] = {0, 0, 0, 0};
            if (pos >= 0 && left > 0) {                          // (the text is readable up to the next multiple of 16)
                const uint4 q = *reinterpret_cast<const uint4*>(w.text + pos);
                v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const int64_t keep = left - 4 * k;
                    if (keep < 4) v[k] = keep <= 0 ? 0u : v[k] & ((1u << (8 * (int)keep)) - 1u);
                    if (fold) v[k] = jtk_ph_fold32(v[k]);
                }
            }
            reinterpret_cast<uint4*>(s_text)[i] = make_uint4(v[0], v[1], v[2], v[3]);
        }
        if (lane == 0 && wv < 2) {                               // the documents of the tile's first and last byte
            const int64_t end = tile0 + JTK_PH_TILE < w.n_bytes ? tile0 + JTK_PH_TILE : w.n_bytes;
            s_d[wv] = jtk_ln_doc_at(w.doc_off, w.n_docs, wv ? end - 1 : tile0);
        }
        __syncthreads();

        // the granule's start positions against the bitmaps
        const uint8_t* const g = s_text + JTK_PH_LEAD + tid * JTK_PH_GRANULE;
        const uint4 q = *reinterpret_cast<const uint4*>(g);
        const uint32_t x5[5] = {q.x, q.y, q.z, q.w, (uint32_t)g[JTK_PH_GRANULE]};
        const int64_t left = w.n_bytes - (tile0 + tid * JTK_PH_GRANULE);
        const int valid = left >= JTK_PH_GRANULE ? JTK_PH_GRANULE : left > 0 ? (int)left : 0;
        uint32_t cand = 0;
#pragma unroll
        for (int i = 0; i < JTK_PH_GRANULE; i++) {
            const uint32_t b0 = (x5[i >> 2] >> (8 * (i & 3))) & 0xFFu, b1 = (x5[(i + 1) >> 2] >> (8 * ((i + 1) & 3))) & 0xFFu;
            bool c = jtk_ph_bit(s_first2, (b0 << 8) | b1);
            if (set.has1) c = c || jtk_ph_bit(s_first1, b0);
            if (c) cand |= 1u << i;
        }
        cand &= (1u << valid) - 1u;
        const uint32_t cnt = (uint32_t)__popc(cand), incl = jtk_wave_incl_scan(cnt);
        const uint32_t total = (uint32_t)__shfl((int)incl, 63);
        uint32_t at = incl - cnt;
        for (uint32_t m = cand; m; m &= m - 1u) s_queue[wv][at++] = (uint16_t)(tid * JTK_PH_GRANULE + __ffs((int)m) - 1);
        __syncthreads();                                         // (the queue is the wave's own; the barrier orders its stores and loads)

        // the walks: one candidate per lane and round, in position order, so a lane's documents and units only ascend
        const PhWindow x{s_text, tile0 - JTK_PH_LEAD};
        const int64_t d0 = s_d[0], d1 = s_d[1];
        int64_t cd = -1, ca = 0, ce = 0, uo0 = 0, uo1 = 0, cu = -1;
        bool cok = false;
        uint32_t acc_mask = 0, acc_cnt = 0, acc_um = 0;
        uint64_t acc_first = JTK_PH_NO_HIT;
        for (uint32_t r = lane; r < total; r += 64) {
            const int64_t p = tile0 + s_queue[wv][r];
            if (cd < 0 || p >= ce) {                             // another document
                if (acc_cnt) ph_send(w, cd, acc_mask, acc_cnt, acc_first);
                acc_mask = acc_cnt = 0; acc_first = JTK_PH_NO_HIT;
                const int64_t hi = d1 + 1 < w.n_docs + 1 ? d1 + 1 : w.n_docs + 1;
                cd = jtk_first_gt(w.doc_off, d0 + 1, hi, p) - 1;                 // (the last k with doc_off[k] <= p, d0 <= k <= d1)
                cok = false;
                if (cd < 0 || cd >= w.n_docs) { cd = -1; continue; }
                ca = ph_clamp(w.doc_off[cd], w.n_bytes); ce = ph_clamp(w.doc_off[cd + 1], w.n_bytes);
                cok = w.status[cd] >= 0 && ca <= p && p < ce;
                if (w.umask) { uo0 = ph_clamp(w.unit_off[cd], w.n_units); uo1 = ph_clamp(w.unit_off[cd + 1], w.n_units); }
                if (!(ca <= p && p < ce)) { cd = -1; continue; }
            }
            if (!cok) continue;
            int64_t u = -2;                                      // the unit that holds p: found at the position's first hit
            jtk_ph_walk(x, ce, p, find, [&](int len, uint32_t v) {
                if (bounds && !jtk_ph_bounded(x, w.uc, ca, ce, p, len)) return;
                const JtkPhInfo t = set.info[v & JTK_PH_V_STATE];
                acc_mask |= t.group_mask;
                acc_cnt++;
                const uint64_t key = jtk_ph_first_key(p - ca, t.index);
                acc_first = key < acc_first ? key : acc_first;
                if (!w.umask) return;
                if (u == -2) u = jtk_first_gt(w.u_begin, uo0, uo1, p) - 1;       // (the last unit of the document that begins at or before p)
                if (u < uo0 || p + len > w.u_end[u]) return;
                if (u != cu) {
                    if (acc_um) atomicOr(w.umask + cu, acc_um);
                    cu = u; acc_um = 0;
                }
                acc_um |= t.group_mask;
            });
        }
        if (acc_um) atomicOr(w.umask + cu, acc_um);
        // what the lanes still hold: one set of atomics for the wave when it is all one document's
        const bool pending = acc_cnt != 0;
        const uint64_t who = __ballot(pending);
        const int64_t d_first = __shfl(cd, who ? jtk_ctz64(who) : 0);
        const bool uniform = __ballot(pending && cd != d_first) == 0ull;
        const uint32_t all_mask = ph_wave_or(acc_mask), all_cnt = jtk_wave_sum(acc_cnt);
        const uint64_t all_first = ph_wave_min(acc_first);
        if (uniform) {
            if (who && lane == jtk_ctz64(who)) ph_send(w, cd, all_mask, all_cnt, all_first);
        } else if (pending) {
            ph_send(w, cd, acc_mask, acc_cnt, acc_first);
        }
    }
}

__global__ void __launch_bounds__(256) k_ph_docs(JtkPhWork w) {
    for (int64_t d = (int64_t)blockIdx.x * 256 + threadIdx.x; d < w.n_docs; d += (int64_t)gridDim.x * 256) {
        const uint64_t key = w.first[d], c = w.count[d];
        if (w.out.n_hits) w.out.n_hits[d] = c > 0x7FFFFFFFull ? 0x7FFFFFFF : (int32_t)c;
        if (w.out.first_hit) w.out.first_hit[d] = key == JTK_PH_NO_HIT ? -1 : (int64_t)(key >> 16);
        if (w.out.first_which) w.out.first_which[d] = key == JTK_PH_NO_HIT ? -1 : (int32_t)(key & 0xFFFFu);
    }
}

// A wave whose units are all one document's adds its count once, from lane 0; a wave that holds several documents adds per lane.
__global__ void __launch_bounds__(256) k_ph_units(JtkPhWork w) {
    const int lane = threadIdx.x & 63;
    const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool live = u < w.n_units;
    const int64_t d = live ? jtk_ln_doc_of_unit(w.unit_off, w.n_docs, u) : -1;
    const uint32_t mine = live && w.umask[u] ? 1u : 0u;
    const int64_t d_first = __shfl(d, 0);
    const bool uniform = __ballot(live && d != d_first) == 0ull;
    const uint32_t all = jtk_wave_sum(mine);
    if (!live || d < 0 || d >= w.n_docs || (uniform && lane != 0)) return;
    const uint32_t v = uniform ? all : mine;
    if (v) atomicAdd(w.out.n_hit_units + d, (int32_t)v);
}

unsigned strided_blocks(int64_t items) {
    const int64_t nb = (items + 255) / 256;
    return (unsigned)(nb < 1 ? 1 : nb < PH_MAX_BLOCKS ? nb : PH_MAX_BLOCKS);
}

}  // namespace

void jtk_launch_phrase_clear(const JtkPhWork& w, hipStream_t s) {
    hipLaunchKernelGGL(k_ph_clear, dim3(strided_blocks(w.n_docs > w.n_units ? w.n_docs : w.n_units)), dim3(256), 0, s, w);
}

void jtk_launch_phrase_scan(const JtkPhWork& w, const JtkPhSet& set, hipStream_t s) {
    const int64_t n_tiles = (w.n_bytes + JTK_PH_TILE - 1) / JTK_PH_TILE;
    if (n_tiles <= 0) return;
    const unsigned blocks = (unsigned)(n_tiles < PH_MAX_BLOCKS ? n_tiles : PH_MAX_BLOCKS);
    if (set.n_slots <= JTK_PH_LDS_SLOTS) hipLaunchKernelGGL(k_ph_scan<true>, dim3(blocks), dim3(PH_THREADS), 0, s, w, set, n_tiles);
    else hipLaunchKernelGGL(k_ph_scan<false>, dim3(blocks), dim3(PH_THREADS), 0, s, w, set, n_tiles);
}

void jtk_launch_phrase_close(const JtkPhWork& w, hipStream_t s) {
    if (w.out.n_hits || w.out.first_hit || w.out.first_which) hipLaunchKernelGGL(k_ph_docs, dim3(strided_blocks(w.n_docs)), dim3(256), 0, s, w);
    if (w.out.n_hit_units && w.n_units > 0) hipLaunchKernelGGL(k_ph_units, dim3(jtk_blocks_for(w.n_units, 256)), dim3(256), 0, s, w);
}
