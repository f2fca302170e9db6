// jtk_seen.hip -- exact duplicates across documents and batches (jtk_seen_set_* / jtk_batch_seen_mark in jtk_abi.cpp), by the
// rule of jtk_seen_rules.h.  The units come from the walk of jtk_lines.hip (jtk_launch_lines_count / jtk_launch_lines_walk) on a
// JtkLnWork of this pass's own, with the threshold of the set's unit; everything behind the walk is here.  Integer only: the
// results are bit-exact.  Every barrier is reached by all threads of its workgroup, and the shuffles are evaluated by all 64 lanes
// outside any condition.
//
//   k_sn_keys      one lane per unit: H from the two prefixes, the unsalted k, chars, and pos from unit_off by one search; the
//                  largest document-relative index + 1 of the batch by a wave maximum and one atomicMax per wave.
//   k_sn_add<1>    entries (key, first, count) into the table -- the units of a batch (count NULL: 1 each), the live slots of the
//                  old planes at a growth (key 0 skipped), entries from the host.  A workgroup takes SN_ITEMS entries and first
//                  merges them in an LDS table of SN_LDS slots (CAS on the key, 64-bit min and add in LDS); behind a barrier every
//                  occupied LDS slot goes to memory once: claim by CAS on the key plane, atomicMin on first, atomicAdd on count.
//                  Whoever wins a claim bumps the key counter, summed over the wave first.  A batch that is one line m times
//                  sends ceil(m / SN_ITEMS) triples of atomics to the line's slot, not m.
//   k_sn_add<0>    the same without the LDS stage: one triple of atomics per entry (JTK_SEEN_NO_COMBINE, for measuring).
//   k_sn_preset    the per-document sums = 0, unit_off out of the walk's.
//   k_sn_query     one lane per unit: its entry, the per-unit outputs and the flag; the per-document sums as k_ln_flags adds them
//                  (a wave whose units are all one document's adds once, from lane 0).
//   k_sn_entries   a workgroup takes 256 slots: occupancy, the exclusive prefix inside the workgroup, one atomicAdd on the output
//                  cursor, and the live slots' (key, first, count) behind it.  In no particular order.
#include "jtk_device_prims.h"
#include "jtk_kernels.h"
#include "jtk_seen_rules.h"

namespace {

constexpr int SN_THREADS = 256;
constexpr int SN_PER = 2;                          // entries per lane of k_sn_add
constexpr int SN_ITEMS = SN_THREADS * SN_PER;      // entries per workgroup
constexpr int SN_LDS = 2 * SN_ITEMS;               // LDS slots: a load of at most 1/2, so every walk meets an empty slot or its key
constexpr int SN_MAX_BLOCKS = 4096;
static_assert((SN_LDS & (SN_LDS - 1)) == 0 && SN_LDS * JTK_SN_SLOT_BYTES <= 32768, "a power of two of slots within 32 KiB of LDS");

struct DevCas {
    __device__ uint64_t operator()(uint64_t* p, uint64_t k) const {
        return (uint64_t)atomicCAS((unsigned long long*)p, 0ull, (unsigned long long)k);
    }
};

__device__ __forceinline__ uint64_t sn_wave_max(uint64_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint64_t o = __shfl_xor(v, d);
        v = o > v ? o : v;
    }
    return v;
}

__global__ void __launch_bounds__(SN_THREADS) k_sn_keys(JtkLnWork w, uint64_t key, uint64_t base, uint64_t* __restrict__ u_pos,
                                                        int64_t* __restrict__ max_doc_units) {
    const int64_t u = (int64_t)blockIdx.x * SN_THREADS + threadIdx.x;
    uint64_t mine = 0;                                           // this unit's document-relative index + 1
    if (u < w.n_units) {
        const int64_t b = w.u_begin[u], e = w.u_end[u];
        const int64_t d = jtk_ln_doc_of_unit(w.unit_off, w.n_docs, u);
        const int64_t rel = u - w.unit_off[d];
        w.u_k[u] = jtk_ln_finish(jtk_ln_range_hash(w.u_k[u], w.u_pe[u], e - b), key);
        w.u_chars[u] = w.u_ce[u] - w.u_chars[u];
        u_pos[u] = jtk_sn_pos(base, d, rel);
        mine = (uint64_t)rel + 1ull;
    }
    const uint64_t top = sn_wave_max(mine);
    if ((threadIdx.x & 63) == 0 && top) atomicMax((unsigned long long*)max_doc_units, (unsigned long long)top);
}

// one entry into the table in memory; returns 1 when its key was new
__device__ __forceinline__ uint32_t sn_put(const JtkSnTable& t, uint64_t k, uint64_t first, uint64_t count) {
    bool fresh;
    const uint64_t slot = jtk_sn_claim(t.key, t.mask, k, DevCas(), &fresh);
    atomicMin((unsigned long long*)t.first + slot, (unsigned long long)first);
    atomicAdd((unsigned long long*)t.count + slot, (unsigned long long)count);
    return fresh ? 1u : 0u;
}

template <bool COMBINE>
__global__ void __launch_bounds__(SN_THREADS) k_sn_add(const uint64_t* __restrict__ keys, const uint64_t* __restrict__ first,
                                                       const uint64_t* __restrict__ count, int64_t n, JtkSnTable t, uint64_t* __restrict__ n_keys) {
    __shared__ uint64_t s_key[COMBINE ? SN_LDS : 1], s_first[COMBINE ? SN_LDS : 1], s_count[COMBINE ? SN_LDS : 1];
    const int tid = threadIdx.x;
    uint32_t fresh = 0;
    for (int64_t i0 = (int64_t)blockIdx.x * SN_ITEMS; i0 < n; i0 += (int64_t)gridDim.x * SN_ITEMS) {     // (uniform in the workgroup)
        if (COMBINE) {
            for (int i = tid; i < SN_LDS; i += SN_THREADS) { s_key[i] = 0; s_first[i] = JTK_SN_ABSENT; s_count[i] = 0; }
            __syncthreads();
        }
#pragma unroll
        for (int j = 0; j < SN_PER; j++) {
            const int64_t i = i0 + (int64_t)j * SN_THREADS + tid;
            const uint64_t k = i < n ? keys[i] : 0ull;
            if (!k) continue;                                    // (an empty slot of the old planes)
            const uint64_t f = first[i], c = count ? count[i] : 1ull;
            if (COMBINE) {
                bool unused;
                const uint64_t slot = jtk_sn_claim(s_key, (uint64_t)SN_LDS - 1, k, DevCas(), &unused);
                atomicMin((unsigned long long*)s_first + slot, (unsigned long long)f);
                atomicAdd((unsigned long long*)s_count + slot, (unsigned long long)c);
            } else {
                fresh += sn_put(t, k, f, c);
            }
        }
        if (COMBINE) {
            __syncthreads();
            for (int i = tid; i < SN_LDS; i += SN_THREADS)
                if (s_key[i]) fresh += sn_put(t, s_key[i], s_first[i], s_count[i]);
            __syncthreads();                                     // (the next round clears the LDS table)
        }
    }
    const uint32_t won = jtk_wave_sum(fresh);
    if (n_keys && (tid & 63) == 0 && won) atomicAdd((unsigned long long*)n_keys, (unsigned long long)won);
}

__global__ void __launch_bounds__(256) k_sn_preset(int64_t n_docs, const int64_t* __restrict__ unit_off, JtkSnOut o) {
    for (int64_t d = (int64_t)blockIdx.x * 256 + threadIdx.x; d <= n_docs; d += (int64_t)gridDim.x * 256) {
        if (o.unit_off) o.unit_off[d] = unit_off[d];
        if (d == n_docs) continue;
        if (o.n_dup) o.n_dup[d] = 0;
        if (o.dup_bytes) o.dup_bytes[d] = 0;
        if (o.dup_chars) o.dup_chars[d] = 0;
        if (o.unit_bytes) o.unit_bytes[d] = 0;
        if (o.unit_chars) o.unit_chars[d] = 0;
    }
}

__global__ void __launch_bounds__(256) k_sn_query(JtkLnWork w, const uint64_t* __restrict__ u_pos, uint64_t base, JtkSnTable t, uint64_t min_count,
                                                  JtkSnOut o) {
    const int lane = threadIdx.x & 63;
    const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool live = u < w.n_units;
    bool dup = false;
    int64_t d = -1, bytes = 0, chars = 0;
    if (live) {
        const uint64_t k = w.u_k[u], pos = u_pos[u];
        const uint64_t slot = jtk_rp_find(t.key, t.mask, k);
        const bool have = t.key[slot] == k;
        const uint64_t first = have ? t.first[slot] : JTK_SN_ABSENT, count = have ? t.count[slot] : 0ull;
        const uint32_t flag = jtk_sn_flag(first, count, pos, min_count);
        dup = (flag & JTK_SEEN_DUP) != 0;
        const int64_t b = w.u_begin[u], e = w.u_end[u];
        if (o.unit_begin) o.unit_begin[u] = b;
        if (o.unit_end) o.unit_end[u] = e;
        if (o.unit_first) o.unit_first[u] = first;
        if (o.unit_count) o.unit_count[u] = count;
        if (o.unit_flags) o.unit_flags[u] = (uint8_t)flag;
        d = (int64_t)((pos >> JTK_SN_UNIT_BITS) - base);         // (pos holds doc_index_base + d)
        bytes = e - b;
        chars = w.u_chars[u];
    }
    const int64_t d0 = __shfl(d, 0);
    const bool uniform = __ballot(live && d != d0) == 0ull;
    const int64_t all_bytes = jtk_wave_sum(bytes), all_chars = jtk_wave_sum(chars);
    const int64_t dup_bytes = jtk_wave_sum(dup ? bytes : (int64_t)0), dup_chars = jtk_wave_sum(dup ? chars : (int64_t)0);
    const uint32_t dups = jtk_wave_sum(dup ? 1u : 0u);
    if (!live || (uniform && lane != 0)) return;
    const int64_t ub = uniform ? all_bytes : bytes, uc = uniform ? all_chars : chars;
    const int64_t db = uniform ? dup_bytes : (dup ? bytes : 0), dc = uniform ? dup_chars : (dup ? chars : 0);
    const uint32_t nr = uniform ? dups : (dup ? 1u : 0u);
    if (o.unit_bytes && ub) atomicAdd((unsigned long long*)o.unit_bytes + d, (unsigned long long)ub);
    if (o.unit_chars && uc) atomicAdd((unsigned long long*)o.unit_chars + d, (unsigned long long)uc);
    if (nr) {
        if (o.n_dup) atomicAdd(o.n_dup + d, (int32_t)nr);
        if (o.dup_bytes && db) atomicAdd((unsigned long long*)o.dup_bytes + d, (unsigned long long)db);
        if (o.dup_chars && dc) atomicAdd((unsigned long long*)o.dup_chars + d, (unsigned long long)dc);
    }
}

__global__ void __launch_bounds__(256) k_sn_entries(JtkSnTable t, uint64_t* __restrict__ keys, uint64_t* __restrict__ first,
                                                    uint64_t* __restrict__ count, int64_t cap, uint64_t* __restrict__ cursor) {
    __shared__ uint64_t s_base;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const uint64_t k = (uint64_t)i <= t.mask ? t.key[i] : 0ull;
    uint32_t total;
    const uint32_t pre = jtk_block_excl_prefix<256>(k ? 1u : 0u, &total);        // (a barrier)
    if (threadIdx.x == 0) s_base = total ? (uint64_t)atomicAdd((unsigned long long*)cursor, (unsigned long long)total) : 0ull;
    __syncthreads();
    const int64_t at = (int64_t)(s_base + pre);
    if (k && at < cap) { keys[at] = k; first[at] = t.first[i]; count[at] = t.count[i]; }
}

unsigned strided_blocks(int64_t items, int per) {
    const int64_t nb = (items + per - 1) / per;
    return (unsigned)(nb < 1 ? 1 : nb < SN_MAX_BLOCKS ? nb : SN_MAX_BLOCKS);
}

}  // namespace

void jtk_launch_seen_keys(const JtkLnWork& w, uint64_t key, uint64_t doc_index_base, uint64_t* u_pos, int64_t* max_doc_units, hipStream_t s) {
    if (w.n_units > 0)
        hipLaunchKernelGGL(k_sn_keys, dim3(jtk_blocks_for(w.n_units, SN_THREADS)), dim3(SN_THREADS), 0, s, w, key, doc_index_base, u_pos, max_doc_units);
}

void jtk_launch_seen_add(const uint64_t* keys, const uint64_t* first, const uint64_t* count_or_null, int64_t n, const JtkSnTable& t,
                         uint64_t* n_keys_or_null, bool combine, hipStream_t s) {
    if (n <= 0) return;
    const dim3 grid(strided_blocks(n, SN_ITEMS));
    if (combine) hipLaunchKernelGGL(k_sn_add<true>, grid, dim3(SN_THREADS), 0, s, keys, first, count_or_null, n, t, n_keys_or_null);
    else hipLaunchKernelGGL(k_sn_add<false>, grid, dim3(SN_THREADS), 0, s, keys, first, count_or_null, n, t, n_keys_or_null);
}

void jtk_launch_seen_query(const JtkLnWork& w, const uint64_t* u_pos, uint64_t doc_index_base, const JtkSnTable& t, uint64_t min_count,
                           const JtkSnOut& o, hipStream_t s) {
    hipLaunchKernelGGL(k_sn_preset, dim3(strided_blocks(w.n_docs + 1, 256)), dim3(256), 0, s, w.n_docs, (const int64_t*)w.unit_off, o);
    if (w.n_units > 0)
        hipLaunchKernelGGL(k_sn_query, dim3(jtk_blocks_for(w.n_units, 256)), dim3(256), 0, s, w, u_pos, doc_index_base, t, min_count, o);
}

void jtk_launch_seen_entries(const JtkSnTable& t, uint64_t* keys, uint64_t* first, uint64_t* count, int64_t cap, uint64_t* cursor, hipStream_t s) {
    hipLaunchKernelGGL(k_sn_entries, dim3(jtk_blocks_for((int64_t)t.mask + 1, 256)), dim3(256), 0, s, t, keys, first, count, cap, cursor);
}
