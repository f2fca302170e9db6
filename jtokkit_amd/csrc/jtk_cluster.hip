// jtk_cluster.hip -- near-duplicate clusters out of MinHash signatures and LSH band keys (jtk_batch_minhash_cluster in
// jtk_abi.cpp), by the rule of jtk_cluster_rules.h.  No sort, no host round trip; integer only: the results are bit-exact and do
// not depend on the order in which waves run.
//
//   k_cl_preset     labels[d] = d.  labels is the union-find's parent array until k_cl_labels has run; a kernel of its own,
//                   queued before k_cl_verify: "the first wave to touch d presets it" would be a race between workgroups.
//   k_cl_insert     one lane per (document, band of the group); consecutive lanes take the consecutive keys of a document.  A
//                   live document claims its key's slot in the band's table (jtk_rp_claim: a 64-bit atomicCAS walk) -- the key 0
//                   has the band's side cell instead -- and takes a 64-bit atomicMin of d into the slot's value.
//   k_cl_probe      the same lanes, after all inserts of the group: rep[d][j] = the value of the key's slot, -1 for a document
//                   that is not live.
//   k_cl_verify<VEC> one wave per live document d.  The wave loads sig[d] into registers once -- one 16-byte load per lane (VEC:
//                   K a multiple of 4 and sig 16-byte aligned, so every row is; K <= 256 makes one load cover the row) or up to
//                   four words per lane --, then takes the bands 64 at a time, a lane a band.  Among the lanes whose rep is an
//                   earlier document the wave picks the lowest, broadcasts its e, and strikes every lane that holds the same e: a
//                   bucket shared in many bands is verified once.  Lane 0 looks up the roots of d and e; where they are the same
//                   the pair is skipped (the two are joined already: the edge adds nothing to any component).  Otherwise all
//                   lanes load row e, compare and take a wave sum, and on >= min_agree lane 0 hooks the two components.
//                   Every ballot, shuffle and wave sum is reached by all 64 lanes: the conditions around them (the document, the
//                   ballot's mask, lane 0's verdict read back with readfirstlane) are the same in every lane.
//   k_cl_labels     labels[d] = the root of d, one lane per document, in place.
//
// The union-find.  parent[x] <= x always: a hook is atomicCAS(&parent[hi], hi, lo) with lo < hi, both roots as far as the lane has
// seen; it succeeds only while hi still is a root, and otherwise returns hi's new parent, from which the lane goes on.  So chains
// strictly descend, there is no cycle, and a component's root is its smallest index whatever the order of the hooks.
// Path halving stores with plain (relaxed) stores: find writes parent[x] = g only after it read parent[x] = p != x and parent[p]
// = g.  (1) x was no root then and a node never becomes a root again, so the store cannot undo a hook: hooks only succeed on
// roots.  (2) g was an ancestor of x then, and "is an ancestor of" only ever gains pairs -- a hook adds ancestors, a halving
// store replaces an edge to an ancestor by an edge to a farther one, and p keeps its own edge towards g --, so a store that
// lands late, over a newer and farther value, still leaves x below an ancestor: the component is the same and the chain still
// descends.  Parents are read with relaxed device-scope atomic loads: another wave's hook may be missed, which costs a verify
// that was not needed or one more round of the hook's loop, and never a result.
#include "jtk_kernels.h"
#include "jtk_cluster_rules.h"

namespace {

constexpr int CL_MAX_BLOCKS = 4096;                              // the kernels stride

struct DevCas {
    __device__ uint64_t operator()(uint64_t* p, uint64_t k) const {
        return (uint64_t)atomicCAS((unsigned long long*)p, 0ull, (unsigned long long)k);
    }
};

__device__ __forceinline__ int64_t cl_parent(const int64_t* parent, int64_t x) {
    return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void cl_set_parent(int64_t* parent, int64_t x, int64_t p) {
    __hip_atomic_store(parent + x, p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// the root of x as far as this lane sees it, halving the path on the way (the argument is at the top of the file)
__device__ int64_t cl_find(int64_t* parent, int64_t x) {
    for (;;) {
        const int64_t p = cl_parent(parent, x);
        if (p == x) return x;
        const int64_t g = cl_parent(parent, p);
        if (g == p) return p;
        cl_set_parent(parent, x, g);
        x = g;
    }
}
__device__ void cl_hook(int64_t* parent, int64_t a, int64_t b) {
    for (;;) {
        a = cl_find(parent, a);
        b = cl_find(parent, b);
        if (a == b) return;
        const int64_t hi = a > b ? a : b, lo = a > b ? b : a;
        const int64_t seen = (int64_t)atomicCAS((unsigned long long*)parent + hi, (unsigned long long)hi, (unsigned long long)lo);
        if (seen == hi) return;
        a = seen;                                                // hi was hooked meanwhile: go on from its parent
        b = lo;
    }
}

__global__ void __launch_bounds__(256) k_cl_preset(int64_t n, int64_t* __restrict__ labels) {
    for (int64_t d = (int64_t)blockIdx.x * 256 + threadIdx.x; d < n; d += (int64_t)gridDim.x * 256) labels[d] = d;
}

__global__ void __launch_bounds__(256) k_cl_insert(const uint64_t* __restrict__ band_keys, const int32_t* __restrict__ n_shingles, int64_t n,
                                                   int32_t B, int32_t j0, int32_t g, JtkClTable t) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n * g; i += (int64_t)gridDim.x * 256) {
        const int64_t d = i / g;
        const int32_t jj = (int32_t)(i - d * g);
        if (!jtk_cl_live(n_shingles, d)) continue;
        uint64_t* const cell = jtk_cl_cell_claim(t, jj, band_keys[d * B + j0 + jj], DevCas());
        atomicMin((unsigned long long*)cell, (unsigned long long)d);
    }
}

__global__ void __launch_bounds__(256) k_cl_probe(const uint64_t* __restrict__ band_keys, const int32_t* __restrict__ n_shingles, int64_t n,
                                                  int32_t B, int32_t j0, int32_t g, JtkClTable t, int64_t* __restrict__ rep) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n * g; i += (int64_t)gridDim.x * 256) {
        const int64_t d = i / g;
        const int32_t jj = (int32_t)(i - d * g);
        const int64_t at = d * B + j0 + jj;
        rep[at] = jtk_cl_live(n_shingles, d) ? (int64_t)*jtk_cl_cell_find(t, jj, band_keys[at]) : -1;
    }
}

// a lane's share of a row: words 4 lane .. 4 lane + 3 (VEC) or words lane, lane + 64, lane + 128, lane + 192; 0 past K
template <bool VEC>
__device__ __forceinline__ uint4 cl_row(const uint32_t* __restrict__ row, int32_t K, int lane) {
    uint4 q = make_uint4(0, 0, 0, 0);
    if (VEC) {
        if (4 * lane < K) q = *(const uint4*)(row + 4 * lane);
    } else {
        if (lane < K) q.x = row[lane];
        if (lane + 64 < K) q.y = row[lane + 64];
        if (lane + 128 < K) q.z = row[lane + 128];
        if (lane + 192 < K) q.w = row[lane + 192];
    }
    return q;
}
// on how many of the lane's words two rows agree (the words past K do not count)
template <bool VEC>
__device__ __forceinline__ uint32_t cl_agree(const uint4& a, const uint4& b, int32_t K, int lane) {
    if (VEC) return 4 * lane < K ? (a.x == b.x) + (a.y == b.y) + (a.z == b.z) + (a.w == b.w) : 0u;
    return (lane < K && a.x == b.x) + (lane + 64 < K && a.y == b.y) + (lane + 128 < K && a.z == b.z) + (lane + 192 < K && a.w == b.w);
}

template <bool VEC>
__global__ void __launch_bounds__(256) k_cl_verify(const uint32_t* __restrict__ sig, const int32_t* __restrict__ n_shingles,
                                                   const int64_t* __restrict__ rep, int64_t n, int32_t K, int32_t B, uint32_t min_agree,
                                                   int64_t* parent) {
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (int64_t d = (int64_t)blockIdx.x * 4 + wv; d < n; d += (int64_t)gridDim.x * 4) {       // (d is the same in all lanes)
        if (!jtk_cl_live(n_shingles, d)) continue;
        const uint4 mine = cl_row<VEC>(sig + d * K, K, lane);
        for (int32_t j0 = 0; j0 < B; j0 += 64) {
            const int64_t e = j0 + lane < B ? rep[d * B + j0 + lane] : -1;
            uint64_t todo = __ballot(e >= 0 && e < d);
            while (todo) {                                                                   // (the same in all lanes)
                const int64_t e0 = __shfl(e, __ffsll((unsigned long long)todo) - 1);
                todo &= ~__ballot(e == e0);
                int joined = 0;
                if (lane == 0) joined = cl_find(parent, d) == cl_find(parent, e0);
                if (__builtin_amdgcn_readfirstlane(joined)) continue;
                const uint4 other = cl_row<VEC>(sig + e0 * K, K, lane);
                const uint32_t agree = jtk_wave_sum(cl_agree<VEC>(mine, other, K, lane));
                if (lane == 0 && agree >= min_agree) cl_hook(parent, d, e0);
            }
        }
    }
}

__global__ void __launch_bounds__(256) k_cl_labels(int64_t n, int64_t* labels) {
    for (int64_t d = (int64_t)blockIdx.x * 256 + threadIdx.x; d < n; d += (int64_t)gridDim.x * 256) {
        // no hook runs any more: a root stays one, and a lane that reads labels[d] finds d's old parent or its root, an ancestor both
        int64_t x = d;
        for (int64_t p = cl_parent(labels, x); p != x; p = cl_parent(labels, x)) x = p;
        cl_set_parent(labels, d, x);
    }
}

unsigned strided_blocks(int64_t items, int per) {
    const int64_t nb = (items + per - 1) / per;
    return (unsigned)(nb < 1 ? 1 : nb < CL_MAX_BLOCKS ? nb : CL_MAX_BLOCKS);
}

}  // namespace

void jtk_launch_cluster_preset(int64_t n, int64_t* labels, hipStream_t s) {
    hipLaunchKernelGGL(k_cl_preset, dim3(strided_blocks(n, 256)), dim3(256), 0, s, n, labels);
}

void jtk_launch_cluster_group(const uint64_t* band_keys, const int32_t* n_shingles, int64_t n, int32_t bands, int32_t j0, int32_t g,
                              const JtkClTable& t, int64_t* rep, hipStream_t s) {
    const dim3 grid(strided_blocks(n * g, 256)), block(256);
    hipLaunchKernelGGL(k_cl_insert, grid, block, 0, s, band_keys, n_shingles, n, bands, j0, g, t);
    hipLaunchKernelGGL(k_cl_probe, grid, block, 0, s, band_keys, n_shingles, n, bands, j0, g, t, rep);
}

void jtk_launch_cluster_join(const uint32_t* sig, const int32_t* n_shingles, const int64_t* rep, int64_t n, int32_t num_hashes, int32_t bands,
                             int32_t min_agree, int64_t* labels, hipStream_t s) {
    const dim3 grid(strided_blocks(n, 4)), block(256);
    if (num_hashes % 4 == 0 && ((uintptr_t)sig & 15u) == 0)
        hipLaunchKernelGGL(k_cl_verify<true>, grid, block, 0, s, sig, n_shingles, rep, n, num_hashes, bands, (uint32_t)min_agree, labels);
    else
        hipLaunchKernelGGL(k_cl_verify<false>, grid, block, 0, s, sig, n_shingles, rep, n, num_hashes, bands, (uint32_t)min_agree, labels);
    hipLaunchKernelGGL(k_cl_labels, dim3(strided_blocks(n, 256)), dim3(256), 0, s, n, labels);
}
