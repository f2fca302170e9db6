// jtk_utf16.hip -- UTF-16 in and out on the device (jtk_batch_transcode_utf16_device / _encode_utf16* / _decode_utf16 in
// jtk_abi.cpp).  Both rules, and a lane's whole work in either pass, are jtk_utf16_rules.h (shared with tests/utf16_sim).
//
// Either direction is count -> scan -> write over fixed tiles of 256 lanes, one coalesced 16-byte load per lane (E: 8 units,
// D: 16 bytes):
//   count     the lane's output count: a granule of units below 0x80 (E) or bytes below 0x80 (D) is recognised on its OR-ed words
//             and counts 8 / 16; any other granule goes unit by unit / byte by byte.  The unit before and after the granule
//             (E), the 4 bytes before and after it (D) come from the neighbour lanes' registers by shuffle; the first and the
//             last lane of a wave take them with one guarded load.  jtk_block_excl_prefix gives the lane's place in its tile
//             (sub, uint16 per lane) and the tile's total.  The E count pass also checks the caller's offsets.
//   scan      jtk_launch_scan_u32 over the tile totals
//   write     the lane's output again, into the tile's LDS stage at the byte it has in its 16-byte granule of the output; after
//             one barrier the tile's granules leave as 16-byte stores, the ragged first and last granule byte by byte
//   offsets   doc_off[d] / unit_off[q] = tile_off + sub + the part of one lane before the position: one lane per offset
// Document edges matter only to a surrogate next to its partner (E) and to bytes >= 0x80 within 3 of an edge (D): one
// jtk_first_gt over the offsets by the lanes that hold such a unit or byte, none by the others.
#include "jtk_utf16_rules.h"
#include "jtk_device_prims.h"
#include "jtk_kernels.h"

namespace {

constexpr int UL = JTK_U16_LANES;
static_assert(UL == 256 && JTK_U16_E_PER_LANE * 2 == 16 && JTK_U16_D_PER_LANE == 16, "a lane holds one 16-byte granule");
static_assert(JTK_U16_E_TILE * 3 < 65536 && JTK_U16_D_TILE < 65536, "a lane's place in its tile fits the uint16 of sub");

__device__ __forceinline__ int64_t u16_clamp(int64_t v, int64_t n) { return v < 0 ? 0 : v > n ? n : v; }

// ---- E ------------------------------------------------------------------------------------------------------------------
// units g0 .. g0 + 7; ALIGNED: one 16-byte load (the granule that holds unit g0 < n_units), else unit by unit below n_units
template <bool ALIGNED>
__device__ __forceinline__ JtkU16Quad e_load(const uint16_t* units, int64_t n_units, int64_t g0) {
    JtkU16Quad g{};
    if (g0 >= n_units) return g;
    if (ALIGNED) return *reinterpret_cast<const JtkU16Quad*>(units + g0);
#pragma unroll
    for (int k = 0; k < JTK_U16_E_PER_LANE; k++)
        if (g0 + k < n_units) g.w[k >> 1] |= (uint32_t)units[g0 + k] << (16 * (k & 1));
    return g;
}

struct EEdge {                  // unit x is one of unit_off[0 .. n_docs]
    const int64_t* off;
    int64_t n_docs;
    __device__ bool operator()(int64_t x) const {
        const int64_t k = jtk_first_gt(off, 0, n_docs + 1, x - 1);     // the first offset >= x
        return k <= n_docs && off[k] == x;
    }
};

// a lane of a tile in either pass.  Called by all 64 lanes of every wave, outside any condition (it shuffles).
template <bool ALIGNED>
__device__ __forceinline__ uint32_t e_tile_lane(const JtkU16EncWork& w, int64_t lo, int64_t hi, int64_t g0, uint8_t* out) {
    const int lane = threadIdx.x & 63;
    const JtkU16Quad g = e_load<ALIGNED>(w.units, w.n_units, g0);
    uint32_t prev = (uint32_t)__shfl_up((int)g.w[3], 1) >> 16;
    uint32_t next = (uint32_t)__shfl_down((int)g.w[0], 1) & 0xFFFFu;
    if (lane == 0) prev = (g0 > 0 && g0 - 1 < w.n_units) ? w.units[g0 - 1] : 0u;
    if (lane == 63) next = (g0 + JTK_U16_E_PER_LANE < w.n_units) ? w.units[g0 + JTK_U16_E_PER_LANE] : 0u;
    return jtk_u16_e_lane(g, prev, next, g0, lo, hi, EEdge{w.unit_off, w.n_docs}, out);
}

template <bool ALIGNED>
__global__ void __launch_bounds__(256) k_u16_e_count(JtkU16EncWork w) {
    // the caller's offsets: start at or above 0, never decrease, end at or below n_units
    for (int64_t d = (int64_t)blockIdx.x * UL + threadIdx.x; d <= w.n_docs; d += (int64_t)gridDim.x * UL) {
        const int64_t v = w.unit_off[d];
        if (v < 0 || v > w.n_units || (d < w.n_docs && w.unit_off[d + 1] < v)) w.hdr[1] = 1;
    }
    const int64_t tile = blockIdx.x;
    const int64_t lo = u16_clamp(w.unit_off[0], w.n_units), hi = u16_clamp(w.unit_off[w.n_docs], w.n_units);
    const uint32_t cnt = e_tile_lane<ALIGNED>(w, lo, hi, tile * JTK_U16_E_TILE + threadIdx.x * JTK_U16_E_PER_LANE, nullptr);
    uint32_t total;
    const uint32_t pre = jtk_block_excl_prefix<UL>(cnt, &total);
    if (tile >= w.n_tiles) return;                                        // (a batch without units: one idle workgroup)
    w.sub[tile * UL + threadIdx.x] = (uint16_t)pre;
    if (threadIdx.x == 0) w.tile_cnt[tile] = total;
}

// The tile's output, staged in LDS from byte `shift` = (its first byte's offset) % 16 on, to dst[base, base + n): whole 16-byte
// granules of dst as one store each, the ragged first and last one byte by byte (their other bytes are the neighbour tiles').
// dst is 16-byte aligned.  Behind a barrier of the caller's.
__device__ __forceinline__ void u16_flush(const uint8_t* stage, uint8_t* dst, int64_t base, uint32_t n) {
    const uint32_t shift = (uint32_t)(base & 15), end = shift + n;
    uint8_t* const d0 = dst + (base - shift);
    for (uint32_t k = threadIdx.x; k * 16 < end; k += UL) {
        const uint32_t a = k * 16, e = a + 16;
        if (a >= shift && e <= end) {
            *reinterpret_cast<uint4*>(d0 + a) = *reinterpret_cast<const uint4*>(stage + a);
        } else {
            for (uint32_t x = a < shift ? shift : a; x < (e < end ? e : end); x++) d0[x] = stage[x];
        }
    }
}

template <bool ALIGNED>
__global__ void __launch_bounds__(256) k_u16_e_write(JtkU16EncWork w) {
    __shared__ alignas(16) uint8_t stage[JTK_U16_E_TILE * 3 + 32];
    const int64_t tile = blockIdx.x;
    const int64_t base = w.tile_off[tile];
    const uint32_t n = (uint32_t)(w.tile_off[tile + 1] - base);
    const int64_t lo = u16_clamp(w.unit_off[0], w.n_units), hi = u16_clamp(w.unit_off[w.n_docs], w.n_units);
    uint8_t* const mine = stage + (base & 15) + w.sub[tile * UL + threadIdx.x];
    e_tile_lane<ALIGNED>(w, lo, hi, tile * JTK_U16_E_TILE + threadIdx.x * JTK_U16_E_PER_LANE, mine);
    __syncthreads();
    u16_flush(stage, w.out, base, n);
}

__global__ void __launch_bounds__(256) k_u16_e_doc_off(JtkU16EncWork w) {
    const int64_t d = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (d > w.n_docs) return;
    const int64_t lo = w.unit_off[0], g = w.unit_off[d];                  // (checked by the count pass: lo <= g <= n_units)
    int64_t v;
    if ((g & (JTK_U16_E_TILE - 1)) == 0) {
        v = w.tile_off[g / JTK_U16_E_TILE];
    } else {
        v = w.tile_off[g / JTK_U16_E_TILE] + w.sub[g / JTK_U16_E_PER_LANE];
        const int64_t g0 = g & ~(int64_t)(JTK_U16_E_PER_LANE - 1);
        if (g0 < g) {                                                     // the lane's units before g: g itself is an edge
            const JtkU16Quad q = e_load<false>(w.units, w.n_units, g0);
            v += jtk_u16_e_lane(q, g0 > 0 ? (uint32_t)w.units[g0 - 1] : 0u, 0u, g0, lo, g, EEdge{w.unit_off, w.n_docs}, (uint8_t*)nullptr);
        }
    }
    w.doc_off[d] = v;
}

// ---- D ------------------------------------------------------------------------------------------------------------------
struct DEdges {                 // the edge mask of the lane at g0 (jtk_u16_d_avail): the offsets within g0 - 2 .. g0 + 18
    const int64_t* off;
    int64_t n_seqs, g0;
    __device__ uint32_t operator()() const {
        uint32_t m = 0;
        for (int64_t k = jtk_first_gt(off, 0, n_seqs + 1, g0 - 3); k <= n_seqs && off[k] <= g0 + 18; k++) m |= 1u << (int)(off[k] - (g0 - 2));
        return m;
    }
};

__device__ __forceinline__ JtkU16Quad d_load(const uint8_t* text, int64_t n_bytes, int64_t g0) {
    JtkU16Quad g{};
    if (g0 < n_bytes) g = *reinterpret_cast<const JtkU16Quad*>(text + g0);
    return g;
}

// a lane of a tile in either pass.  Called by all 64 lanes of every wave, outside any condition (it shuffles).
__device__ __forceinline__ uint32_t d_tile_lane(const JtkU16DecWork& w, int64_t g0, uint16_t* out) {
    const int lane = threadIdx.x & 63;
    const JtkU16Quad g = d_load(w.text, w.n_bytes, g0);
    uint32_t prev = (uint32_t)__shfl_up((int)g.w[3], 1);
    uint32_t next = (uint32_t)__shfl_down((int)g.w[0], 1);
    if (lane == 0) prev = (g0 >= 4 && g0 - 4 < w.n_bytes) ? *reinterpret_cast<const uint32_t*>(w.text + g0 - 4) : 0u;
    if (lane == 63) next = (g0 + 16 < w.n_bytes) ? *reinterpret_cast<const uint32_t*>(w.text + g0 + 16) : 0u;
    return jtk_u16_d_lane(g, prev, next, g0, w.n_bytes, DEdges{w.byte_off, w.n_seqs, g0}, out);
}

__global__ void __launch_bounds__(256) k_u16_d_count(JtkU16DecWork w) {
    const int64_t tile = blockIdx.x;
    const uint32_t cnt = d_tile_lane(w, tile * JTK_U16_D_TILE + threadIdx.x * JTK_U16_D_PER_LANE, nullptr);
    uint32_t total;
    const uint32_t pre = jtk_block_excl_prefix<UL>(cnt, &total);
    if (tile >= w.n_tiles) return;
    w.sub[tile * UL + threadIdx.x] = (uint16_t)pre;
    if (threadIdx.x == 0) w.tile_cnt[tile] = total;
}

__global__ void __launch_bounds__(256) k_u16_d_write(JtkU16DecWork w) {
    __shared__ alignas(16) uint8_t stage[JTK_U16_D_TILE * 2 + 32];
    const int64_t tile = blockIdx.x;
    const int64_t base = w.tile_off[tile] * 2;                            // in bytes of the output
    const uint32_t n = (uint32_t)(w.tile_off[tile + 1] * 2 - base);
    uint16_t* const mine = reinterpret_cast<uint16_t*>(stage + (base & 15)) + w.sub[tile * UL + threadIdx.x];
    d_tile_lane(w, tile * JTK_U16_D_TILE + threadIdx.x * JTK_U16_D_PER_LANE, mine);
    __syncthreads();
    u16_flush(stage, reinterpret_cast<uint8_t*>(w.out), base, n);
}

__global__ void __launch_bounds__(256) k_u16_d_unit_off(JtkU16DecWork w) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q > w.n_seqs) return;
    const int64_t g = u16_clamp(w.byte_off[q], w.n_bytes);
    int64_t v;
    if ((g & (JTK_U16_D_TILE - 1)) == 0) {
        v = w.tile_off[g / JTK_U16_D_TILE];
    } else {
        v = w.tile_off[g / JTK_U16_D_TILE] + w.sub[g / JTK_U16_D_PER_LANE];
        const int64_t g0 = g & ~(int64_t)(JTK_U16_D_PER_LANE - 1);
        if (g0 < g) {                                                     // the lane's bytes before g: g itself is an edge
            const uint32_t prev = g0 >= 4 ? *reinterpret_cast<const uint32_t*>(w.text + g0 - 4) : 0u;
            v += jtk_u16_d_lane(d_load(w.text, w.n_bytes, g0), prev, 0u, g0, g, DEdges{w.byte_off, w.n_seqs, g0}, (uint16_t*)nullptr);
        }
    }
    w.unit_off[q] = v;
}

}  // namespace

void jtk_launch_u16_enc_count(const JtkU16EncWork& w, bool aligned, hipStream_t s) {
    const dim3 grid((unsigned)(w.n_tiles > 0 ? w.n_tiles : 1));
    if (aligned) hipLaunchKernelGGL(k_u16_e_count<true>, grid, dim3(UL), 0, s, w);
    else hipLaunchKernelGGL(k_u16_e_count<false>, grid, dim3(UL), 0, s, w);
    jtk_launch_scan_u32(w.tile_cnt, w.n_tiles, w.tile_off, &w.hdr[0], s);
}

void jtk_launch_u16_enc_write(const JtkU16EncWork& w, bool aligned, hipStream_t s) {
    if (w.n_tiles > 0) {
        if (aligned) hipLaunchKernelGGL(k_u16_e_write<true>, dim3((unsigned)w.n_tiles), dim3(UL), 0, s, w);
        else hipLaunchKernelGGL(k_u16_e_write<false>, dim3((unsigned)w.n_tiles), dim3(UL), 0, s, w);
    }
    hipLaunchKernelGGL(k_u16_e_doc_off, dim3(jtk_blocks_for(w.n_docs + 1, 256)), dim3(256), 0, s, w);
}

void jtk_launch_u16_dec_count(const JtkU16DecWork& w, hipStream_t s) {
    if (w.n_tiles > 0) hipLaunchKernelGGL(k_u16_d_count, dim3((unsigned)w.n_tiles), dim3(UL), 0, s, w);
    jtk_launch_scan_u32(w.tile_cnt, w.n_tiles, w.tile_off, &w.hdr[0], s);
}

void jtk_launch_u16_dec_write(const JtkU16DecWork& w, hipStream_t s) {
    if (w.n_tiles > 0) hipLaunchKernelGGL(k_u16_d_write, dim3((unsigned)w.n_tiles), dim3(UL), 0, s, w);
    hipLaunchKernelGGL(k_u16_d_unit_off, dim3(jtk_blocks_for(w.n_seqs + 1, 256)), dim3(256), 0, s, w);
}
