// jtk_stop.hip -- stop strings over the last decode of a batch (jtk_batch_decode_find_stops): per sequence the first match of
// up to JTK_ST_MAX_STRINGS strings, the held-back tail when there is none, and the cell that holds the match.  The rule is
// jtk_stop_rules.h.  A post-pass: it reads every byte of the decode's output once, in order, and changes nothing of it.
//
//   stop_find    a workgroup per JTK_STOP_TILE bytes, one aligned 16-byte word per lane.  The tile and a halo of 64 bytes (a
//                match may end maxlen - 1 bytes into the next tile) are staged in LDS with the strings and the 256-bit map of
//                their first bytes.  A lane compares only at positions whose byte is in the map, finds its sequence when it
//                has such a position and steps it along by search, never by a walk: a row of 1 MB costs what its bytes cost
//                in short rows.  Hits go into one 64-bit key per sequence (p * JTK_ST_MAX_STRINGS + i) by atomicMin, a lane's
//                first per sequence only, and only when a plain read of the key is not already below it (the key only falls,
//                so a stale read costs an atomic, never a result); proper-prefix tails go into a second key the same way.
//   stop_finish  one lane per sequence: the keys -> stop_pos, stop_which, hold; stop_col by a binary search in the row's
//                cell_byte.
#include "jtk_device_prims.h"
#include "jtk_kernels.h"
#include "jtk_stop_rules.h"

namespace {

constexpr int ST = JTK_STOP_LANES;
constexpr int HALO = JTK_ST_MAX_BYTES;   // bytes staged past the tile: maxlen - 1 rounded up to whole 16-byte words
static_assert(ST * JTK_STOP_LANE == JTK_STOP_TILE && HALO % 16 == 0 && HALO >= JTK_ST_MAX_BYTES - 1, "tile geometry");
static_assert(sizeof(((JtkStopSet*)nullptr)->bytes) == ST * 4, "one word of the strings per lane");

__global__ void __launch_bounds__(ST) k_stop_find(JtkStopWork w) {
    __shared__ __attribute__((aligned(16))) uint8_t s_text[JTK_STOP_TILE + HALO];
    __shared__ __attribute__((aligned(16))) uint32_t s_str[ST];
    __shared__ uint32_t s_first[8];
    __shared__ uint8_t s_len[JTK_ST_MAX_STRINGS];
    const int tid = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * JTK_STOP_TILE;
    const int64_t p0 = base + (int64_t)tid * JTK_STOP_LANE;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (p0 < w.n_bytes) v = *reinterpret_cast<const uint4*>(w.out + p0);              // (readable up to the next multiple of 16)
    *reinterpret_cast<uint4*>(s_text + tid * JTK_STOP_LANE) = v;
    if (tid < HALO / 16) {
        const int64_t h = base + JTK_STOP_TILE + (int64_t)tid * 16;
        uint4 hv = make_uint4(0u, 0u, 0u, 0u);
        if (h < w.n_bytes) hv = *reinterpret_cast<const uint4*>(w.out + h);
        *reinterpret_cast<uint4*>(s_text + JTK_STOP_TILE + tid * 16) = hv;
    }
    s_str[tid] = w.set.bytes[tid];
    if (tid < 8) s_first[tid] = w.set.first[tid];
    if (tid < JTK_ST_MAX_STRINGS) s_len[tid] = w.set.len[tid];
    __syncthreads();
    if (p0 >= w.n_bytes) return;
    const uint32_t d4[4] = {v.x, v.y, v.z, v.w};
    const uint32_t cand = jtk_stop_cand16(s_first, d4, w.n_bytes - p0);
    if (cand == 0) return;                 // (most lanes of ordinary text hold no byte that starts a stop string)
    // a compare reads [p, E) with p inside the tile and at most JTK_ST_MAX_BYTES bytes: inside the staged tile + halo
    auto at = [&](int64_t x) -> uint8_t { return s_text[x - base]; };
    auto emit = [&](int64_t q, bool tail, uint64_t key) {
        unsigned long long* k = w.keys + (tail ? w.n_seqs + q : q);
        if (*k > key) atomicMin(k, (unsigned long long)key);
    };
    jtk_stop_lane((const uint8_t*)s_str, s_len, w.set.n, w.set.maxlen, cand, p0, w.byte_off, w.n_seqs, w.from, at, emit);
}

__global__ void __launch_bounds__(256) k_stop_finish(JtkStopWork w) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= w.n_seqs) return;
    const JtkStopResult r = jtk_stop_result(w.keys[q], w.keys[w.n_seqs + q], w.byte_off[q + 1]);
    w.stop_pos[q] = r.pos;
    w.stop_which[q] = r.which;
    w.hold[q] = r.hold;
    w.stop_col[q] = (w.cell_byte && r.which >= 0) ? jtk_stop_col(w.cell_byte, q, w.width, r.pos) : -1;
}

}  // namespace

void jtk_launch_stop_find(const JtkStopWork& w, hipStream_t s) {
    if (w.set.n > 0) hipLaunchKernelGGL(k_stop_find, dim3((unsigned)w.n_tiles), dim3(ST), 0, s, w);
    hipLaunchKernelGGL(k_stop_finish, dim3(jtk_blocks_for(w.n_seqs, 256)), dim3(256), 0, s, w);
}
