// stop_sim.cpp -- TEST INFRASTRUCTURE.  Runs the stop-string rule that the device kernels use
// (jtokkit_amd/csrc/jtk_stop_rules.h) serially on the CPU, partitioned the way jtk_stop.hip partitions it, so that the CPU test
// tier can check it against a restatement (tests/stop_ref.py): tile by tile, the tile and its halo copied into a staging buffer
// of exactly the kernel's LDS size, lane by lane over the candidate positions, the two keys per sequence as running minima,
// then the finish per sequence.  Nothing in the product loads this library.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../jtokkit_amd/csrc/jtk_stop_rules.h"

extern "C" {

int sim_stop_tile() { return JTK_STOP_TILE; }
int sim_stop_lane() { return JTK_STOP_LANE; }
int sim_stop_max_strings() { return JTK_ST_MAX_STRINGS; }
int sim_stop_max_bytes() { return JTK_ST_MAX_BYTES; }

// out: 16-byte aligned, readable up to the next multiple of 16 past n_bytes.  byte_off[n_seqs + 1]; from[n_seqs] or NULL;
// cell_byte[n_seqs * width] or NULL.  Results [n_seqs] each.  -> 0, or -1 when the strings break the limits.
int sim_find_stops(const uint8_t* out, int64_t n_bytes, const int64_t* byte_off, int64_t n_seqs, const uint8_t* strings,
                   const uint32_t* str_off, int n_strings, const int64_t* from, const int64_t* cell_byte, int64_t width,
                   int64_t* stop_pos, int32_t* stop_which, int32_t* hold, int64_t* stop_col) {
    JtkStopSet set;
    if (!jtk_stop_set_init(&set, strings, str_off, n_strings)) return -1;
    std::vector<uint64_t> keys(2 * (size_t)n_seqs, JTK_STOP_NONE);
    constexpr int HALO = JTK_ST_MAX_BYTES;
    std::vector<uint8_t> s_text(JTK_STOP_TILE + HALO);
    const int64_t n_tiles = (n_bytes + JTK_STOP_TILE - 1) / JTK_STOP_TILE;
    for (int64_t tile = 0; set.n > 0 && n_seqs > 0 && tile < n_tiles; tile++) {
        const int64_t base = tile * JTK_STOP_TILE;
        for (int64_t g = 0; g < JTK_STOP_TILE + HALO; g += 16) {                   // whole words, zero past the end of `out`
            if (base + g < n_bytes) memcpy(&s_text[g], out + base + g, 16);
            else memset(&s_text[g], 0, 16);
        }
        for (int lane = 0; lane < JTK_STOP_LANES; lane++) {
            const int64_t p0 = base + (int64_t)lane * JTK_STOP_LANE;
            if (p0 >= n_bytes) break;
            uint32_t w[4];
            memcpy(w, &s_text[lane * JTK_STOP_LANE], 16);
            const uint32_t cand = jtk_stop_cand16(set.first, w, n_bytes - p0);
            if (cand == 0) continue;
            auto at = [&](int64_t x) -> uint8_t { return s_text.at((size_t)(x - base)); };
            auto emit = [&](int64_t q, bool tail, uint64_t key) {
                uint64_t& k = keys.at((size_t)(tail ? n_seqs + q : q));
                if (key < k) k = key;
            };
            jtk_stop_lane((const uint8_t*)set.bytes, set.len, set.n, set.maxlen, cand, p0, byte_off, n_seqs, from, at, emit);
        }
    }
    for (int64_t q = 0; q < n_seqs; q++) {
        const JtkStopResult r = jtk_stop_result(keys[q], keys[n_seqs + q], byte_off[q + 1]);
        stop_pos[q] = r.pos;
        stop_which[q] = r.which;
        hold[q] = r.hold;
        stop_col[q] = (cell_byte && r.which >= 0) ? jtk_stop_col(cell_byte, q, width, r.pos) : -1;
    }
    return 0;
}

}
