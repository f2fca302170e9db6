// utf16_sim -- jtokkit_amd/csrc/jtk_utf16_rules.h on the host, for tests/test_utf16_rules_cpu.py: both directions run serially the
// way jtk_utf16.hip partitions the work -- tile by tile, lane by lane, one 16-byte granule per lane, the neighbour units / bytes
// from the lane before and after (a guarded load at a wave's first and last lane), count -> prefix inside the tile (sub) and tile
// totals -> scan -> write -> offsets.  The kernels' LDS stage is a copy and is not modelled: a lane writes at tile_off + sub.
// Reads stay inside what the ABI documents as readable: the 16-byte granule that holds the last unit / byte (E with `aligned`,
// D), or the n_units units alone (E without).  Includes only the rule header.  Built with g++ by the test's fixture.
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../jtokkit_amd/csrc/jtk_utf16_rules.h"

namespace {

struct Edge {                   // x is one of off[0 .. n]
    const int64_t* off;
    int64_t n;
    bool operator()(int64_t x) const { return std::binary_search(off, off + n + 1, x); }
};

struct Edges {                  // the edge mask of the lane at g0
    const int64_t* off;
    int64_t n, g0;
    uint32_t operator()() const {
        uint32_t m = 0;
        for (const int64_t* p = std::lower_bound(off, off + n + 1, g0 - 2); p < off + n + 1 && *p <= g0 + 18; p++) m |= 1u << (int)(*p - (g0 - 2));
        return m;
    }
};

int64_t clampi(int64_t v, int64_t n) { return v < 0 ? 0 : v > n ? n : v; }

JtkU16Quad e_load(const uint16_t* units, int64_t n_units, int64_t g0, bool aligned) {
    JtkU16Quad g{};
    if (g0 >= n_units) return g;
    if (aligned) { memcpy(&g, units + g0, 16); return g; }
    for (int k = 0; k < JTK_U16_E_PER_LANE; k++)
        if (g0 + k < n_units) g.w[k >> 1] |= (uint32_t)units[g0 + k] << (16 * (k & 1));
    return g;
}

JtkU16Quad d_load(const uint8_t* text, int64_t n_bytes, int64_t g0) {
    JtkU16Quad g{};
    if (g0 < n_bytes) memcpy(&g, text + g0, 16);
    return g;
}

uint32_t load32(const uint8_t* p) { uint32_t v; memcpy(&v, p, 4); return v; }

}  // namespace

extern "C" {

int sim_u16_tile(int dir) { return dir == 0 ? JTK_U16_E_TILE : JTK_U16_D_TILE; }

// E.  Returns the byte total, or -1 for bad offsets; out (capacity out_cap; NULL: sizes only) and doc_off [n_docs + 1] are
// written when the total fits.
int64_t sim_u16_encode(const uint16_t* units, const int64_t* unit_off, int64_t n_docs, int64_t n_units, int aligned, uint8_t* out,
                       int64_t out_cap, int64_t* doc_off) {
    for (int64_t d = 0; d <= n_docs; d++)
        if (unit_off[d] < 0 || unit_off[d] > n_units || (d < n_docs && unit_off[d + 1] < unit_off[d])) return -1;
    const int64_t lo = clampi(unit_off[0], n_units), hi = clampi(unit_off[n_docs], n_units);
    const int64_t n_tiles = (n_units + JTK_U16_E_TILE - 1) / JTK_U16_E_TILE;
    const Edge edge{unit_off, n_docs};
    std::vector<uint16_t> sub((size_t)n_tiles * JTK_U16_LANES);
    std::vector<int64_t> tile_off((size_t)n_tiles + 1, 0);
    for (int pass = 0; pass < 2; pass++) {
        if (pass == 1 && (!out || out_cap < tile_off[(size_t)n_tiles])) break;
        for (int64_t t = 0; t < n_tiles; t++) {
            uint32_t run = 0;
            JtkU16Quad before{};
            for (int l = 0; l < JTK_U16_LANES; l++) {
                const int64_t g0 = t * JTK_U16_E_TILE + (int64_t)l * JTK_U16_E_PER_LANE;
                const JtkU16Quad g = e_load(units, n_units, g0, aligned != 0);
                uint32_t prev, next;
                if (l % 64 == 0) prev = (g0 > 0 && g0 - 1 < n_units) ? units[g0 - 1] : 0u;
                else prev = before.w[3] >> 16;
                if (l % 64 == 63) next = (g0 + JTK_U16_E_PER_LANE < n_units) ? units[g0 + JTK_U16_E_PER_LANE] : 0u;
                else next = e_load(units, n_units, g0 + JTK_U16_E_PER_LANE, aligned != 0).w[0] & 0xFFFFu;
                before = g;
                if (pass == 0) {
                    sub[(size_t)(t * JTK_U16_LANES + l)] = (uint16_t)run;
                    run += jtk_u16_e_lane(g, prev, next, g0, lo, hi, edge, (uint8_t*)nullptr);
                } else {
                    jtk_u16_e_lane(g, prev, next, g0, lo, hi, edge, out + tile_off[(size_t)t] + sub[(size_t)(t * JTK_U16_LANES + l)]);
                }
            }
            if (pass == 0) tile_off[(size_t)t + 1] = tile_off[(size_t)t] + run;
        }
    }
    for (int64_t d = 0; d <= n_docs && doc_off; d++) {
        const int64_t g = unit_off[d];
        int64_t v;
        if ((g & (JTK_U16_E_TILE - 1)) == 0) {
            v = tile_off[(size_t)(g / JTK_U16_E_TILE)];
        } else {
            v = tile_off[(size_t)(g / JTK_U16_E_TILE)] + sub[(size_t)(g / JTK_U16_E_PER_LANE)];
            const int64_t g0 = g & ~(int64_t)(JTK_U16_E_PER_LANE - 1);
            if (g0 < g)
                v += jtk_u16_e_lane(e_load(units, n_units, g0, false), g0 > 0 ? (uint32_t)units[g0 - 1] : 0u, 0u, g0, unit_off[0], g, edge, (uint8_t*)nullptr);
        }
        doc_off[d] = v;
    }
    return tile_off[(size_t)n_tiles];
}

// D.  text is readable up to the next multiple of 16 past n_bytes; byte_off starts at 0, never decreases and ends at n_bytes.
// Returns the unit total; out (capacity out_cap units; NULL: sizes only) and unit_off [n_seqs + 1].
int64_t sim_u16_decode(const uint8_t* text, const int64_t* byte_off, int64_t n_seqs, int64_t n_bytes, uint16_t* out, int64_t out_cap,
                       int64_t* unit_off) {
    const int64_t n_tiles = (n_bytes + JTK_U16_D_TILE - 1) / JTK_U16_D_TILE;
    std::vector<uint16_t> sub((size_t)n_tiles * JTK_U16_LANES);
    std::vector<int64_t> tile_off((size_t)n_tiles + 1, 0);
    for (int pass = 0; pass < 2; pass++) {
        if (pass == 1 && (!out || out_cap < tile_off[(size_t)n_tiles])) break;
        for (int64_t t = 0; t < n_tiles; t++) {
            uint32_t run = 0;
            JtkU16Quad before{};
            for (int l = 0; l < JTK_U16_LANES; l++) {
                const int64_t g0 = t * JTK_U16_D_TILE + (int64_t)l * JTK_U16_D_PER_LANE;
                const JtkU16Quad g = d_load(text, n_bytes, g0);
                uint32_t prev, next;
                if (l % 64 == 0) prev = (g0 >= 4 && g0 - 4 < n_bytes) ? load32(text + g0 - 4) : 0u;
                else prev = before.w[3];
                if (l % 64 == 63) next = (g0 + 16 < n_bytes) ? load32(text + g0 + 16) : 0u;
                else next = d_load(text, n_bytes, g0 + 16).w[0];
                before = g;
                const Edges edges{byte_off, n_seqs, g0};
                if (pass == 0) {
                    sub[(size_t)(t * JTK_U16_LANES + l)] = (uint16_t)run;
                    run += jtk_u16_d_lane(g, prev, next, g0, n_bytes, edges, (uint16_t*)nullptr);
                } else {
                    jtk_u16_d_lane(g, prev, next, g0, n_bytes, edges, out + tile_off[(size_t)t] + sub[(size_t)(t * JTK_U16_LANES + l)]);
                }
            }
            if (pass == 0) tile_off[(size_t)t + 1] = tile_off[(size_t)t] + run;
        }
    }
    for (int64_t q = 0; q <= n_seqs && unit_off; q++) {
        const int64_t g = clampi(byte_off[q], n_bytes);
        int64_t v;
        if ((g & (JTK_U16_D_TILE - 1)) == 0) {
            v = tile_off[(size_t)(g / JTK_U16_D_TILE)];
        } else {
            v = tile_off[(size_t)(g / JTK_U16_D_TILE)] + sub[(size_t)(g / JTK_U16_D_PER_LANE)];
            const int64_t g0 = g & ~(int64_t)(JTK_U16_D_PER_LANE - 1);
            if (g0 < g)
                v += jtk_u16_d_lane(d_load(text, n_bytes, g0), g0 >= 4 ? load32(text + g0 - 4) : 0u, 0u, g0, g, Edges{byte_off, n_seqs, g0}, (uint16_t*)nullptr);
        }
        unit_off[q] = v;
    }
    return tile_off[(size_t)n_tiles];
}

// the per-position functions alone, for the exhaustive checks: the bytes of units[i] of ONE document / the units of text[i] of ONE sequence
int sim_u16_e_unit(const uint16_t* units, int64_t n, int64_t i, uint8_t* out4) {
    const uint32_t u = units[i], prev = i > 0 ? units[i - 1] : 0u, next = i + 1 < n ? units[i + 1] : 0u;
    bool edge = false;
    if (jtk_u16_e_needs_edge(u, prev, next)) edge = jtk_u16_is_high(u) ? i + 1 >= n : i <= 0;
    const uint32_t len = jtk_u16_e_len(u, prev, next, edge);
    jtk_u16_e_put(u, next, len, out4);
    return (int)len;
}
int sim_u16_d_byte(const uint8_t* text, int64_t n, int64_t i, uint16_t* out2) {
    uint64_t win = 0;
    for (int k = -3; k <= 3; k++)
        if (i + k >= 0 && i + k < n) win |= (uint64_t)text[i + k] << (8 * (k + 3));
    return jtk_u16_d_emit(win, (int)std::min<int64_t>(3, i), (int)std::min<int64_t>(3, n - 1 - i), out2);
}

}  // extern "C"
