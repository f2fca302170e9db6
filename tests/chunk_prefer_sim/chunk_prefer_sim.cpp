// chunk_prefer_sim.cpp -- TEST INFRASTRUCTURE.  Runs the boundary-preferring chunking rule the device kernels use
// (jtokkit_amd/csrc/jtk_chunk_prefer_rules.h) on the CPU, so that the CPU test tier can check it against a restatement and the
// oracle.  Nothing in the product loads this library.
#include <cstddef>
#include <cstdint>

#include "../../jtokkit_amd/csrc/jtk_chunk_prefer_rules.h"

extern "C" {

// One document: D[0, n_bytes) is its decoded stream and pos[i], i < n, the start of token i in it.  level[i] = the level of
// the cut before token i (6 for i = 0).
void sim_cut_levels(const uint8_t* D, const int64_t* pos, int64_t n, uint32_t prefer, uint8_t* level) {
    for (int64_t i = 0; i < n; i++) {
        if (i == 0) { level[i] = JTK_LEVEL_DOC_END; continue; }
        const int64_t p = pos[i];
        auto x = [&](int64_t k) { return p - k >= 0 ? (int)D[p - k] : -1; };
        level[i] = (uint8_t)jtk_cut_level(prefer, D[p], x(1), x(2), x(3));
    }
}

// The walk over a level plane of n tokens.  Writes chunk k as (s[k], e[k], split[k], end_level[k]) for k < cap and returns the
// chunk count.
int64_t sim_chunk_prefer(const uint8_t* level, int64_t n, int64_t N, int64_t overlap, int64_t min_tokens, int64_t* s, int64_t* e,
                         uint8_t* split, uint8_t* end_level, int64_t cap) {
    return jtk_chunk_prefer_walk(n, N, overlap, min_tokens, [&](int64_t i) { return (int)level[i]; },
                                 [&](int64_t k, int64_t cs, int64_t ce, bool sp, int el) {
                                     if (k < cap) { s[k] = cs; e[k] = ce; split[k] = sp ? 1 : 0; end_level[k] = (uint8_t)el; }
                                 });
}

}  // extern "C"
