// chunk_sim.cpp -- TEST INFRASTRUCTURE.  Runs the token-budget chunking rule the device kernels use
// (jtokkit_amd/csrc/jtk_chunk_rules.h) on the CPU, so that the CPU test tier can check it against a restatement and the
// oracle.  Nothing in the product loads this library.
#include <cstddef>
#include <cstdint>

#include "../../jtokkit_amd/csrc/jtk_chunk_rules.h"

extern "C" {

// One document of n tokens; first_byte[i] = the first byte of token i's byte string (0 for an empty one).  Writes chunk k as
// (s[k], e[k], split[k]) for k < cap and returns the chunk count.
int64_t sim_chunk(const uint8_t* first_byte, int64_t n, int64_t N, int64_t overlap, int64_t* s, int64_t* e, uint8_t* split,
                  int64_t cap) {
    auto bnd = [&](int64_t i) { return (first_byte[i] & 0xC0) != 0x80; };
    return jtk_chunk_walk(n, N, overlap, bnd, [&](int64_t k, int64_t cs, int64_t ce, bool sp) {
        if (k < cap) { s[k] = cs; e[k] = ce; split[k] = sp ? 1 : 0; }
    });
}

}  // extern "C"
