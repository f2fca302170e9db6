// compact_sim.cpp -- TEST INFRASTRUCTURE.  Runs the compact-ids rule the device kernel and the host widening routine use
// (jtokkit_amd/csrc/jtk_compact_rules.h) on the CPU, so that the CPU test tier can check it against a restatement
// (tests/compact_ref.py).  A stream is compacted range by range, as the chunks of a job hand their tokens over, with the
// header's serial pass; widening goes through the header's per-token function.  Nothing in the product loads this library.
#include <cstdint>

#include "../../jtokkit_amd/csrc/jtk_compact_rules.h"

extern "C" {

int sim_compact_hb(int64_t max_id) { return jtk_compact_hb(max_id); }
int sim_compact_valid_bits(int id_bits) { return jtk_compact_valid_bits(id_bits) ? 1 : 0; }
int64_t sim_compact_hi_words(int64_t n, int hb) { return jtk_compact_hi_words(n, hb); }
int64_t sim_compact_lo_bytes(int64_t n) { return jtk_compact_lo_bytes(n); }

// ids[n] in the ranges [cuts[k], cuts[k + 1]) for k < n_cuts - 1 (cuts[0] = 0, cuts[n_cuts - 1] = n), in that order
void sim_compact(const int32_t* ids, const int64_t* cuts, int64_t n_cuts, uint16_t* lo, uint32_t* hi, int hb) {
    for (int64_t k = 0; k + 1 < n_cuts; k++) jtk_compact_range_serial(ids, cuts[k], cuts[k + 1], lo, hi, hb);
}

void sim_widen(const uint16_t* lo, const uint32_t* hi, int hb, int64_t first, int64_t n, int32_t* out) {
    for (int64_t k = 0; k < n; k++) out[k] = jtk_compact_widen(lo, hi, hb, first + k);
}

}
