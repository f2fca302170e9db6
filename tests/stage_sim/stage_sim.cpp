// stage_sim.cpp -- TEST INFRASTRUCTURE.  Runs the rule by which k_pack_tokens places a tile's merge results in LDS
// (jtokkit_amd/csrc/jtk_stage_rules.h) on the CPU, so that the CPU test tier can check it.  Nothing in the product loads
// this library.
#include <cstdint>

#include "../../jtokkit_amd/csrc/jtk_stage_rules.h"

extern "C" {

// the constants, by index: 0 head slots, 1 assembly slots, 2 assembly words, 3 bins
int sim_stage_const(int k) {
    return k == 0 ? JTK_PACK_SLOTS : k == 1 ? JTK_PACK_OUT_SLOTS : k == 2 ? JTK_PACK_STAGE : JTK_NBINS_STAGE;
}
int sim_stage_cap(int bin) { return JTK_PACK_CAP(bin); }
int sim_stage_head(int bin) { return JTK_PACK_OFF(bin); }

// m tiles at once: total[t], nq[t][bins] -> off[t][bins], n[t][bins], word[t][bins]
void sim_stage_rules(int64_t m, const uint32_t* total, const uint32_t* nq, uint32_t* off, uint32_t* n, uint32_t* word) {
    for (int64_t t = 0; t < m; t++) {
        jtk_stage_rules(total[t], nq + t * JTK_NBINS_STAGE, off + t * JTK_NBINS_STAGE, n + t * JTK_NBINS_STAGE);
        for (int b = 0; b < JTK_NBINS_STAGE; b++)
            word[t * JTK_NBINS_STAGE + b] = jtk_stage_word(b, off[t * JTK_NBINS_STAGE + b], n[t * JTK_NBINS_STAGE + b]);
    }
}

}
