// phrase_sim -- the CPU shim of phrase sets: the host build of jtokkit_amd/csrc/jtk_phrase_rules.h as jtk_abi.cpp calls it, and the
// walk of jtk_phrase.hip over its tables, one start position after the other: bitmap test, probe, boundary.  No GPU, no HIP.
#include <stdint.h>

#define JTK_PHRASE_HOST_BUILD
#include "../../jtokkit_amd/csrc/jtk_device_prims.h"
#include "../../jtokkit_amd/csrc/jtk_phrase_rules.h"
#include "../../jtokkit_amd/csrc/jtk_unicode_tables.h"

namespace {
struct Text {                      // the (folded) byte at a batch position, 0 behind the text: what the kernel stages
    const uint8_t* x;
    int64_t n;
    bool fold;
    uint32_t operator[](int64_t i) const { return i < 0 || i >= n ? 0u : fold ? jtk_ph_fold_byte(x[i]) : x[i]; }
};
}  // namespace

extern "C" {
// NULL and *what = the refusal, or a set
void* sim_ph_build(const uint8_t* bytes, const uint32_t* off, const uint8_t* group, int64_t n, uint32_t flags, const char** what) {
    JtkPhHostSet* s = new JtkPhHostSet();
    *what = jtk_ph_build(bytes, off, group, n, flags, s);
    if (!*what) return s;
    delete s;
    return nullptr;
}
void sim_ph_free(void* s) { delete (JtkPhHostSet*)s; }
// first_hit / first_which preset to -1 and the rest to 0 by the caller
void sim_ph_hits(const void* set, const uint8_t* text, int64_t n_bytes, const int64_t* doc_off, const int32_t* status, int64_t n_docs,
                 uint32_t* group_mask, int32_t* n_hits, int64_t* first_hit, int32_t* first_which) {
    const JtkPhHostSet& s = *(const JtkPhHostSet*)set;
    const JtkUcTables uc{jtk_uc_stage1_init, jtk_uc_stage2_init};
    const Text x{text, n_bytes, (s.flags & JTK_PHRASE_FOLD_ASCII) != 0};
    const auto find = [&](uint32_t state, uint32_t byte) { return jtk_ph_find(s.edges.data(), s.n_slots, state, byte); };
    for (int64_t p = 0; p < n_bytes && s.n_distinct; p++) {
        if (!jtk_ph_candidate(s.first2.data(), s.first1.data(), x[p], x[p + 1])) continue;
        const int64_t d = jtk_first_gt(doc_off, 0, n_docs + 1, p) - 1;
        if (d < 0 || d >= n_docs || status[d] < 0) continue;
        const int64_t a = doc_off[d], e = doc_off[d + 1];
        jtk_ph_walk(x, e, p, find, [&](int len, uint32_t v) {
            if ((s.flags & JTK_PHRASE_WORD_BOUNDS) && !jtk_ph_bounded(x, uc, a, e, p, len)) return;
            const JtkPhInfo t = s.info[v & JTK_PH_V_STATE];
            group_mask[d] |= t.group_mask;
            n_hits[d]++;
            if (first_hit[d] >= 0 && jtk_ph_first_key(p - a, t.index) >= jtk_ph_first_key(first_hit[d], (uint32_t)first_which[d])) return;
            first_hit[d] = p - a;
            first_which[d] = (int32_t)t.index;
        });
    }
}
}
