// seen_sim -- the CPU shim of the seen set (jtk_seen_set_*, jtk_batch_seen_mark): the functions of the rule header
// jtokkit_amd/csrc/jtk_seen_rules.h as they are, and entries merged into three planes the way k_sn_add does it, one entry after
// the other: claim with wrap-around, min on first, sum on count.  No GPU, no HIP.
#include <stdint.h>

#include "../../jtokkit_amd/csrc/jtk_seen_rules.h"

namespace {
struct HostCas {
    uint64_t operator()(uint64_t* p, uint64_t k) const {
        const uint64_t old = *p;
        if (old == 0) *p = k;
        return old;
    }
};
}  // namespace

extern "C" {
int sim_sn_docs_ok(uint64_t base, int64_t n_docs) { return jtk_sn_docs_ok(base, n_docs) ? 1 : 0; }
uint64_t sim_sn_key(uint64_t seed, int32_t unit) { return jtk_sn_key(seed, unit); }
uint64_t sim_sn_finish(uint64_t h, uint64_t key) { return jtk_ln_finish(h, key); }
uint32_t sim_sn_threshold(int32_t unit) { return jtk_sn_threshold(unit); }
int sim_sn_breaks(uint32_t s, uint32_t thr) { return jtk_ln_breaks(s, thr) ? 1 : 0; }
uint64_t sim_sn_pos(uint64_t base, int64_t d, int64_t u) { return jtk_sn_pos(base, d, u); }
int64_t sim_sn_max_doc_units() { return JTK_SN_MAX_DOC_UNITS; }
int64_t sim_sn_capacity(int64_t c, int64_t m) { return jtk_sn_capacity(c, m); }
// n entries into planes[3 * capacity] (jtk_sn_table_at, preset by the caller); slots[i] = where entry i went; returns the new keys
int64_t sim_sn_add_entries(uint64_t* planes, int64_t capacity, const uint64_t* keys, const uint64_t* first, const uint64_t* count, int64_t n,
                           int64_t* slots) {
    const JtkSnTable t = jtk_sn_table_at(planes, capacity);
    int64_t fresh = 0;
    for (int64_t i = 0; i < n; i++) {
        bool f;
        const uint64_t slot = jtk_sn_claim(t.key, t.mask, keys[i], HostCas(), &f);
        jtk_sn_merge(t.first + slot, t.count + slot, first[i], count[i]);
        slots[i] = (int64_t)slot;
        fresh += f ? 1 : 0;
    }
    return fresh;
}
}
