// special_sim.cpp -- TEST INFRASTRUCTURE.  Runs the match selection of the allow-special encode the device kernels use
// (jtokkit_amd/csrc/jtk_special_rules.h) on the CPU -- candidates, the certain test, the chain walk --, so that the CPU test
// tier can check it against a restatement.  Nothing in the product loads this library.
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../jtokkit_amd/csrc/jtk_special_rules.h"

extern "C" {

// One document of n bytes; literal i = blob[off[i], off[i + 1]), allowed[i].  Writes kept match k as (s[k], e[k], lit[k])
// for k < cap and returns the match count; *dis = some literal outside the allowed set occurs in the document.
int64_t sim_special(const uint8_t* text, int64_t n, int n_lits, const uint32_t* off, const uint8_t* blob, const uint8_t* allowed,
                    int64_t* s, int64_t* e, int32_t* lit, int64_t cap, int32_t* dis) {
    auto at = [&](int64_t q) -> uint32_t { return text[q]; };
    int64_t maxlen = 0;
    for (int i = 0; i < n_lits; i++) if (allowed[i] && (int64_t)(off[i + 1] - off[i]) > maxlen) maxlen = off[i + 1] - off[i];
    std::vector<int64_t> cp, ce;
    std::vector<int32_t> cl;
    *dis = 0;
    for (int64_t p = 0; p < n; p++) {
        int len, idx;
        if (jtk_special_scan_at(p, n, at, n_lits, off, blob, allowed, &len, &idx)) *dis = 1;
        if (len > 0) { cp.push_back(p); ce.push_back(p + len); cl.push_back(idx); }
    }
    const int64_t nc = (int64_t)cp.size();
    auto fs = [&](int64_t k) { return cp[(size_t)k]; };
    auto fe = [&](int64_t k) { return ce[(size_t)k]; };
    std::vector<uint8_t> keep((size_t)nc, 0);
    for (int64_t i = 0; i < nc; i++) keep[(size_t)i] = jtk_special_certain(i, maxlen, fs, fe) ? 1 : 2;
    for (int64_t i = 0; i + 1 < nc; i++)
        if (keep[(size_t)i] == 1 && keep[(size_t)i + 1] != 1)
            jtk_special_walk(i, nc, fs, fe, [&](int64_t k) { return keep[(size_t)k] == 1; },
                             [&](int64_t k, bool kept) { keep[(size_t)k] = kept ? 3 : 0; });
    int64_t m = 0;
    for (int64_t i = 0; i < nc; i++) {
        if (keep[(size_t)i] != 1 && keep[(size_t)i] != 3) continue;
        if (m < cap) { s[m] = cp[(size_t)i]; e[m] = ce[(size_t)i]; lit[m] = cl[(size_t)i]; }
        m++;
    }
    return m;
}

}  // extern "C"
