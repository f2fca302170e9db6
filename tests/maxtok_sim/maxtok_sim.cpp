// maxtok_sim.cpp -- TEST INFRASTRUCTURE.  Runs the maxTokens early-exit rules the host and the device share
// (jtokkit_amd/csrc/jtk_maxtok_rules.h) on the CPU, so that the CPU test tier can check them against the oracle.
// Nothing in the product loads this library.
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../jtokkit_amd/csrc/jtk_maxtok_rules.h"

extern "C" {

// The decision for one document of `len` bytes whose first p bytes were encoded: text = the document (only the prefix and
// the few bytes after the cut that the back-off counts are read), starts[p + 1] = 1 where a piece of the prefix starts,
// tok_len[n] = byte lengths of the prefix's tokens.  Returns the tokens kept (and *truncated), or -1: undecided.
int64_t sim_maxtok_decide(const uint8_t* text, int64_t len, int64_t p, const uint8_t* starts, const int32_t* tok_len, int64_t n,
                          int64_t max_tokens, int* truncated) {
    std::vector<uint64_t> mask((size_t)(p + 64) / 64 + 1, 0);
    for (int64_t i = 0; i <= p; i++)
        if (starts[i]) mask[(size_t)(i >> 6)] |= 1ull << (i & 63);
    int64_t k = -1, nb = 0;
    if (p == len) {
        k = n < max_tokens ? n : max_tokens;
        for (int64_t j = 0; j < k; j++) nb += tok_len[j];
    } else {
        const int64_t q = jtk_maxtok_last_safe_start(mask.data(), 0, text, p);
        if (q > 0 && n >= max_tokens) {
            int64_t cum = 0;
            for (int64_t j = 0; j < max_tokens && cum <= q; j++) cum += tok_len[j];
            if (jtk_maxtok_decided(n, max_tokens, cum, q)) { k = max_tokens; nb = cum; }
        }
    }
    if (k < 0) return -1;
    const JtkBackoff r = jtk_maxtok_backoff(text, len, k, nb, [&](int64_t j) { return (int64_t)tok_len[j]; });
    *truncated = r.ok && jtk_more_units_than(text, r.from, len, r.units);
    return r.keep;
}

// The last safe piece start of a prefix of p bytes whose bits begin at `base` of `mask` (the host passes a document's offset in
// its group's gather buffer, the device its offset from the chunk's origin): t = the prefix.
int64_t sim_maxtok_last_safe_start(const uint64_t* mask, int64_t base, const uint8_t* t, int64_t p) {
    return jtk_maxtok_last_safe_start(mask, base, t, p);
}

// The prefix sizes of the rounds: out[r] for r < n_rounds (cb: the chunk size past which a document goes whole).
void sim_maxtok_prefixes(int64_t len, int64_t max_tokens, int64_t cb, int n_rounds, int64_t* out) {
    int64_t P = jtk_maxtok_first_prefix(max_tokens);
    for (int r = 0; r < n_rounds; r++, P = jtk_maxtok_next_prefix(P)) out[r] = jtk_maxtok_prefix_bytes(len, P, cb);
}

}  // extern "C"
