// validate_sim -- jtokkit_amd/csrc/jtk_validate_rules.h on the host, for tests/test_validate_rules_cpu.py: the rule run serially
// the way k_validate_utf8 (jtk_kernels.hip) runs it over one chunk of a job -- the chunk's text window starts at the tile at or
// below its first byte (`lead` bytes of the chunk before lie in front), the docmask holds one bit per document start of the
// chunk and one for its end as k_mark_docs sets them, one lane per byte of the window judges its byte, and a bad byte flags
// the document that find_doc names: the last one that starts at or before it, so never an empty one, and none for a byte in
// front of the chunk.  Reads stay inside [0, n_bytes) of the text.  Includes only the rule header.  Built with g++ by the
// test's fixture.
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../jtokkit_amd/csrc/jtk_validate_rules.h"

extern "C" {

// Documents [d0, d1) of the batch (text, doc_off [n_docs + 1]) as one chunk; tile: the alignment of the window's origin.
// status [n_docs] of the whole batch: JTK_ERR_BAD_UTF8 (-6) is written (as a minimum) for the chunk's malformed documents,
// nothing else is touched.  Returns 0, or -1 for offsets that k_mark_docs would refuse.
int sim_validate_chunk(const uint8_t* text, const int64_t* doc_off, int64_t d0, int64_t d1, int64_t tile, int32_t* status) {
    const int64_t b0 = doc_off[d0], b1 = doc_off[d1];
    const int64_t origin = b0 / tile * tile, lead = b0 - origin, n_bytes = b1 - origin, n_docs = d1 - d0;
    const uint8_t* win = text + origin;
    const int64_t* off = doc_off + d0;
    std::vector<uint64_t> docmask((size_t)(n_bytes / 64 + 1), 0);
    for (int64_t d = 0; d <= n_docs; d++) {
        const int64_t q = off[d] - origin;
        if (q < lead || q > n_bytes || (d > 0 && off[d - 1] - origin > q)) return -1;
        docmask[(size_t)(q >> 6)] |= 1ull << (q & 63);
    }
    auto ds = [&](int64_t q) { return q >= n_bytes || ((docmask[(size_t)(q >> 6)] >> (q & 63)) & 1ull) != 0; };
    auto at = [&](int64_t q) -> uint32_t { return (q >= 0 && q < n_bytes) ? win[q] : 0u; };
    for (int64_t p = 0; p < n_bytes; p++) {
        if (!jtk_utf8_byte_bad(p, at, ds)) continue;
        // the one before the first d with off[d] > p (-1: p is before all)
        int64_t lo = 0, hi = n_docs;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (off[mid] > p + origin) hi = mid; else lo = mid + 1;
        }
        const int64_t d = lo - 1;
        if (d >= 0 && status[d0 + d] > -6) status[d0 + d] = -6;
    }
    return 0;
}

}  // extern "C"
