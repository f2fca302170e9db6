// charpos_sim -- jtokkit_amd/csrc/jtk_charpos_rules.h on the host, for tests/test_charpos_rules_cpu.py: the index built granule
// by granule as k_cp_build's lanes count it (jtk_cp_quad_units over 16 bytes, summed in the order of the kernel's loads), and
// the header's own rank, forward and inverse walks over it.  Built with g++ by the test's fixture.
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../jtokkit_amd/csrc/jtk_charpos_rules.h"

namespace {

struct Sim {
    uint8_t* text = nullptr;                 // 16-byte aligned copy, filled with 0xFF up to the next multiple of 16 (bytes that must count 0)
    std::vector<int64_t> doc_off, sup, dunit;
    std::vector<uint16_t> sub;
    JtkCharIndex ix{};
    int64_t n_docs = 0;
};

}  // namespace

extern "C" {

void* sim_cp_open(const uint8_t* text, int64_t n_bytes, const int64_t* doc_off, int64_t n_docs, int unit) {
    Sim* s = new Sim;
    const size_t padded = ((size_t)n_bytes + 15) / 16 * 16 + 16;
    s->text = (uint8_t*)aligned_alloc(16, padded);
    memset(s->text, 0xFF, padded);
    if (n_bytes) memcpy(s->text, text, (size_t)n_bytes);
    s->doc_off.assign(doc_off, doc_off + n_docs + 1);
    s->n_docs = n_docs;
    const int64_t n_sup = (n_bytes + JTK_CP_SUPER - 1) / JTK_CP_SUPER;
    s->sup.assign((size_t)n_sup + 1, 0);
    s->sub.assign((size_t)n_sup * JTK_CP_BLOCKS_PER_SUPER + 1, 0);
    int64_t total = 0;
    for (int64_t sb = 0; sb < n_sup; sb++) {
        s->sup[(size_t)sb] = total;
        uint32_t run = 0;
        for (int j = 0; j < 4; j++)                                       // the kernel's load j, lanes 0 .. 63
            for (int lane = 0; lane < 64; lane++) {
                const int64_t off = sb * JTK_CP_SUPER + j * 1024 + lane * 16;
                if ((lane & 3) == 0) s->sub[(size_t)(sb * JTK_CP_BLOCKS_PER_SUPER + j * 16 + (lane >> 2))] = (uint16_t)run;
                if (off < n_bytes) run += jtk_cp_quad_units(jtk_cp_load_quad(s->text, off), n_bytes - off, unit);
            }
        total += run;
    }
    s->sup[(size_t)n_sup] = total;
    s->ix.text = s->text; s->ix.n_bytes = n_bytes; s->ix.sup = s->sup.data(); s->ix.sub = s->sub.data(); s->ix.n_sup = n_sup; s->ix.unit = unit;
    s->dunit.resize((size_t)n_docs + 1);
    for (int64_t d = 0; d <= n_docs; d++) s->dunit[(size_t)d] = jtk_cp_rank(s->ix, jtk_cp_clamp(doc_off[d], n_bytes));
    return s;
}

void sim_cp_close(void* h) {
    Sim* s = (Sim*)h;
    free(s->text);
    delete s;
}

void sim_cp_doc_units(void* h, int64_t* out) {
    Sim* s = (Sim*)h;
    for (int64_t d = 0; d < s->n_docs; d++) out[d] = s->dunit[(size_t)d + 1] - s->dunit[(size_t)d];
}

void sim_cp_char_positions(void* h, int round, const int64_t* doc_or_null, const int64_t* byte_pos, int64_t n, int64_t* out) {
    Sim* s = (Sim*)h;
    for (int64_t i = 0; i < n; i++) {
        const int64_t d = doc_or_null ? doc_or_null[i] : jtk_cp_doc_of(s->doc_off.data(), s->n_docs, s->ix.n_bytes, byte_pos[i]);
        out[i] = jtk_cp_char_index(s->ix, s->doc_off.data(), s->dunit.data(), s->n_docs, d, byte_pos[i], round);
    }
}

void sim_cp_byte_positions(void* h, const int64_t* doc, const int64_t* char_pos, int64_t n, int64_t* out) {
    Sim* s = (Sim*)h;
    for (int64_t i = 0; i < n; i++) out[i] = jtk_cp_byte_pos(s->ix, s->doc_off.data(), s->dunit.data(), s->n_docs, doc[i], char_pos[i]);
}

// the word-at-a-time count against the per-byte weights, for every 4-byte word the test passes
int64_t sim_cp_word_mismatches(const uint32_t* words, int64_t n) {
    int64_t bad = 0;
    for (int64_t i = 0; i < n; i++)
        for (int unit = 0; unit < 3; unit++)
            for (int valid = 0; valid <= 4; valid++) {
                uint32_t want = 0;
                for (int k = 0; k < valid; k++) want += jtk_cp_weight((uint8_t)(words[i] >> (8 * k)), unit);
                if (jtk_cp_word_units(words[i], valid, unit) != want) bad++;
            }
    return bad;
}

int sim_cp_valid(int unit, int round) { return (jtk_cp_valid_unit(unit) ? 1 : 0) | (jtk_cp_valid_round(round) ? 2 : 0); }

}  // extern "C"
