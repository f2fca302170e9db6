// fim_sim -- the rule header jtokkit_amd/csrc/jtk_fim_rules.h compiled for the host and walked the way the kernels of
// jtk_fim.hip partition the work: one "lane" per offset for the cuts, one per document for the counts, a serial scan, and the
// gather in tiles of JTK_FIM_TILE cells with 256 lanes of 4 cells, every workgroup taking every n_blocks-th tile and every
// lane keeping its cursor from tile to tile.  Test infrastructure only (tests/test_fim_rules_cpu.py); no GPU.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../jtokkit_amd/csrc/jtk_fim_rules.h"

extern "C" {

int sim_fim_tile(void) { return JTK_FIM_TILE; }

// k_fim_cuts: kind [n_docs], cut [n_docs][2], sub_off [3 n_docs + 1]; returns whether the offsets are bad
int sim_fim_cuts(const uint8_t* text, const int64_t* doc_off, int64_t n_docs, int64_t n_bytes, uint64_t seed, int64_t doc_index_base,
                 uint32_t fim_rate, uint32_t spm_rate, uint8_t* kind, int64_t* cut, int64_t* sub_off) {
    int bad = 0;
    for (int64_t d = n_docs; d >= 0; d--) {                      // (any order: the lanes are independent)
        if (jtk_fim_offset_bad(doc_off, n_docs, n_bytes, d)) bad = 1;
        if (d == n_docs) { sub_off[3 * d] = doc_off[d]; continue; }
        jtk_fim_cuts_doc(text, doc_off, n_bytes, d, seed, doc_index_base, fim_rate, spm_rate, kind, cut, sub_off);
    }
    return bad;
}

// k_fim_count, the scan and k_fim_gather: status [n_docs], part_tok [n_docs][3], tok_off [n_docs + 1], tokens (NULL: count only);
// returns the token total
int64_t sim_fim_stitch(int64_t n_docs, int bad, const uint8_t* kind, const int64_t* sub_tok_off, const int32_t* sub_status,
                       const int32_t* sub_tokens, int32_t prefix_id, int32_t middle_id, int32_t suffix_id, int n_blocks,
                       int32_t* status, int64_t* part_tok, int64_t* tok_off, int32_t* tokens) {
    for (int64_t d = 0; d < n_docs; d++) tok_off[d] = jtk_fim_count_doc(d, bad != 0, kind, sub_tok_off, sub_status, status, part_tok);
    int64_t run = 0;
    for (int64_t d = 0; d < n_docs; d++) { const int64_t c = tok_off[d]; tok_off[d] = run; run += c; }
    tok_off[n_docs] = run;
    if (!tokens) return run;
    JtkFimView v;
    v.n_docs = n_docs; v.kind = kind; v.part_tok = part_tok; v.tok_off = tok_off; v.sub_tok_off = sub_tok_off; v.sub_tokens = sub_tokens;
    v.prefix_id = prefix_id; v.middle_id = middle_id; v.suffix_id = suffix_id;
    const int64_t total = run, n_tiles = (total + JTK_FIM_TILE - 1) / JTK_FIM_TILE;
    if (n_blocks < 1) n_blocks = 1;
    for (int blk = 0; blk < n_blocks; blk++) {
        std::vector<int64_t> cursor(256, 0);
        for (int64_t t = blk; t < n_tiles; t += n_blocks) {
            for (int lane = 0; lane < 256; lane++) {
                const int64_t e0 = t * JTK_FIM_TILE + lane * 4;
                if (e0 >= total) break;
                int32_t id[4] = {0, 0, 0, 0};
                const int n = jtk_fim_cells4(v, e0, total, &cursor[(size_t)lane], id);
                for (int j = 0; j < n; j++) tokens[e0 + j] = id[j];
            }
        }
    }
    return run;
}

}  // extern "C"
