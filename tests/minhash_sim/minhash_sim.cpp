// minhash_sim -- CPU shim of jtokkit_amd/csrc/jtk_minhash_rules.h for the tests: the rule header is included and a batch is
// walked the way the kernels of jtk_minhash.hip partition it.  A preset pass fills sig with 0xFFFFFFFF and n_shingles; then
// every tile of JTK_MH_TILE tokens first gets x of the shingles that start in it -- 64 lanes of 8 consecutive tokens, each lane
// searching the document of its first token and moving forward (the shingles read into the halo past the tile's end) -- and is
// then walked document by document: the minimum per hash function over the part's shingles, flushed at the document's end or
// the tile's, stored when the document lies inside the tile and min-combined into the preset row when it spans tiles.  Tiles
// are taken in the order `order` gives (0: ascending, 1: descending), which must not matter.  No GPU.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../jtokkit_amd/csrc/jtk_minhash_rules.h"

extern "C" {

int sim_mh_tile() { return JTK_MH_TILE; }
int sim_mh_block_tiles() { return JTK_MH_BLOCK_TILES; }
int sim_mh_lane_hashes() { return JTK_MH_LANE_HASHES; }
int sim_mh_max_hashes() { return JTK_MH_MAX_HASHES; }
int sim_mh_max_ngram() { return JTK_MH_MAX_NGRAM; }
uint64_t sim_mh_g() { return JTK_MH_G; }
uint32_t sim_mh_empty() { return JTK_MH_EMPTY; }
int sim_mh_params_ok(int32_t ngram, int32_t num_hashes, int32_t bands, uint32_t flags) { return jtk_mh_params_ok(ngram, num_hashes, bands, flags); }
uint32_t sim_mh_value(uint64_t a, uint64_t b, uint32_t x) { return jtk_mh_value((uint32_t)a, (uint32_t)(a >> 32), b, x); }

// sig[n_docs * K], n_shingles[n_docs], band_keys[n_docs * bands] (NULL: none).  Returns the number of row flushes that were
// min-combines (documents' parts in tiles they do not lie inside).
int64_t sim_mh_batch(const int32_t* tokens, const int64_t* tok_off, const int32_t* status, int64_t n_docs, uint64_t seed, int32_t ngram,
                     int32_t K, int32_t bands, int order, uint32_t* sig, int32_t* n_shingles, uint64_t* band_keys) {
    if (n_docs <= 0) return 0;
    const uint64_t key = jtk_mh_key(seed, ngram);
    JtkMhView v;
    v.tokens = tokens; v.tok_off = tok_off; v.status = status; v.n_docs = n_docs; v.total = tok_off[n_docs]; v.ngram = ngram;
    // the preset kernel
    for (int64_t i = 0; i < n_docs * K; i++) sig[i] = JTK_MH_EMPTY;
    for (int64_t d = 0; d < n_docs; d++) n_shingles[d] = (int32_t)jtk_mh_n_shingles(status[d] < 0 ? 0 : tok_off[d + 1] - tok_off[d], ngram);
    // the tiles
    const int64_t n_tiles = (v.total + JTK_MH_TILE - 1) / JTK_MH_TILE;
    const int lane_tokens = JTK_MH_TILE / 64;
    int64_t combines = 0;
    std::vector<uint32_t> xs(JTK_MH_TILE), mn(K);
    std::vector<uint64_t> a(K), b(K);                                  // (what the lanes hold in registers)
    for (int k = 0; k < K; k++) { a[k] = jtk_mh_a(key, k); b[k] = jtk_mh_b(key, k); }
    std::vector<uint8_t> have(JTK_MH_TILE);
    for (int64_t q = 0; q < n_tiles; q++) {
        const int64_t tile = order ? n_tiles - 1 - q : q;
        const int64_t w0 = tile * JTK_MH_TILE, w1 = w0 + JTK_MH_TILE < v.total ? w0 + JTK_MH_TILE : v.total;
        // step 1
        memset(have.data(), 0, have.size());
        for (int lane = 0; lane < 64; lane++) {
            const int64_t i0 = w0 + (int64_t)lane * lane_tokens;
            if (i0 >= v.total) continue;
            int64_t d = jtk_mh_doc_of(v, 0, i0);
            for (int j = 0; j < lane_tokens && i0 + j < v.total; j++) {
                const int64_t i = i0 + j;
                if (tok_off[d + 1] <= i) d = jtk_mh_next_doc(v, d, i);
                uint32_t x;
                if (jtk_mh_x_at(v, d, i, key, &x)) { xs[i - w0] = x; have[i - w0] = 1; }
            }
        }
        // step 2
        int64_t d = jtk_mh_doc_of(v, 0, w0), pos = w0;
        for (int k = 0; k < K; k++) mn[k] = JTK_MH_EMPTY;
        while (pos < w1) {
            const JtkMhSeg seg = jtk_mh_segment(v, d, pos, w0, w1);
            if (seg.live && seg.sh_hi > seg.sh_lo) {
                for (int64_t i = seg.sh_lo; i < seg.sh_hi; i++) {
                    if (!have[i - w0]) return -1;                      // (step 1 and step 2 disagree about where shingles start)
                    for (int k = 0; k < K; k++) {
                        const uint32_t val = jtk_mh_value((uint32_t)a[k], (uint32_t)(a[k] >> 32), b[k], xs[i - w0]);
                        mn[k] = val < mn[k] ? val : mn[k];
                    }
                }
                uint32_t* row = sig + d * K;
                for (int k = 0; k < K; k++) {
                    if (seg.whole) row[k] = mn[k];
                    else row[k] = mn[k] < row[k] ? mn[k] : row[k];
                    mn[k] = JTK_MH_EMPTY;
                }
                combines += !seg.whole;
            }
            pos = seg.end;
            if (pos < w1) d = jtk_mh_next_doc(v, d, pos);
        }
    }
    // the band kernel
    if (bands > 0 && band_keys)
        for (int64_t i = 0; i < n_docs * bands; i++) {
            const int64_t d = i / bands;
            band_keys[i] = jtk_mh_band_key(key, sig + d * K, K, bands, (int32_t)(i - d * bands));
        }
    return combines;
}

// agree[n_pairs]; a row is read only for a pair whose two indices are inside [0, n_sig)
void sim_mh_agree(const uint32_t* sig, int64_t n_sig, int32_t K, const int64_t* pair_a, const int64_t* pair_b, int64_t n_pairs, int32_t* agree) {
    for (int64_t p = 0; p < n_pairs; p++) {
        const int64_t a = pair_a[p], b = pair_b[p];
        agree[p] = (a >= 0 && a < n_sig && b >= 0 && b < n_sig) ? jtk_mh_agree(sig + a * K, sig + b * K, K) : -1;
    }
}

}  // extern "C"
