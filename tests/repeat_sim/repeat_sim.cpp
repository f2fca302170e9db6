// repeat_sim -- CPU shim of jtokkit_amd/csrc/jtk_repeat_rules.h for the tests: the rule header is included and a batch is walked
// the way jtk_batch_ngram_repeats and the kernels of jtk_repeat.hip do it.  The groups are planned by jtk_rp_group_end under a
// byte budget; each group gets a table of EXACTLY its capacity (one allocation of capacity * JTK_RP_SLOT_BYTES, laid out by
// jtk_rp_table_at, preset as the host presets it) and is walked in tiles of JTK_NG_TILE tokens of the batch's token array, 64
// lanes of JTK_NG_LANE tokens, restricted to the group's token range.  Pass 1 claims slots with a compare-and-swap that is plain
// here and merges a lane's runs (jtk_rp_lane_runs); pass 2 probes, decides the start bits, recomputes the halo, builds the window
// words (jtk_ng_window) and adds the lanes' per-document results and top offers.  Tiles are taken in ascending (order 0) or
// descending (1) order, the lanes of a tile in pass 1 in an order shuffled by `shuffle`: none of it may matter.  No GPU.
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../jtokkit_amd/csrc/jtk_repeat_rules.h"

namespace {

struct PlainCas {
    uint64_t operator()(uint64_t* p, uint64_t k) const {
        const uint64_t old = *p;
        if (old == 0) *p = k;
        return old;
    }
};

// a permutation of 0 .. n - 1 (Fisher-Yates on an LCG); the identity for shuffle == 0
std::vector<int64_t> order_of(int64_t n, uint64_t shuffle) {
    std::vector<int64_t> p((size_t)n);
    for (int64_t i = 0; i < n; i++) p[(size_t)i] = i;
    uint64_t x = shuffle;
    for (int64_t i = n - 1; i > 0 && shuffle; i--) {
        x = x * 6364136223846793005ull + 1442695040888963407ull;
        const int64_t j = (int64_t)((x >> 33) % (uint64_t)(i + 1));
        const int64_t t = p[(size_t)i]; p[(size_t)i] = p[(size_t)j]; p[(size_t)j] = t;
    }
    return p;
}

}  // namespace

extern "C" {

int sim_rp_start() { return JTK_RP_START; }
int sim_rp_covered() { return JTK_RP_COVERED; }
int sim_rp_mark_first() { return (int)JTK_REPEAT_MARK_FIRST; }
int sim_rp_max_ngram() { return JTK_RP_MAX_NGRAM; }
int sim_rp_slot_bytes() { return JTK_RP_SLOT_BYTES; }
int sim_rp_min_table_bytes() { return JTK_RP_MIN_TABLE_BYTES; }
int64_t sim_rp_max_doc_tokens() { return JTK_RP_MAX_DOC_TOKENS; }
int sim_rp_tile() { return JTK_NG_TILE; }
int sim_rp_lane() { return JTK_NG_LANE; }
int sim_rp_block_tiles() { return JTK_NG_BLOCK_TILES; }
int sim_rp_params_ok(int32_t ngram, uint32_t flags) { return jtk_rp_params_ok(ngram, flags); }
uint64_t sim_rp_key(uint64_t seed, int32_t ngram) { return jtk_rp_key(seed, ngram); }
uint64_t sim_rp_doc_key(uint64_t key, uint64_t base, int64_t d) { return jtk_rp_doc_key(key, base, d); }
int64_t sim_rp_capacity(int64_t m) { return jtk_rp_capacity(m); }
uint64_t sim_rp_top_pack(uint32_t count, int64_t rel) { return jtk_rp_top_pack(count, rel); }
int32_t sim_rp_top_count(uint64_t packed) { return jtk_rp_top_count(packed); }
int64_t sim_rp_top_first(uint64_t packed) { return jtk_rp_top_first(packed); }

// k of the n-gram that starts at every token of the batch, 0 where none does: the lanes' walk (rolled within a document) and,
// where check != 0, the direct form of the halo beside it (-1 when the two disagree)
int sim_rp_keys(const int32_t* tokens, const int64_t* tok_off, const int32_t* status, int64_t n_docs, uint64_t seed, uint64_t base, int32_t ngram,
                int check, uint64_t* out) {
    if (n_docs <= 0) return 0;
    JtkMhView v;
    v.tokens = tokens; v.tok_off = tok_off; v.status = status; v.n_docs = n_docs; v.total = tok_off[n_docs]; v.ngram = ngram;
    const uint64_t key = jtk_rp_key(seed, ngram), gn1 = jtk_ng_pow(ngram);
    for (int64_t i0 = 0; i0 < v.total; i0 += JTK_NG_LANE) {
        uint64_t ks[JTK_NG_LANE];
        const uint32_t have = jtk_rp_lane_keys(v, key, base, gn1, i0, 0, v.total, ks);
        for (int j = 0; j < JTK_NG_LANE && i0 + j < v.total; j++) {
            out[i0 + j] = ((have >> j) & 1u) ? ks[j] : 0;
            uint64_t k = 0;
            if (check && (jtk_rp_key_at(v, key, base, i0 + j, &k) ? k : 0) != out[i0 + j]) return -1;
        }
    }
    return 0;
}

// The whole call.  tok_flags[total], n_repeat / n_covered / top_count / top_first [n_docs]; each may be NULL and is then not
// written.  info[0] = the groups, info[1] = the largest capacity, info[2] = the pairs of atomics pass 1 issued (runs), info[3] =
// the n-grams it inserted.  Returns 0, -1 when a window word disagrees with the lane's own bits, -2 when a probe of pass 2 does
// not find its key, -3 without memory.
int sim_rp_repeats(const int32_t* tokens, const int64_t* tok_off, const int32_t* status, int64_t n_docs, uint64_t seed, uint64_t base, int32_t ngram,
                   uint32_t mode, int64_t budget, int order, uint64_t shuffle, uint8_t* tok_flags, int32_t* n_repeat, int32_t* n_covered,
                   int32_t* top_count, int64_t* top_first, int64_t* info) {
    info[0] = info[1] = info[2] = info[3] = 0;
    if (n_docs <= 0) return 0;
    JtkMhView v;
    v.tokens = tokens; v.tok_off = tok_off; v.status = status; v.n_docs = n_docs; v.total = tok_off[n_docs]; v.ngram = ngram;
    const uint64_t key = jtk_rp_key(seed, ngram), gn1 = jtk_ng_pow(ngram);
    const bool want_top = top_count || top_first;
    std::vector<uint64_t> top(want_top ? (size_t)n_docs : 0, 0);
    // the preset kernel
    for (int64_t d = 0; d < n_docs; d++) {
        if (n_repeat) n_repeat[d] = 0;
        if (n_covered) n_covered[d] = 0;
    }
    for (int64_t d0 = 0; d0 < n_docs;) {
        int64_t m = 0;
        const int64_t d1 = jtk_rp_group_end(tok_off, status, n_docs, ngram, d0, budget, &m);
        const int64_t lo = tok_off[d0], hi = tok_off[d1];
        d0 = d1;
        info[0]++;
        if (hi <= lo) continue;
        if (m == 0) {
            if (tok_flags) memset(tok_flags + lo, 0, (size_t)(hi - lo));
            continue;
        }
        const int64_t cap = jtk_rp_capacity(m);
        if (cap > info[1]) info[1] = cap;
        void* mem = malloc((size_t)cap * JTK_RP_SLOT_BYTES);       // exactly the table: a probe that leaves it is caught
        if (!mem) return -3;
        const JtkRpTable t = jtk_rp_table_at(mem, cap);
        memset(t.key, 0, (size_t)cap * 12);
        memset(t.first, 0xFF, (size_t)cap * 8);
        const int64_t tile0 = lo / JTK_NG_TILE, n_tiles = (hi + JTK_NG_TILE - 1) / JTK_NG_TILE - tile0;
        // pass 1
        for (int64_t q = 0; q < n_tiles; q++) {
            const int64_t w0 = (tile0 + (order ? n_tiles - 1 - q : q)) * JTK_NG_TILE;
            for (int64_t lane : order_of(64, shuffle ? shuffle + (uint64_t)q : 0)) {
                const int64_t i0 = w0 + lane * JTK_NG_LANE;
                if (i0 >= hi || i0 + JTK_NG_LANE <= lo) continue;
                uint64_t ks[JTK_NG_LANE];
                const uint32_t have = jtk_rp_lane_keys(v, key, base, gn1, i0, lo, hi, ks);
                jtk_rp_lane_runs(have, ks, i0, [&](uint64_t k, int64_t at, uint32_t r) {
                    const uint64_t slot = jtk_rp_claim(t.key, t.mask, k, PlainCas());
                    if ((uint64_t)at < t.first[slot]) t.first[slot] = (uint64_t)at;
                    t.count[slot] += r;
                    info[2]++;
                    info[3] += r;
                });
            }
        }
        // pass 2
        int rc = 0;
        for (int64_t q = 0; q < n_tiles && rc == 0; q++) {
            const int64_t w0 = (tile0 + (order ? n_tiles - 1 - q : q)) * JTK_NG_TILE;
            uint32_t mine[64], have[64];
            uint64_t first[64][JTK_NG_LANE];
            uint32_t count[64][JTK_NG_LANE];
            uint32_t halo = 0;
            for (int lane = 0; lane < 64; lane++) {
                const int64_t i0 = w0 + (int64_t)lane * JTK_NG_LANE;
                mine[lane] = have[lane] = 0;
                if (i0 < hi && i0 + JTK_NG_LANE > lo) {
                    uint64_t ks[JTK_NG_LANE];
                    have[lane] = jtk_rp_lane_keys(v, key, base, gn1, i0, lo, hi, ks);
                    for (int j = 0; j < JTK_NG_LANE; j++)
                        if ((have[lane] >> j) & 1u) {
                            const uint64_t slot = jtk_rp_find_on(t.key, t.mask, ks[j] & t.mask, t.key[ks[j] & t.mask], ks[j]);
                            if (t.key[slot] != ks[j]) rc = -2;
                            first[lane][j] = t.first[slot];
                            count[lane][j] = t.count[slot];
                            if (jtk_rp_is_repeat(mode, i0 + j, first[lane][j], count[lane][j])) mine[lane] |= 1u << j;
                        }
                }
                const int64_t hp = w0 - 32 + lane;
                uint64_t k;
                if (lane < 32 && lane >= 33 - ngram && hp >= lo && hp < hi && w0 < hi && jtk_rp_key_at(v, key, base, hp, &k)) {
                    const uint64_t slot = jtk_rp_find(t.key, t.mask, k);
                    if (jtk_rp_is_repeat(mode, hp, t.first[slot], t.count[slot])) halo |= 1u << lane;
                }
            }
            for (int lane = 0; lane < 64; lane++) {
                const int64_t i0 = w0 + (int64_t)lane * JTK_NG_LANE;
                if (!(i0 < hi && i0 + JTK_NG_LANE > lo)) continue;
                uint32_t before[4];
                for (int k = 1; k <= 4; k++) before[k - 1] = lane >= k ? mine[lane - k] : 0u;
                const uint64_t w = jtk_ng_window(mine[lane], before, halo, lane);
                if ((uint32_t)(w >> 31) != mine[lane]) rc = -1;
                if (tok_flags)
                    for (int j = 0; j < JTK_NG_LANE; j++)
                        if (i0 + j >= lo && i0 + j < hi) tok_flags[i0 + j] = (uint8_t)jtk_ng_flag(w, ngram, j);
                if (n_repeat || n_covered) {
                    JtkMhView vv = v;
                    vv.total = hi;
                    jtk_ng_lane_docs(vv, i0, w, [&](int64_t d, int32_t hit, int32_t cov, int64_t) {
                        if (n_repeat && hit) n_repeat[d] += hit;
                        if (n_covered && cov) n_covered[d] += cov;
                    });
                }
                if (want_top)
                    jtk_rp_lane_top(v, i0, have[lane], first[lane], count[lane], [&](int64_t d, uint64_t packed) {
                        if (packed > top[(size_t)d]) top[(size_t)d] = packed;
                    });
            }
        }
        free(mem);
        if (rc) return rc;
    }
    // the top kernel
    for (int64_t d = 0; d < n_docs && want_top; d++) {
        if (top_count) top_count[d] = jtk_rp_top_count(top[(size_t)d]);
        if (top_first) top_first[d] = jtk_rp_top_first(top[(size_t)d]);
    }
    return 0;
}

}  // extern "C"
