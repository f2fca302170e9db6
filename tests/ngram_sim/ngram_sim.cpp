// ngram_sim -- CPU shim of jtokkit_amd/csrc/jtk_ngram_rules.h for the tests: the rule header is included and a batch is walked
// the way the kernels of jtk_ngram.hip partition it -- tiles of JTK_NG_TILE tokens, 64 lanes of JTK_NG_LANE consecutive tokens,
// each lane searching the document of its first token and moving forward (jtk_ng_lane_keys).  The insert claims slots with a
// compare-and-swap that is plain here; the overlap looks the lanes' keys up, recomputes the starts of the n - 1 positions before
// the tile in lanes 33 - n .. 31 (jtk_ng_key_at), builds every lane's window word from its own bits, those of the four lanes
// before it and the halo (jtk_ng_window), and adds the lanes' per-document results into preset rows (jtk_ng_lane_docs).  Tiles
// are taken in ascending (order 0) or descending (1) order and the lanes of a tile, like the keys of an array, in an order
// shuffled by `shuffle`: none of it may matter for membership, counts and results.  No GPU.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../jtokkit_amd/csrc/jtk_ngram_rules.h"

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

JtkMhView view_of(const int32_t* tokens, const int64_t* tok_off, const int32_t* status, int64_t n_docs, int32_t ngram) {
    JtkMhView v;
    v.tokens = tokens; v.tok_off = tok_off; v.status = status; v.n_docs = n_docs; v.total = tok_off[n_docs]; v.ngram = ngram;
    return v;
}

}  // namespace

extern "C" {

int sim_ng_tile() { return JTK_NG_TILE; }
int sim_ng_lane() { return JTK_NG_LANE; }
int sim_ng_block_tiles() { return JTK_NG_BLOCK_TILES; }
int sim_ng_max_ngram() { return JTK_NG_MAX_NGRAM; }
int sim_ng_min_capacity() { return JTK_NG_MIN_CAPACITY; }
int sim_ng_start() { return JTK_NG_START; }
int sim_ng_covered() { return JTK_NG_COVERED; }
int sim_ng_params_ok(int32_t ngram, uint32_t flags) { return jtk_ng_params_ok(ngram, flags); }
uint64_t sim_ng_key(uint64_t seed, int32_t ngram) { return jtk_ng_key(seed, ngram); }
uint64_t sim_ng_finish(uint64_t h, uint64_t key) { return jtk_ng_finish(h, key); }
int64_t sim_ng_capacity(int64_t c, int64_t m) { return jtk_ng_capacity(c, m); }
// k of t[0 .. n) directly, and rolled from the n-gram before it (t[-1] must be readable)
uint64_t sim_ng_k(const int32_t* t, int32_t n, uint64_t key) { return jtk_ng_finish(jtk_ng_hash(t, n), key); }
uint64_t sim_ng_k_rolled(const int32_t* t, int32_t n, uint64_t key) {
    return jtk_ng_finish(jtk_ng_roll(jtk_ng_hash(t - 1, n), t[-1], t[n - 1], jtk_ng_pow(n)), key);
}
int sim_ng_lookup(const uint64_t* table, int64_t capacity, uint64_t k) { return jtk_ng_lookup(table, (uint64_t)capacity - 1, k); }

// the n-grams of the documents: what an insert of the batch adds at most
int64_t sim_ng_count(const int64_t* tok_off, const int32_t* status, int64_t n_docs, int32_t ngram) {
    int64_t n = 0;
    for (int64_t d = 0; d < n_docs; d++)
        if (status[d] >= 0) n += jtk_ng_n_ngrams(tok_off[d + 1] - tok_off[d], ngram);
    return n;
}

// keys[n] into table[capacity], zeros skipped (so an old table may be given: the rehash); the keys that were new
int64_t sim_ng_insert_keys(const uint64_t* keys, int64_t n, uint64_t* table, int64_t capacity, uint64_t shuffle) {
    int64_t added = 0;
    for (int64_t i : order_of(n, shuffle))
        if (keys[i]) added += jtk_ng_insert(table, (uint64_t)capacity - 1, keys[i], PlainCas());
    return added;
}

// every n-gram of the batch into table[capacity]; the keys that were new
int64_t sim_ng_insert_batch(const int32_t* tokens, const int64_t* tok_off, const int32_t* status, int64_t n_docs, uint64_t seed, int32_t ngram,
                            uint64_t* table, int64_t capacity, int order, uint64_t shuffle) {
    if (n_docs <= 0) return 0;
    const JtkMhView v = view_of(tokens, tok_off, status, n_docs, ngram);
    const uint64_t key = jtk_ng_key(seed, ngram), gn1 = jtk_ng_pow(ngram);
    const int64_t n_tiles = (v.total + JTK_NG_TILE - 1) / JTK_NG_TILE;
    int64_t added = 0;
    for (int64_t q = 0; q < n_tiles; q++) {
        const int64_t w0 = (order ? n_tiles - 1 - q : q) * JTK_NG_TILE;
        for (int64_t lane : order_of(64, shuffle ? shuffle + (uint64_t)q : 0)) {
            const int64_t i0 = w0 + lane * JTK_NG_LANE;
            if (i0 >= v.total) continue;
            uint64_t ks[JTK_NG_LANE];
            const uint32_t have = jtk_ng_lane_keys(v, key, gn1, i0, ks);
            for (int j = 0; j < JTK_NG_LANE; j++)
                if ((have >> j) & 1u) added += jtk_ng_insert(table, (uint64_t)capacity - 1, ks[j], PlainCas());
        }
    }
    return added;
}

// flags[total], n_hit / n_covered / first_hit [n_docs]; each may be NULL and is then not written.  Returns the number of
// per-document adds (what the kernel does with atomics), or -1 when a window word disagrees with the lanes' own bits.
int64_t sim_ng_overlap(const int32_t* tokens, const int64_t* tok_off, const int32_t* status, int64_t n_docs, uint64_t seed, int32_t ngram,
                       const uint64_t* table, int64_t capacity, int order, uint8_t* flags, int32_t* n_hit, int32_t* n_covered,
                       int64_t* first_hit) {
    if (n_docs <= 0) return 0;
    const JtkMhView v = view_of(tokens, tok_off, status, n_docs, ngram);
    const uint64_t key = jtk_ng_key(seed, ngram), gn1 = jtk_ng_pow(ngram), mask = (uint64_t)capacity - 1;
    // the preset kernel
    for (int64_t d = 0; d < n_docs; d++) {
        if (n_hit) n_hit[d] = 0;
        if (n_covered) n_covered[d] = 0;
        if (first_hit) first_hit[d] = -1;
    }
    const int64_t n_tiles = (v.total + JTK_NG_TILE - 1) / JTK_NG_TILE;
    int64_t adds = 0;
    for (int64_t q = 0; q < n_tiles; q++) {
        const int64_t w0 = (order ? n_tiles - 1 - q : q) * JTK_NG_TILE;
        uint32_t mine[64];
        uint32_t halo = 0;
        for (int lane = 0; lane < 64; lane++) {
            const int64_t i0 = w0 + (int64_t)lane * JTK_NG_LANE;
            mine[lane] = 0;
            if (i0 < v.total) {
                uint64_t ks[JTK_NG_LANE];
                const uint32_t have = jtk_ng_lane_keys(v, key, gn1, i0, ks);
                for (int j = 0; j < JTK_NG_LANE; j++)
                    if (((have >> j) & 1u) && jtk_ng_probe_on(table, mask, ks[j] & mask, table[ks[j] & mask], ks[j])) mine[lane] |= 1u << j;
            }
            const int64_t hp = w0 - 32 + lane;
            uint64_t k;
            if (lane < 32 && lane >= 33 - ngram && hp >= 0 && jtk_ng_key_at(v, key, hp, &k) && jtk_ng_lookup(table, mask, k)) halo |= 1u << lane;
        }
        for (int lane = 0; lane < 64; lane++) {
            const int64_t i0 = w0 + (int64_t)lane * JTK_NG_LANE;
            if (i0 >= v.total) continue;
            uint32_t before[4];
            for (int k = 1; k <= 4; k++) before[k - 1] = lane >= k ? mine[lane - k] : 0u;
            const uint64_t w = jtk_ng_window(mine[lane], before, halo, lane);
            if ((uint32_t)(w >> 31) != mine[lane]) return -1;
            if (flags)
                for (int j = 0; j < JTK_NG_LANE && i0 + j < v.total; j++) flags[i0 + j] = (uint8_t)jtk_ng_flag(w, ngram, j);
            if (n_hit || n_covered || first_hit)
                jtk_ng_lane_docs(v, i0, w, [&](int64_t d, int32_t hit, int32_t cov, int64_t first) {
                    if (n_hit && hit) n_hit[d] += hit;
                    if (n_covered && cov) n_covered[d] += cov;
                    if (first_hit && first >= 0 && (uint64_t)first < (uint64_t)first_hit[d]) first_hit[d] = first;
                    adds++;
                });
        }
    }
    return adds;
}

}  // extern "C"
