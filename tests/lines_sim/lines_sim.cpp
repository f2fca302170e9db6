// lines_sim -- the CPU shim of the line / paragraph pass (jtk_batch_line_units, jtk_batch_line_repeats): the rule header
// jtokkit_amd/csrc/jtk_lines_rules.h, walked serially the way jtk_lines.hip partitions the text -- the two bit planes, pass A
// (a summary per tile of 4096 bytes, granule by granule), pass B (the scan of the summaries, forward and backward), pass C (the
// write pass with the carries), the per-document offsets, one k per unit, then the groups of jtk_abi.cpp with a table of exactly
// the group's capacity.  Tiles are taken ascending or descending (`order`), the inserts of pass 1 in a shuffled order
// (`shuffle`).  Every output may be NULL and is then not written.  No GPU, no HIP.
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../jtokkit_amd/csrc/jtk_lines_rules.h"

namespace {

struct Planes {
    std::vector<uint16_t> edge, ref;
    void set(std::vector<uint16_t>& p, int64_t q) { p[(size_t)(q >> 4)] |= (uint16_t)(1u << (q & 15)); }
};
struct Tiles {
    std::vector<uint32_t> word, units, chars, cf, cb;
    std::vector<uint64_t> hash, p0;
    std::vector<int64_t> u0, c0;
};
struct Units {
    std::vector<int64_t> begin, end, chars, ce;
    std::vector<uint64_t> k, pe;
};

int64_t clampq(int64_t v, int64_t n) { return v < 0 ? 0 : v > n ? n : v; }

struct Sim {
    const uint8_t* text; int64_t n_bytes; const int64_t* doc_off; const int32_t* status; int64_t n_docs;
    int32_t unit; uint32_t flags;
    Planes pl; Tiles tl; Units un;
    std::vector<int64_t> doc_units, doc_chars, unit_off, char_off;
    int64_t n_units = 0;

    // one tile, granule by granule; write = pass C
    void tile(int64_t t, bool write) {
        const uint32_t thr = jtk_ln_threshold(unit);
        const int64_t d0 = jtk_ln_doc_at(doc_off, n_docs, t * JTK_LN_TILE);
        uint32_t r = (d0 < 0 || d0 >= n_docs || status[d0] < 0) ? 1u : 0u;
        JtkLnGran gr[JTK_LN_TILE_GRANULES];
        uint32_t edge[JTK_LN_TILE_GRANULES], eend[JTK_LN_TILE_GRANULES], w4[JTK_LN_TILE_GRANULES][4];
        int valid[JTK_LN_TILE_GRANULES];
        for (int i = 0; i < JTK_LN_TILE_GRANULES; i++) {
            const int64_t g = t * JTK_LN_TILE_GRANULES + i, g0 = g * JTK_LN_GRANULE, left = n_bytes - g0;
            valid[i] = left >= JTK_LN_GRANULE ? JTK_LN_GRANULE : left > 0 ? (int)left : 0;
            memset(w4[i], 0, 16);
            if (valid[i] > 0) memcpy(w4[i], text + g0, (size_t)valid[i]);      // (the device reads the whole granule: the text is padded there)
            const uint32_t e32 = (uint32_t)pl.edge[(size_t)g] | ((uint32_t)pl.edge[(size_t)g + 1] << 16), vmask = (1u << valid[i]) - 1u;
            edge[i] = e32 & vmask;
            eend[i] = (e32 >> 1) & vmask;
            const uint32_t refused = jtk_ln_refused_mask(edge[i], pl.ref[(size_t)g] & vmask, r, &r);
            gr[i] = jtk_ln_classify(w4[i], valid[i], flags, refused);
        }
        if (!write) {
            uint32_t tf = JTK_LN_T_ID, tb = JTK_LN_T_ID, open = 0, units = 0, chars = 0;
            uint64_t h = 0;
            for (int i = 0; i < JTK_LN_TILE_GRANULES; i++) {
                units += (uint32_t)__builtin_popcount(jtk_ln_starts(gr[i], edge[i], tf, thr, &open));
                tf = jtk_ln_then(tf, jtk_ln_gran_fwd(gr[i], edge[i]));
                tb = jtk_ln_then(tb, jtk_ln_gran_bwd(gr[JTK_LN_TILE_GRANULES - 1 - i], eend[JTK_LN_TILE_GRANULES - 1 - i]));
                chars += (uint32_t)__builtin_popcount(gr[i].nonc);
                h = h * jtk_ln_pow(JTK_LN_GRANULE) + jtk_ln_gran_hash(w4[i]);
            }
            tl.word[(size_t)t] = jtk_ln_tile_word(tf, tb, open);
            tl.units[(size_t)t] = units; tl.chars[(size_t)t] = chars; tl.hash[(size_t)t] = h;
            return;
        }
        uint32_t ends[JTK_LN_TILE_GRANULES];
        uint32_t sb = tl.cb[(size_t)t];
        for (int i = JTK_LN_TILE_GRANULES - 1; i >= 0; i--) {
            ends[i] = jtk_ln_ends(gr[i], eend[i], sb, thr);
            sb = jtk_ln_apply(jtk_ln_gran_bwd(gr[i], eend[i]), sb);
        }
        uint32_t tf = jtk_ln_fix(tl.cf[(size_t)t]);
        int64_t u = tl.u0[(size_t)t], ch = tl.c0[(size_t)t];
        uint64_t H = tl.p0[(size_t)t];
        for (int i = 0; i < JTK_LN_TILE_GRANULES; i++) {
            uint32_t open = 0;
            const uint32_t starts = jtk_ln_starts(gr[i], edge[i], tf, thr, &open);
            if (open) abort();                                   // (pass C knows every state)
            tf = jtk_ln_then(tf, jtk_ln_gran_fwd(gr[i], edge[i]));
            const int64_t g0 = (t * JTK_LN_TILE_GRANULES + i) * JTK_LN_GRANULE;
            for (int j = 0; j < JTK_LN_GRANULE; j++) {
                const int64_t p = g0 + j;
                if ((edge[i] >> j) & 1u) {
                    const int64_t d = jtk_ln_doc_at(doc_off, n_docs, p);
                    if (d >= 0 && d < n_docs) { doc_units[(size_t)d] = u; doc_chars[(size_t)d] = ch; }
                }
                if ((starts >> j) & 1u) { un.begin.at((size_t)u) = p; un.k.at((size_t)u) = H; un.chars.at((size_t)u) = ch; u++; }
                ch += (gr[i].nonc >> j) & 1u;
                H = jtk_ln_step(H, (w4[i][j >> 2] >> (8 * (j & 3))) & 0xFFu);
                if ((ends[i] >> j) & 1u) { un.end.at((size_t)u - 1) = p + 1; un.pe.at((size_t)u - 1) = H; un.ce.at((size_t)u - 1) = ch; }
            }
        }
    }

    int64_t find_units(int order, uint64_t seed, uint64_t base) {
        const int64_t n_tiles = (n_bytes + JTK_LN_TILE - 1) / JTK_LN_TILE;
        const size_t words = (size_t)n_tiles * JTK_LN_TILE_GRANULES + 2;
        pl.edge.assign(words, 0); pl.ref.assign(words, 0);
        for (int64_t d = 0; d <= n_docs; d++) {
            const int64_t q = clampq(doc_off[d], n_bytes);
            bool mark = true, refused = true;
            if (d < n_docs) { mark = clampq(doc_off[d + 1], n_bytes) > q; refused = status[d] < 0; }
            if (!mark) continue;
            pl.set(pl.edge, q);
            if (refused) pl.set(pl.ref, q);
        }
        const size_t nt = (size_t)n_tiles;
        tl.word.assign(nt, 0); tl.units.assign(nt, 0); tl.chars.assign(nt, 0); tl.cf.assign(nt, 0); tl.cb.assign(nt, 0);
        tl.hash.assign(nt, 0); tl.p0.assign(nt, 0); tl.u0.assign(nt, 0); tl.c0.assign(nt, 0);
        for (int64_t i = 0; i < n_tiles; i++) tile(order ? n_tiles - 1 - i : i, false);
        // pass B
        const uint32_t thr = jtk_ln_threshold(unit);
        uint32_t s = JTK_LN_NOINK;
        int64_t u = 0, c = 0;
        uint64_t P = 0;
        for (int64_t t = 0; t < n_tiles; t++) {
            tl.cf[(size_t)t] = s; tl.u0[(size_t)t] = u; tl.c0[(size_t)t] = c; tl.p0[(size_t)t] = P;
            u += tl.units[(size_t)t] + jtk_ln_open_starts(jtk_ln_word_open(tl.word[(size_t)t]), s, thr);
            c += tl.chars[(size_t)t];
            P = P * jtk_ln_pow(JTK_LN_TILE) + tl.hash[(size_t)t];
            s = jtk_ln_apply(jtk_ln_word_fwd(tl.word[(size_t)t]), s);
        }
        s = JTK_LN_NOINK;
        for (int64_t t = n_tiles - 1; t >= 0; t--) {
            tl.cb[(size_t)t] = s;
            s = jtk_ln_apply(jtk_ln_word_bwd(tl.word[(size_t)t]), s);
        }
        n_units = u;
        const size_t n = (size_t)n_units;                        // the list at its exact size
        un.begin.assign(n, -1); un.end.assign(n, -1); un.chars.assign(n, 0); un.ce.assign(n, 0); un.k.assign(n, 0); un.pe.assign(n, 0);
        doc_units.assign((size_t)n_docs + 1, -1); doc_chars.assign((size_t)n_docs + 1, -1);
        doc_units[(size_t)n_docs] = u; doc_chars[(size_t)n_docs] = c;
        for (int64_t i = 0; i < n_tiles; i++) tile(order ? n_tiles - 1 - i : i, true);
        unit_off.assign((size_t)n_docs + 1, 0); char_off.assign((size_t)n_docs + 1, 0);
        for (int64_t d = 0; d <= n_docs; d++) {
            int64_t at = jtk_ln_doc_at(doc_off, n_docs, clampq(doc_off[d], n_bytes));
            if (at < 0) at = 0;
            if (d == n_docs) at = n_docs;
            unit_off[(size_t)d] = doc_units[(size_t)at];
            char_off[(size_t)d] = doc_chars[(size_t)at];
        }
        const uint64_t key = jtk_ln_key(seed, unit);
        for (int64_t i = 0; i < n_units; i++) {
            const int64_t d = jtk_ln_doc_of_unit(unit_off.data(), n_docs, i);
            const uint64_t h = jtk_ln_range_hash(un.k[(size_t)i], un.pe[(size_t)i], un.end[(size_t)i] - un.begin[(size_t)i]);
            un.k[(size_t)i] = jtk_ln_finish(h, jtk_rp_doc_key(key, base, d));
            un.chars[(size_t)i] = un.ce[(size_t)i] - un.chars[(size_t)i];
        }
        return n_units;
    }
};

}  // namespace

extern "C" {

int sim_ln_granule() { return JTK_LN_GRANULE; }
int sim_ln_wave_bytes() { return JTK_LN_WAVE_BYTES; }
int sim_ln_tile() { return JTK_LN_TILE; }
int sim_ln_scan_step() { return JTK_LN_SCAN_STEP; }
int sim_ln_key_c() { return JTK_LN_KEY_C; }
int sim_ln_unit_bytes() { return JTK_LN_UNIT_BYTES; }
int64_t sim_ln_max_doc_units() { return JTK_LN_MAX_DOC_UNITS; }
int sim_ln_params_ok(int32_t unit, uint32_t flags) { return jtk_ln_params_ok(unit, flags) ? 1 : 0; }
uint64_t sim_ln_key(uint64_t seed, int32_t unit) { return jtk_ln_key(seed, unit); }
uint64_t sim_ln_pow(uint64_t e) { return jtk_ln_pow(e); }
uint32_t sim_ln_then(uint32_t a, uint32_t b) { return jtk_ln_then(a, b); }
uint32_t sim_ln_apply(uint32_t t, uint32_t s) { return jtk_ln_apply(t, s); }

// info: [0] groups, [1] the largest group's units, [2] probe steps of pass 1 that wrapped to slot 0, [3] units
int sim_ln_repeats(const uint8_t* text, int64_t n_bytes, const int64_t* doc_off, const int32_t* status, int64_t n_docs, uint64_t seed, uint64_t base,
                   int32_t unit, uint32_t flags, int64_t budget, int order, uint64_t shuffle, int64_t* unit_begin, int64_t* unit_end,
                   uint8_t* unit_flags, int64_t* unit_off, int32_t* n_dup, int64_t* dup_bytes, int64_t* dup_chars, int64_t* unit_bytes,
                   int64_t* unit_chars, int64_t* doc_chars, int32_t* top_count, int64_t* top_first, uint64_t* unit_k, int64_t* info) {
    if (!jtk_ln_params_ok(unit, flags)) return 1;
    Sim s{text, n_bytes, doc_off, status, n_docs, unit, flags};
    const int64_t n = s.find_units(order, seed, base);
    info[0] = info[1] = info[2] = 0; info[3] = n;
    for (int64_t u = 0; u < n; u++) {
        if (unit_begin) unit_begin[u] = s.un.begin[(size_t)u];
        if (unit_end) unit_end[u] = s.un.end[(size_t)u];
        if (unit_k) unit_k[u] = s.un.k[(size_t)u];
    }
    std::vector<uint64_t> top((size_t)n_docs, 0);
    for (int64_t d = 0; d < n_docs; d++) {
        if (s.unit_off[(size_t)d + 1] - s.unit_off[(size_t)d] > JTK_LN_MAX_DOC_UNITS) return 2;
        if (n_dup) n_dup[d] = 0;
        if (dup_bytes) dup_bytes[d] = 0;
        if (dup_chars) dup_chars[d] = 0;
        if (unit_bytes) unit_bytes[d] = 0;
        if (unit_chars) unit_chars[d] = 0;
        if (doc_chars) doc_chars[d] = s.char_off[(size_t)d + 1] - s.char_off[(size_t)d];
    }
    if (unit_off) for (int64_t d = 0; d <= n_docs; d++) unit_off[d] = s.unit_off[(size_t)d];
    uint64_t rng = shuffle * 0x9E3779B97F4A7C15ull + 1;
    for (int64_t d0 = 0; d0 < n_docs;) {
        int64_t m = 0;
        const int64_t d1 = jtk_ln_group_end(s.unit_off.data(), n_docs, d0, budget, &m);
        const int64_t lo = s.unit_off[(size_t)d0], hi = s.unit_off[(size_t)d1];
        d0 = d1;
        info[0]++;
        if (m > info[1]) info[1] = m;
        if (m == 0) continue;
        const int64_t cap = jtk_rp_capacity(m);
        void* mem = malloc((size_t)cap * JTK_RP_SLOT_BYTES);     // exactly the table
        if (!mem) return 3;
        const JtkRpTable t = jtk_rp_table_at(mem, cap);
        memset(t.key, 0, (size_t)cap * 12);
        memset(t.first, 0xFF, (size_t)cap * 8);
        std::vector<int64_t> ord;
        for (int64_t u = lo; u < hi; u++) ord.push_back(u);
        if (shuffle)
            for (size_t i = ord.size(); i > 1; i--) {
                rng = rng * 6364136223846793005ull + 1442695040888963407ull;
                std::swap(ord[i - 1], ord[(size_t)((rng >> 33) % i)]);
            }
        for (int64_t u : ord) {
            uint64_t prev = s.un.k[(size_t)u] & t.mask;
            bool started = false;
            const uint64_t slot = jtk_rp_claim(t.key, t.mask, s.un.k[(size_t)u], [&](uint64_t* p, uint64_t k) {
                const uint64_t at = (uint64_t)(p - t.key);
                if (started && at == 0 && prev == t.mask) info[2]++;
                started = true; prev = at;
                const uint64_t old = *p;
                if (old == 0) *p = k;
                return old;
            });
            if (t.first[slot] > (uint64_t)u) t.first[slot] = (uint64_t)u;
            t.count[slot]++;
        }
        for (int64_t u = lo; u < hi; u++) {
            const uint64_t slot = jtk_rp_find(t.key, t.mask, s.un.k[(size_t)u]);
            const uint64_t first = t.first[slot];
            const uint32_t count = t.count[slot];
            const bool rep = jtk_rp_is_repeat(flags & JTK_LINES_MARK_FIRST, u, first, count);
            if (unit_flags) unit_flags[u] = rep ? 1 : 0;
            const int64_t d = jtk_ln_doc_of_unit(s.unit_off.data(), n_docs, u);
            const int64_t bytes = s.un.end[(size_t)u] - s.un.begin[(size_t)u], chars = s.un.chars[(size_t)u];
            if (unit_bytes) unit_bytes[d] += bytes;
            if (unit_chars) unit_chars[d] += chars;
            if (rep) {
                if (n_dup) n_dup[d]++;
                if (dup_bytes) dup_bytes[d] += bytes;
                if (dup_chars) dup_chars[d] += chars;
            }
            if (first == (uint64_t)u) top[(size_t)d] = std::max(top[(size_t)d], jtk_rp_top_pack(count, u - s.unit_off[(size_t)d]));
        }
        free(mem);
    }
    for (int64_t d = 0; d < n_docs; d++) {
        if (top_count) top_count[d] = jtk_rp_top_count(top[(size_t)d]);
        if (top_first) top_first[d] = jtk_rp_top_first(top[(size_t)d]);
    }
    return 0;
}

}  // extern "C"
