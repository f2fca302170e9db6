// jtk_ngram_rules.h -- token n-gram sets and overlap for benchmark decontamination (jtk_ngram_set_*, jtk_batch_ngram_overlap): the
// rule the device kernels (jtk_ngram.hip) and the CPU test shim tests/ngram_sim share.  A corpus document is flagged, and the
// exact token ranges marked, where it shares a token n-gram with a set of held-out texts (Brown et al., "Language Models are
// Few-Shot Learners", appendix C: 13-grams).  Integer only: every result is exact.
//
// The rule, all arithmetic modulo 2^64; G = JTK_MH_G, mix = the splitmix64 finaliser (jtk_fim_mix):
//   key         = mix(seed + G * (n + 33)), n = ngram in 1..32 (MinHash has n + 1: the two families never share a key).
//   n-grams     of a document of l tokens t[0 .. l) (the int32 ids of the encode: special ids, FIM sentinels and pseudo ids
//               count as ids): the windows t[i .. i + n), 0 <= i <= l - n.  None when l < n -- not MinHash's short-document
//               rule: a 3-token document must not match as a 13-gram -- and none when the document's status < 0.
//               n_ngrams = max(l - n + 1, 0).
//   H           = H * G + (uint32)id + 1 over the n ids, from 0;  k = mix(H ^ key), and G where that is 0 (0 is the empty slot).
//               Membership is membership of k: a 64-bit collision is part of the rule.
//   set         the distinct k inserted so far, in a table of C 64-bit slots, C a power of two: home slot k & (C - 1), linear
//               probing with wrap-around; a lookup ends at the first empty slot or at a match.  Before an insert of at most m
//               new keys into a set of c keys the capacity becomes the smallest power of two >= max(64, 2 (c + m)) when that
//               is larger (it never shrinks): m = the keys given for add_keys (duplicates and all), the sum of n_ngrams over the
//               batch's documents for add_batch.  A new set has 64 slots.  Where a key lands depends on the insertion order;
//               membership, the key count and the capacity do not.
//   per token   p of document d, a byte: JTK_NG_START when an n-gram starts at p and its k is in the set; JTK_NG_COVERED when a
//               start-flagged position i of the same document has p - n < i <= p.  A start at i implies i + n <= the document's
//               end, so the tokens a start covers are its document's, and a start more than n - 1 tokens back -- in another
//               document or not -- covers nothing here: the window of the n positions up to p needs no document test.
//   per doc     n_hit = the start flags, n_covered = the covered tokens, first_hit = the document-relative index of the first
//               start, or -1.
//
// How the kernels walk a batch (and the shim with them): tiles of JTK_NG_TILE tokens, one wave each; a lane takes JTK_NG_LANE
// consecutive tokens, finds the document of the first by one search over tok_off and moves forward (jtk_ng_lane_keys: the first k
// of a run directly, the following ones rolled).  For the overlap a lane needs the start bits of the 31 positions before its own
// 8: those of the four lanes before it, and for the tile's first four lanes the starts of the n - 1 positions BEFORE the tile,
// which the tile recomputes (jtk_ng_key_at: the backward halo), so that no tile waits for another.  Per-document results are
// gathered by each lane over the documents of its 8 tokens and added into rows preset by an earlier kernel.
#ifndef JTK_NGRAM_RULES_H
#define JTK_NGRAM_RULES_H

#include <stdint.h>

#include "jtk_minhash_rules.h"     // JTK_MH_G, JtkMhView and the walk over tok_off (jtk_mh_doc_of, jtk_mh_next_doc); jtk_fim_mix

#define JTK_NG_HD JTK_MH_HD

#ifndef JTK_NG_START
#define JTK_NG_START 1             // (as in include/jtokkit_amd.h)
#define JTK_NG_COVERED 2
#endif
#define JTK_NG_MAX_NGRAM 32
#define JTK_NG_MIN_CAPACITY 64
#define JTK_NG_TILE 512            // tokens per wave
#define JTK_NG_LANE 8              // consecutive tokens per lane
#define JTK_NG_BLOCK_TILES 4       // tiles (waves) per workgroup

JTK_NG_HD bool jtk_ng_params_ok(int32_t ngram, uint32_t flags) { return flags == 0 && ngram >= 1 && ngram <= JTK_NG_MAX_NGRAM; }
JTK_NG_HD uint64_t jtk_ng_key(uint64_t seed, int32_t ngram) { return jtk_fim_mix(seed + JTK_MH_G * ((uint64_t)ngram + 33ull)); }
JTK_NG_HD int64_t jtk_ng_n_ngrams(int64_t l, int32_t ngram) { return l < ngram ? 0 : l - ngram + 1; }

// G^(n - 1): what the id that leaves a rolled window was multiplied by
JTK_NG_HD uint64_t jtk_ng_pow(int32_t ngram) {
    uint64_t g = 1;
    for (int j = 1; j < ngram; j++) g *= JTK_MH_G;
    return g;
}
JTK_NG_HD uint64_t jtk_ng_term(int32_t id) { return (uint64_t)(uint32_t)id + 1ull; }
JTK_NG_HD uint64_t jtk_ng_hash(const int32_t* t, int n) {
    uint64_t h = 0;
    for (int j = 0; j < n; j++) h = h * JTK_MH_G + jtk_ng_term(t[j]);
    return h;
}
// H of t[1 .. n] from H of t[0 .. n)
JTK_NG_HD uint64_t jtk_ng_roll(uint64_t h, int32_t out, int32_t in, uint64_t gn1) {
    return (h - jtk_ng_term(out) * gn1) * JTK_MH_G + jtk_ng_term(in);
}
JTK_NG_HD uint64_t jtk_ng_finish(uint64_t h, uint64_t key) {
    const uint64_t k = jtk_fim_mix(h ^ key);
    return k ? k : JTK_MH_G;
}

// ---- the set
JTK_NG_HD int64_t jtk_ng_capacity(int64_t c, int64_t m) {
    const int64_t need = 2 * (c + m);
    int64_t cap = JTK_NG_MIN_CAPACITY;
    while (cap < need) cap <<= 1;
    return cap;
}
// the rest of a lookup whose slot `slot` held `seen`
JTK_NG_HD bool jtk_ng_probe_on(const uint64_t* table, uint64_t mask, uint64_t slot, uint64_t seen, uint64_t k) {
    while (seen != k && seen != 0) {
        slot = (slot + 1) & mask;
        seen = table[slot];
    }
    return seen == k;
}
JTK_NG_HD bool jtk_ng_lookup(const uint64_t* table, uint64_t mask, uint64_t k) {
    const uint64_t slot = k & mask;
    return jtk_ng_probe_on(table, mask, slot, table[slot], k);
}
// cas(p, k): *p = k where *p == 0, and what *p held before (atomic on the device).  1 when k was not in the set.  The table
// holds an empty slot throughout: capacity >= 2 (keys + what is being inserted).
template <class Cas>
JTK_NG_HD int jtk_ng_insert(uint64_t* table, uint64_t mask, uint64_t k, Cas cas) {
    for (uint64_t slot = k & mask;; slot = (slot + 1) & mask) {
        const uint64_t old = cas(table + slot, k);
        if (old == 0) return 1;
        if (old == k) return 0;
    }
}

// ---- the walk
// k of the n-gram that starts at position i of document d (which holds i), or false when none starts there
JTK_NG_HD bool jtk_ng_starts(const JtkMhView& v, int64_t d, int64_t i) { return v.status[d] >= 0 && i + v.ngram <= v.tok_off[d + 1]; }
JTK_NG_HD bool jtk_ng_key_at(const JtkMhView& v, uint64_t key, int64_t i, uint64_t* k) {
    const int64_t d = jtk_mh_doc_of(v, 0, i);
    if (!jtk_ng_starts(v, d, i)) return false;
    *k = jtk_ng_finish(jtk_ng_hash(v.tokens + i, v.ngram), key);
    return true;
}
// a lane's positions [i0, i0 + JTK_NG_LANE) below total (i0 < total): bit j of the result says an n-gram starts at i0 + j, and
// ks[j] is then its k
JTK_NG_HD uint32_t jtk_ng_lane_keys(const JtkMhView& v, uint64_t key, uint64_t gn1, int64_t i0, uint64_t* ks) {
    int64_t d = jtk_mh_doc_of(v, 0, i0);
    uint32_t have = 0;
    uint64_t h = 0;
    bool rolling = false;                                      // h is H of the n-gram at i - 1, of the same document
#pragma unroll
    for (int j = 0; j < JTK_NG_LANE; j++) {
        const int64_t i = i0 + j;
        if (i >= v.total) break;
        if (v.tok_off[d + 1] <= i) { d = jtk_mh_next_doc(v, d, i); rolling = false; }
        if (!jtk_ng_starts(v, d, i)) { rolling = false; continue; }
        h = rolling ? jtk_ng_roll(h, v.tokens[i - 1], v.tokens[i + v.ngram - 1], gn1) : jtk_ng_hash(v.tokens + i, v.ngram);
        rolling = true;
        ks[j] = jtk_ng_finish(h, key);
        have |= 1u << j;
    }
    return have;
}

// The window word of a lane: bit b says that position i0 - 31 + b is a start, b < 31 + JTK_NG_LANE.  mine = the lane's own start
// bits, before[k - 1] = those of lane - k (0 where there is no such lane in the tile), k = 1..4; halo bit q = position
// w0 - 32 + q of the tokens before the tile, lane = (i0 - w0) / 8.
JTK_NG_HD uint64_t jtk_ng_window(uint32_t mine, const uint32_t* before, uint32_t halo, int lane) {
    uint64_t w = ((uint64_t)mine << 31) | ((uint64_t)before[0] << 23) | ((uint64_t)before[1] << 15) | ((uint64_t)before[2] << 7) |
                 ((uint64_t)before[3] >> 1);
    if (lane < 4) w |= (uint64_t)(halo >> (8 * lane + 1));
    return w;
}
// the flag byte of the lane's token j
JTK_NG_HD uint32_t jtk_ng_flag(uint64_t w, int32_t ngram, int j) {
    const uint64_t reach = (1ull << ngram) - 1ull;                                      // the n positions up to this one (n <= 32)
    const uint32_t start = (uint32_t)(w >> (31 + j)) & 1u;
    return (start ? JTK_NG_START : 0) | (((w >> (32 + j - ngram)) & reach) ? JTK_NG_COVERED : 0);
}
// the per-document results of a lane's tokens: add(d, n_hit, n_covered, first_hit or -1) once per document that has tokens here
template <class Add>
JTK_NG_HD void jtk_ng_lane_docs(const JtkMhView& v, int64_t i0, uint64_t w, Add add) {
    int64_t d = jtk_mh_doc_of(v, 0, i0), first = -1;
    int32_t hit = 0, cov = 0;
#pragma unroll
    for (int j = 0; j < JTK_NG_LANE; j++) {
        const int64_t i = i0 + j;
        if (i >= v.total) break;
        if (v.tok_off[d + 1] <= i) {
            if (hit | cov) add(d, hit, cov, first);
            hit = cov = 0; first = -1;
            d = jtk_mh_next_doc(v, d, i);
        }
        const uint32_t f = jtk_ng_flag(w, v.ngram, j);
        if (f & JTK_NG_START) { if (!hit) first = i - v.tok_off[d]; hit++; }
        if (f & JTK_NG_COVERED) cov++;
    }
    if (hit | cov) add(d, hit, cov, first);
}

#endif  // JTK_NGRAM_RULES_H
