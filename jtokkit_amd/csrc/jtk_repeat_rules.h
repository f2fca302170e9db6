// jtk_repeat_rules.h -- repeated token n-grams inside a document (jtk_batch_ngram_repeats): the rule the device kernels
// (jtk_repeat.hip) and the CPU test shim tests/repeat_sim share.  The repetition filters of Gopher (Rae et al., "Scaling Language
// Models", table A1), which RedPajama-v2, Dolma and FineWeb / datatrove carry: for n = 2..4 the share of a document inside its
// most frequent n-gram, for n = 5..10 the share inside n-grams that occur more than once.  Integer only: every result is exact.
//
// The rule, all arithmetic modulo 2^64; G = JTK_MH_G, mix = the splitmix64 finaliser (jtk_fim_mix):
//   key         = mix(seed + G * (n + 97)), n = ngram in 1..32 (MinHash has n + 1, the n-gram set n + 33: no shared key family).
//   key_D       = mix(key + G * (D + 1)), D = doc_index_base + d for document d of the batch (doc_index_base as in
//               jtk_fim_params: a shard of a corpus gives what the whole corpus would).
//   n-grams     of a document of l tokens: the windows t[i .. i + n), 0 <= i <= l - n; none when l < n, none when status < 0
//               whatever tokens the encode left it (as in jtk_ngram_rules.h).
//   H           = H * G + (uint32)id + 1 over the n ids, from 0 (jtk_ng_hash);  k = mix(H ^ key_D), and G where that is 0.
//               Two n-grams of ONE document are the same when their k are equal: a 64-bit collision inside a document is part
//               of the rule.  N-grams of different documents are never compared.
//   first(i)    the smallest document-relative position whose n-gram has the k of the one at i; count(i) the number of such
//               positions.
//   per token   p, a byte: JTK_RP_START when an n-gram starts at p and is a repeat; JTK_RP_COVERED when a start-flagged i of the
//               same document has p - n < i <= p.  A repeat: first(p) < p (a later occurrence); with JTK_REPEAT_MARK_FIRST in
//               the flags: count(p) >= 2, so the first occurrence is marked too, as RedPajama-v2 counts it.  (datatrove's
//               variant skips ahead n tokens behind every repeat it finds: that is sequential in the document and not offered.)
//   per doc     n_repeat = the start flags, n_covered = the covered tokens, top_count = the largest count over the document's
//               n-grams (0 without any), top_first = the smallest first among the n-grams with that count (-1 without any).
//
// What the device may deviate in, and the bound: the kernels keep the n-grams of many documents in ONE table keyed by k alone,
// so two n-grams of different documents whose k coincide -- under different key_D: probability 2^-64 per pair -- would be
// conflated.  For a table holding m n-grams the expected number of such pairs is at most m^2 / 2^65 (2^-17 for a table of 2^24
// n-grams): the order of the false-hit rate the n-gram set accepts, and the table budget keeps m small.
//
// The table: `capacity` slots, a power of two, the smallest >= max(64, 2 m) for the m n-grams of a group of documents
// (jtk_ng_capacity(0, m)).  A slot: key (0 = empty), first (preset to all ones), count (preset to 0); home slot k & (capacity -
// 1), linear probing with wrap-around (jtk_ng_insert's walk, here returning the slot).  JTK_RP_SLOT_BYTES per slot.
// Groups: documents are independent, so a call walks the batch in groups of whole consecutive documents and reuses one table.
// A group starts at d0, takes d0, and takes further documents while the table of its n-grams stays within the byte budget
// (jtk_rp_group_end): a document larger than the budget is a group of its own.  No result depends on the grouping.
//
// How the kernels walk a group (and the shim with them): the partition of jtk_ngram_rules.h -- tiles of JTK_NG_TILE tokens at
// multiples of JTK_NG_TILE of the BATCH's token array, a lane 8 consecutive tokens -- restricted to the group's token range
// [lo, hi): a lane takes the positions of its 8 that lie in the range (jtk_rp_lane_keys).  Pass 1 inserts: runs of equal k
// among a lane's consecutive keys become one (min, +r) pair (jtk_rp_lane_runs).  Pass 2 probes, decides the start bits
// (jtk_rp_is_repeat), recomputes those of the n - 1 positions before the tile that lie in the range (the backward halo), and
// goes on with jtk_ng_window / jtk_ng_flag / jtk_ng_lane_docs; an n-gram at its own first position offers (count, position)
// to its document's top (jtk_rp_top_pack: the larger count, then the smaller position wins a 64-bit maximum).
#ifndef JTK_REPEAT_RULES_H
#define JTK_REPEAT_RULES_H

#include <stdint.h>

#include "jtk_ngram_rules.h"       // the hash, the roll, the walk, the window and flag algebra; through it jtk_minhash_rules.h

#define JTK_RP_HD JTK_NG_HD

#ifndef JTK_RP_START
#define JTK_RP_START 1             // (as in include/jtokkit_amd.h)
#define JTK_RP_COVERED 2
#define JTK_REPEAT_MARK_FIRST 1u
#endif
#define JTK_RP_MAX_NGRAM JTK_NG_MAX_NGRAM
#define JTK_RP_SLOT_BYTES 20       // key 8 + first 8 + count 4
#define JTK_RP_MIN_TABLE_BYTES (JTK_NG_MIN_CAPACITY * JTK_RP_SLOT_BYTES)
#define JTK_RP_MAX_DOC_TOKENS 0x7FFFFFFFll     // a document-relative position fits 31 bits (jtk_rp_top_pack)

static_assert(JTK_RP_START == JTK_NG_START && JTK_RP_COVERED == JTK_NG_COVERED, "the flag algebra of jtk_ngram_rules.h is reused");

JTK_RP_HD bool jtk_rp_params_ok(int32_t ngram, uint32_t flags) {
    return (flags & ~JTK_REPEAT_MARK_FIRST) == 0 && ngram >= 1 && ngram <= JTK_RP_MAX_NGRAM;
}
JTK_RP_HD uint64_t jtk_rp_key(uint64_t seed, int32_t ngram) { return jtk_fim_mix(seed + JTK_MH_G * ((uint64_t)ngram + 97ull)); }
JTK_RP_HD uint64_t jtk_rp_doc_key(uint64_t key, uint64_t doc_index_base, int64_t d) {
    return jtk_fim_mix(key + JTK_MH_G * (doc_index_base + (uint64_t)d + 1ull));
}
JTK_RP_HD int64_t jtk_rp_capacity(int64_t m) { return jtk_ng_capacity(0, m); }
JTK_RP_HD int64_t jtk_rp_table_bytes(int64_t m) { return jtk_rp_capacity(m) * JTK_RP_SLOT_BYTES; }

// ---- the groups (host side; the shim plans with the same function)
// The group that starts at document d0 < n_docs: one past its last document, and *m = its n-grams.
inline int64_t jtk_rp_group_end(const int64_t* tok_off, const int32_t* status, int64_t n_docs, int32_t ngram, int64_t d0, int64_t budget_bytes,
                                int64_t* m) {
    int64_t have = 0, d = d0;
    for (; d < n_docs; d++) {
        const int64_t md = status[d] >= 0 ? jtk_ng_n_ngrams(tok_off[d + 1] - tok_off[d], ngram) : 0;
        if (d > d0 && jtk_rp_table_bytes(have + md) > budget_bytes) break;
        have += md;
    }
    *m = have;
    return d;
}

// ---- the table
struct JtkRpTable {
    uint64_t* key;                 // [capacity], 0 = empty
    uint64_t* first;               // [capacity], preset to all ones: the smallest batch position with this k
    uint32_t* count;               // [capacity]
    uint64_t mask;                 // capacity - 1
};
// where the parts of a table of `capacity` slots lie in one allocation: key | count | first (one memset of 0, one of 0xFF)
JTK_RP_HD JtkRpTable jtk_rp_table_at(void* base, int64_t capacity) {
    JtkRpTable t;
    t.key = (uint64_t*)base;
    t.count = (uint32_t*)(t.key + capacity);
    t.first = (uint64_t*)(t.count + capacity);     // (capacity >= 64: 8-byte aligned)
    t.mask = (uint64_t)capacity - 1;
    return t;
}
// cas(p, k) as for jtk_ng_insert; the slot that holds k afterwards.  The table holds an empty slot throughout.
template <class Cas>
JTK_RP_HD uint64_t jtk_rp_claim(uint64_t* keys, uint64_t mask, uint64_t k, Cas cas) {
    for (uint64_t slot = k & mask;; slot = (slot + 1) & mask) {
        const uint64_t old = cas(keys + slot, k);
        if (old == 0 || old == k) return slot;
    }
}
// the slot of a k that pass 1 inserted; find_on: the rest of the walk when slot `slot` held `seen`
JTK_RP_HD uint64_t jtk_rp_find_on(const uint64_t* keys, uint64_t mask, uint64_t slot, uint64_t seen, uint64_t k) {
    while (seen != k && seen != 0) {
        slot = (slot + 1) & mask;
        seen = keys[slot];
    }
    return slot;
}
JTK_RP_HD uint64_t jtk_rp_find(const uint64_t* keys, uint64_t mask, uint64_t k) {
    return jtk_rp_find_on(keys, mask, k & mask, keys[k & mask], k);
}
JTK_RP_HD bool jtk_rp_is_repeat(uint32_t flags, int64_t i, uint64_t first, uint32_t count) {
    return (flags & JTK_REPEAT_MARK_FIRST) ? count >= 2u : first < (uint64_t)i;
}
// what an n-gram at its own first position `rel` (document-relative, < 2^31) with `count` occurrences offers to its document's
// top: the maximum over a document's offers has the largest count and, among those, the smallest position.  0 = no n-gram.
JTK_RP_HD uint64_t jtk_rp_top_pack(uint32_t count, int64_t rel) { return ((uint64_t)count << 32) | (uint64_t)(0xFFFFFFFFu - (uint32_t)rel); }
JTK_RP_HD int32_t jtk_rp_top_count(uint64_t packed) { return (int32_t)(packed >> 32); }
JTK_RP_HD int64_t jtk_rp_top_first(uint64_t packed) { return packed ? (int64_t)(0xFFFFFFFFu - (uint32_t)packed) : -1; }

// ---- the walk
// a lane's positions [i0, i0 + JTK_NG_LANE) inside [lo, hi) (hi <= v.total, the range holds whole documents): bit j of the result
// says an n-gram starts at i0 + j, and ks[j] is then its k under its document's key
JTK_RP_HD uint32_t jtk_rp_lane_keys(const JtkMhView& v, uint64_t key, uint64_t base, uint64_t gn1, int64_t i0, int64_t lo, int64_t hi, uint64_t* ks) {
    const int64_t from = i0 < lo ? lo : i0;
    if (from >= hi || from >= i0 + JTK_NG_LANE) return 0;
    int64_t d = jtk_mh_doc_of(v, 0, from);
    uint64_t kd = jtk_rp_doc_key(key, base, d);
    uint32_t have = 0;
    uint64_t h = 0;
    bool rolling = false;                                      // h is H of the n-gram at i - 1, of the same document
#pragma unroll
    for (int j = 0; j < JTK_NG_LANE; j++) {
        const int64_t i = i0 + j;
        if (i < from) continue;
        if (i >= hi) break;
        if (v.tok_off[d + 1] <= i) { d = jtk_mh_next_doc(v, d, i); kd = jtk_rp_doc_key(key, base, d); rolling = false; }
        if (!jtk_ng_starts(v, d, i)) { rolling = false; continue; }
        h = rolling ? jtk_ng_roll(h, v.tokens[i - 1], v.tokens[i + v.ngram - 1], gn1) : jtk_ng_hash(v.tokens + i, v.ngram);
        rolling = true;
        ks[j] = jtk_ng_finish(h, kd);
        have |= 1u << j;
    }
    return have;
}
// k of the n-gram that starts at position i (lo <= i < hi), or false when none starts there
JTK_RP_HD bool jtk_rp_key_at(const JtkMhView& v, uint64_t key, uint64_t base, int64_t i, uint64_t* k) {
    const int64_t d = jtk_mh_doc_of(v, 0, i);
    if (!jtk_ng_starts(v, d, i)) return false;
    *k = jtk_ng_finish(jtk_ng_hash(v.tokens + i, v.ngram), jtk_rp_doc_key(key, base, d));
    return true;
}
// pass 1 of a lane: put(k, position of the run's first n-gram, r) once per run of r equal k at consecutive positions
template <class Put>
JTK_RP_HD void jtk_rp_lane_runs(uint32_t have, const uint64_t* ks, int64_t i0, Put put) {
    uint64_t k = 0;                                            // the open run: its k, where it began, its length
    int64_t at = 0;
    uint32_t r = 0;
#pragma unroll
    for (int j = 0; j < JTK_NG_LANE; j++) {
        const bool here = (have >> j) & 1u;
        if (r && !(here && ks[j] == k)) { put(k, at, r); r = 0; }
        if (here) {
            if (!r) { k = ks[j]; at = i0 + j; }
            r++;
        }
    }
    if (r) put(k, at, r);
}
// the top offers of a lane: offer(d, packed) once per document that has an n-gram at its own first position here
template <class Offer>
JTK_RP_HD void jtk_rp_lane_top(const JtkMhView& v, int64_t i0, uint32_t have, const uint64_t* first, const uint32_t* count, Offer offer) {
    int64_t d = -1;
    uint64_t best = 0;
#pragma unroll
    for (int j = 0; j < JTK_NG_LANE; j++) {
        if (!((have >> j) & 1u)) continue;
        const int64_t i = i0 + j;
        if (d < 0 || v.tok_off[d + 1] <= i) {
            if (best) offer(d, best);
            best = 0;
            d = d < 0 ? jtk_mh_doc_of(v, 0, i) : jtk_mh_next_doc(v, d, i);
        }
        if (first[j] != (uint64_t)i) continue;
        const uint64_t mine = jtk_rp_top_pack(count[j], i - v.tok_off[d]);
        if (mine > best) best = mine;
    }
    if (best) offer(d, best);
}

#endif  // JTK_REPEAT_RULES_H
