// jtk_seen_rules.h -- exact duplicates across documents and batches (jtk_seen_set_*, jtk_batch_seen_mark): the rule the device
// kernels (jtk_seen.hip), the host code and the CPU test shim tests/seen_sim share.  CCNet's and Dolma's paragraph dedup, Dolma's
// document dedup, the "drop lines that occur N times in the crawl" step of RefinedWeb and FineWeb: a set that outlives batches maps
// the 64-bit key of a text unit -- a whole document, a paragraph or a line -- to the smallest global position at which the unit
// was ever added and to how often it was added.  Integer only: every result is exact.
//
// The rule, all arithmetic modulo 2^64; G = JTK_MH_G, mix = the splitmix64 finaliser (jtk_fim_mix):
//   parameters  of a set, fixed at creation: seed, unit = JTK_SEEN_LINE (0), JTK_SEEN_PARAGRAPH (1) or JTK_SEEN_DOCUMENT (2), flags =
//               JTK_SEEN_TRIM (2u, the bit of JTK_LINES_TRIM) or 0; anything else is refused.
//   units       LINE and PARAGRAPH are the units of jtk_lines_rules.h, under its ink, blank and newline definitions; a document
//               with status < 0 has none.  DOCUMENT is the same rule with a threshold that no newline count reaches (3: the carry
//               saturates at 2, so jtk_ln_breaks(s, 3) holds for JTK_LN_NOINK alone): one unit from the document's first ink byte
//               to its last ink byte + 1, none for a document that is empty, all blank or refused.
//   key         key = mix(seed + G * (unit + 193)) (MinHash has n + 1, the n-gram set n + 33, n-gram repeats n + 97, line repeats
//               unit + 161: a family of its own).  H = H * G + byte + 1 over the unit's bytes, from 0 (jtk_ln_step); k = mix(H ^
//               key), and G where that is 0.  No per-document salt: equal units of different documents have equal k, and a 64-bit
//               collision is part of the rule, as for the n-gram set.
//   position    pos = (D << 24) | u, D = doc_index_base + d < 2^40 for document d of the batch, u < 2^24 the unit's
//               document-relative index.  A batch that would break either bound is refused and the set stays as it was.
//   the set     for every k ever added: first = the smallest pos added with it, count = the number of units added with it (both
//               uint64).  Adding the same batch twice leaves first alone and doubles its share of count.  Entries of two sets
//               merge by (min, +): associative and commutative, so what a set holds does not depend on the order in which
//               batches or shards arrive.
//   marking     mode out of JTK_SEEN_ADD (1) and JTK_SEEN_QUERY (2), at least one.  With ADD all units of the batch are added
//               first.  With QUERY every unit then reads its k's entry: first and count, all ones and 0 when k is absent; flag
//               JTK_SEEN_DUP (1) when first < pos, JTK_SEEN_FREQUENT (2) when min_count > 0 and count >= min_count.
//   results     per unit, in document order then text order: begin, end (batch byte positions), first, count, flag.  Per
//               document: unit_off [n_docs + 1]; n_dup, dup_bytes, dup_chars over the DUP-flagged units; unit_bytes, unit_chars
//               over all units.  chars as in jtk_lines_rules.h.
//
// The table: three planes of `capacity` uint64 -- key (0 = empty), first (preset to all ones), count (preset to 0) --, 24 bytes per
// slot and, at a load of at most 1/2, 48 bytes per key.  Home slot k & (capacity - 1), linear probing with wrap-around
// (jtk_rp_claim's walk; jtk_seen_claim also says whether the slot was empty, which is what counts the keys).  Before m units are
// added to a set of c keys the capacity becomes the smallest power of two >= max(64, 2 (c + m)) when that is larger
// (jtk_ng_capacity); it never shrinks.  Where a key lands depends on the order of arrival; keys, first, count and capacity do not.
#ifndef JTK_SEEN_RULES_H
#define JTK_SEEN_RULES_H

#include <stdint.h>

#include "jtk_lines_rules.h"

#define JTK_SN_HD JTK_LN_HD

#ifndef JTK_SEEN_LINE
#define JTK_SEEN_LINE 0            // (as in include/jtokkit_amd.h)
#define JTK_SEEN_PARAGRAPH 1
#define JTK_SEEN_DOCUMENT 2
#define JTK_SEEN_TRIM 2u
#define JTK_SEEN_ADD 1u
#define JTK_SEEN_QUERY 2u
#define JTK_SEEN_NO_COMBINE 4u
#define JTK_SEEN_DUP 1
#define JTK_SEEN_FREQUENT 2
#endif
static_assert(JTK_SEEN_LINE == JTK_LINES_LINE && JTK_SEEN_PARAGRAPH == JTK_LINES_PARAGRAPH && JTK_SEEN_TRIM == JTK_LINES_TRIM,
              "the walk of jtk_lines_rules.h takes unit and flags as they are");

#define JTK_SN_KEY_C 193
#define JTK_SN_UNIT_BITS 24
#define JTK_SN_MAX_DOC_UNITS ((int64_t)1 << JTK_SN_UNIT_BITS)      // u < 2^24
#define JTK_SN_MAX_DOCS ((uint64_t)1 << 40)                        // D < 2^40
#define JTK_SN_SLOT_BYTES 24
#define JTK_SN_ABSENT (~0ull)

JTK_SN_HD bool jtk_sn_params_ok(int32_t unit, uint32_t flags) { return unit >= JTK_SEEN_LINE && unit <= JTK_SEEN_DOCUMENT && (flags & ~JTK_SEEN_TRIM) == 0; }
JTK_SN_HD bool jtk_sn_mode_ok(uint32_t mode) {
    return (mode & (JTK_SEEN_ADD | JTK_SEEN_QUERY)) != 0 && (mode & ~(JTK_SEEN_ADD | JTK_SEEN_QUERY | JTK_SEEN_NO_COMBINE)) == 0;
}
JTK_SN_HD uint64_t jtk_sn_key(uint64_t seed, int32_t unit) { return jtk_fim_mix(seed + JTK_MH_G * ((uint64_t)unit + (uint64_t)JTK_SN_KEY_C)); }
// the walk's threshold: newlines between two ink bytes from which on the second starts a unit
JTK_SN_HD uint32_t jtk_sn_threshold(int32_t unit) { return unit == JTK_SEEN_DOCUMENT ? 3u : jtk_ln_threshold(unit); }
// may the documents [doc_index_base, doc_index_base + n_docs) be packed into positions?
JTK_SN_HD bool jtk_sn_docs_ok(uint64_t doc_index_base, int64_t n_docs) {
    return n_docs >= 0 && doc_index_base < JTK_SN_MAX_DOCS && (uint64_t)n_docs <= JTK_SN_MAX_DOCS - doc_index_base;
}
JTK_SN_HD uint64_t jtk_sn_pos(uint64_t doc_index_base, int64_t d, int64_t u) { return ((doc_index_base + (uint64_t)d) << JTK_SN_UNIT_BITS) | (uint64_t)u; }
JTK_SN_HD int64_t jtk_sn_capacity(int64_t c, int64_t m) { return jtk_ng_capacity(c, m); }

// ---- the table
struct JtkSnTable {
    uint64_t *key, *first, *count;     // [capacity] each
    uint64_t mask;                     // capacity - 1
};
// where the planes of a table of `capacity` slots lie in one allocation: key | count | first (one memset of 0, one of 0xFF)
JTK_SN_HD JtkSnTable jtk_sn_table_at(void* base, int64_t capacity) {
    JtkSnTable t;
    t.key = (uint64_t*)base;
    t.count = t.key + capacity;
    t.first = t.count + capacity;
    t.mask = (uint64_t)capacity - 1;
    return t;
}
// jtk_rp_claim's walk; *fresh: the slot was empty and this call took it.  The table holds an empty slot throughout.
template <class Cas>
JTK_SN_HD uint64_t jtk_sn_claim(uint64_t* keys, uint64_t mask, uint64_t k, Cas cas, bool* fresh) {
    for (uint64_t slot = k & mask;; slot = (slot + 1) & mask) {
        const uint64_t old = cas(keys + slot, k);
        if (old == 0 || old == k) { *fresh = old == 0; return slot; }
    }
}
// the (min, +) merge of an entry into a slot, as the kernels do it with two atomics
JTK_SN_HD void jtk_sn_merge(uint64_t* first, uint64_t* count, uint64_t e_first, uint64_t e_count) {
    if (e_first < *first) *first = e_first;
    *count += e_count;
}
// what a unit at `pos` reads from its entry (first = JTK_SN_ABSENT and count = 0 when its k is absent)
JTK_SN_HD uint32_t jtk_sn_flag(uint64_t first, uint64_t count, uint64_t pos, uint64_t min_count) {
    return (first < pos ? (uint32_t)JTK_SEEN_DUP : 0u) | (min_count > 0 && count >= min_count ? (uint32_t)JTK_SEEN_FREQUENT : 0u);
}

#endif  // JTK_SEEN_RULES_H
