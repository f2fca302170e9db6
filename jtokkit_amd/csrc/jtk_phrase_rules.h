// jtk_phrase_rules.h -- phrase sets (jtk_phrase_set_*, jtk_batch_phrase_hits): the rule the device kernels (jtk_phrase.hip), the
// host table build (jtk_abi.cpp) and the CPU walk tests/phrase_sim share.  "Does this document, or this line, contain one of these
// strings": C4's bad-words list, `lorem ipsum`, `{` and its line rules (`javascript`, the policy phrases), the blocklists of
// RefinedWeb, FineWeb and Dolma, a user's own boilerplate and canary strings.  A pass over the TEXT of the last encode.  Exact.
//
// The rule:
//   set         n phrases, 0 <= n <= JTK_PH_MAX_PHRASES.  Phrase i is bytes[off[i], off[i + 1]), 1 .. JTK_PH_MAX_LEN bytes; group[i]
//               is in 0..31 (a NULL group array: all 0); the bytes of all phrases are at most JTK_PH_MAX_BYTES.  flags out of
//               JTK_PHRASE_FOLD_ASCII and JTK_PHRASE_WORD_BOUNDS.  Anything else is refused and no set is made.  With FOLD_ASCII
//               'A'..'Z' of the phrases are folded to 'a'..'z' when the set is made and 'A'..'Z' of the text when it is matched; no
//               other byte changes.  Equal phrases (after folding) are ONE phrase: its group mask is the OR of 1 << group over them,
//               its index the smallest of theirs.  n == 0 is a valid set: every output is 0 and first_* is -1.
//   hit         a pair (p, phrase) in document d = x[a, e), a = doc_off[d], e = doc_off[d + 1], is a hit when a <= p and
//               p + len <= e (nothing crosses a document edge), the folded text bytes x[p, p + len) equal the phrase, and, with
//               WORD_BOUNDS, both edges are boundaries: p == a or the character that ENDS at p - 1 is no word character; p + len == e
//               or the character that STARTS at p + len is no word character.  A word character is '_' or a code point whose class
//               in the library's Unicode tables is L or N (jtk_wd_class_of).  The character that ends at p - 1 is found by stepping
//               back over at most three continuation bytes without leaving the document.  The rule is defined for well-formed
//               UTF-8; on ill-formed bytes the result is some value and no access leaves the text.  This is Python's
//               (?:\W|^)phrase(?:\W|$) with re.UNICODE up to the Unicode version of the tables and the categories Python's \w adds
//               beyond L, N and '_'; no more is claimed.  A document with status < 0 has no hits.
//   document    group_mask = the OR of the hits' group masks; n_hits = the number of hits, one per pair of p and distinct phrase,
//               saturated at 2^31 - 1; first_hit = the smallest p - a, -1 without a hit; first_which = the smallest phrase index
//               among the hits at that p, -1 without; n_hit_units = the units with a mask that is not 0.
//   unit        of the list jtk_batch_line_units holds: unit_mask = the OR over the hits with begin <= p and p + len <= end.  A hit
//               that straddles a unit's edge belongs to no unit.
//
// The tables (built once by jtk_ph_build on the host, immutable on the device).  Failureless Aho-Corasick: a trie without failure
// links; every start byte walks it on its own.
//   first2      a bitmap of 65,536 bits: bit (b0 << 8 | b1) is set when a phrase of 2 or more bytes begins with b0 b1.
//   first1      a bitmap of 256 bits: the 1-byte phrases.  A start byte whose two tests fail walks nothing.
//   edges       open addressing, n_slots >= 2 * edges (load <= 1/2), any size (the home slot is a multiply-shift reduction, not a
//               mask): a slot is 8 bytes, key = state << 8 | byte (states < 2^24; JTK_PH_EMPTY: no key), value = the next state |
//               JTK_PH_V_TERMINAL when a phrase ends there | JTK_PH_V_CHILDREN when it has edges of its own -- the walk needs no
//               second read to know whether to report and whether to go on.  State 0 is the root.
//   info        16 bytes per state, read at terminal states only: terminal, group mask, smallest phrase index, depth.
#ifndef JTK_PHRASE_RULES_H
#define JTK_PHRASE_RULES_H

#include <stdint.h>

#include "jtk_common.h"
#include "jtk_words_rules.h"

#ifndef JTK_PHRASE_FOLD_ASCII
#define JTK_PHRASE_FOLD_ASCII 1u   // (as in include/jtokkit_amd.h)
#define JTK_PHRASE_WORD_BOUNDS 2u
#endif
#define JTK_PH_MAX_PHRASES 65536
#define JTK_PH_MAX_LEN 64
#define JTK_PH_MAX_BYTES (1 << 20)

// how jtk_phrase.hip cuts the text: a lane's granule of start positions, a workgroup's tile, the bytes staged before and behind it
#define JTK_PH_GRANULE 16
#define JTK_PH_TILE 4096
#define JTK_PH_LEAD 16             // bytes before the tile (the character that ends before its first byte; a whole 16-byte load)
#define JTK_PH_TAIL 80             // bytes behind it: 63 of a phrase that starts on its last byte, 4 of the character behind that
#define JTK_PH_WINDOW (JTK_PH_LEAD + JTK_PH_TILE + JTK_PH_TAIL)
#define JTK_PH_LDS_SLOTS 5120      // an edge table of up to this many slots is staged in LDS (40 KB); a larger one is probed in L2
static_assert(JTK_PH_TAIL >= JTK_PH_MAX_LEN - 1 + 4 && JTK_PH_TAIL % 16 == 0 && JTK_PH_LEAD >= 4, "the walk and both boundary characters stay inside the window");

#define JTK_PH_EMPTY 0xFFFFFFFFu
#define JTK_PH_V_TERMINAL 0x80000000u
#define JTK_PH_V_CHILDREN 0x40000000u
#define JTK_PH_V_STATE 0x00FFFFFFu
#define JTK_PH_NO_HIT 0xFFFFFFFFFFFFFFFFull

struct JtkPhEdge { uint32_t key, value; };
struct JtkPhInfo { uint32_t terminal, group_mask, index, depth; };

JTK_HD uint32_t jtk_ph_fold_byte(uint32_t b) { return (b - 'A') < 26u ? b | 0x20u : b; }
JTK_HD uint32_t jtk_ph_fold32(uint32_t x) {                     // 'A'..'Z' -> 'a'..'z' in every byte
    const uint32_t y = x & 0x7F7F7F7Fu;
    const uint32_t up = (y + 0x3F3F3F3Fu) & ~(y + 0x25252525u) & ~x & 0x80808080u;
    return x | (up >> 2);
}

// the probe: the home slot of a key, then linear with wrap-around until the key or an empty slot (there is one: load <= 1/2)
JTK_HD uint32_t jtk_ph_home(uint32_t key, uint32_t n_slots) { return (uint32_t)(((uint64_t)(key * 0x9E3779B1u) * n_slots) >> 32); }
JTK_HD uint32_t jtk_ph_find(const JtkPhEdge* edges, uint32_t n_slots, uint32_t state, uint32_t byte) {      // the value; 0: no edge
    const uint32_t key = (state << 8) | byte;
    uint32_t s = jtk_ph_home(key, n_slots);
    for (uint32_t k = 0; k < n_slots; k++) {
        const JtkPhEdge e = edges[s];
        if (e.key == key) return e.value;
        if (e.key == JTK_PH_EMPTY) return 0u;
        s = s + 1u == n_slots ? 0u : s + 1u;
    }
    return 0u;
}
JTK_HD bool jtk_ph_bit(const uint32_t* bits, uint32_t i) { return (bits[i >> 5] >> (i & 31u)) & 1u; }
// does a walk start at a byte b0 followed by b1 (0 behind the text: the walk itself stops at the document's end)
JTK_HD bool jtk_ph_candidate(const uint32_t* first2, const uint32_t* first1, uint32_t b0, uint32_t b1) {
    return jtk_ph_bit(first2, (b0 << 8) | b1) || jtk_ph_bit(first1, b0);
}

// ---- the boundary.  T: x[i] is the (folded) byte at batch position i, 0 behind the text; only positions in [a - 0, e + 3] of a
// document x[a, e) are read
template <class T>
JTK_HD uint32_t jtk_ph_cp_at(const T& x, int64_t i) {           // the code point whose lead byte is at i; 0xFFFFFFFF: none starts here
    const uint32_t b0 = x[i];
    if (b0 < 0x80u) return b0;
    if (b0 < 0xC0u) return 0xFFFFFFFFu;
    const uint32_t b1 = x[i + 1] & 0x3Fu;
    if (b0 < 0xE0u) return ((b0 & 0x1Fu) << 6) | b1;
    const uint32_t b2 = x[i + 2] & 0x3Fu;
    if (b0 < 0xF0u) return ((b0 & 0x0Fu) << 12) | (b1 << 6) | b2;
    return ((b0 & 0x07u) << 18) | (b1 << 12) | (b2 << 6) | (x[i + 3] & 0x3Fu);
}
JTK_HD bool jtk_ph_word_cp(const JtkUcTables& uc, uint32_t cp) {
    if (cp == 0x5Fu) return true;
    if (cp == 0xFFFFFFFFu) return false;
    const uint32_t c = jtk_wd_class_of(uc, cp);
    return c == JTK_CLS_L || c == JTK_CLS_N;
}
template <class T>
JTK_HD bool jtk_ph_bounded(const T& x, const JtkUcTables& uc, int64_t a, int64_t e, int64_t p, int64_t len) {
    if (p > a) {
        int64_t j = p - 1;
        for (int k = 0; k < 3 && j > a && (x[j] & 0xC0u) == 0x80u; k++) j--;
        if (jtk_ph_word_cp(uc, jtk_ph_cp_at(x, j))) return false;
    }
    return p + len >= e || !jtk_ph_word_cp(uc, jtk_ph_cp_at(x, p + len));
}

// ---- the walk from one start position p of document x[a, e): report(len, value) at every terminal state (before the boundary
// test, which the caller makes).  F: value = find(state, byte)
template <class T, class F, class R>
JTK_HD void jtk_ph_walk(const T& x, int64_t e, int64_t p, const F& find, R&& report) {
    const int64_t room = e - p;
    const int lim = room < JTK_PH_MAX_LEN ? (int)room : JTK_PH_MAX_LEN;
    uint32_t state = 0;
    for (int k = 0; k < lim; k++) {
        const uint32_t v = find(state, x[p + k]);
        if (!v) return;
        if (v & JTK_PH_V_TERMINAL) report(k + 1, v);
        if (!(v & JTK_PH_V_CHILDREN)) return;
        state = v & JTK_PH_V_STATE;
    }
}

// the packed first hit of a document: (p - a) << 16 | phrase index, smaller is earlier
JTK_HD uint64_t jtk_ph_first_key(int64_t rel, uint32_t index) { return ((uint64_t)rel << 16) | index; }

// ---- the host build (jtk_abi.cpp and tests/phrase_sim define JTK_PHRASE_HOST_BUILD before the include)
#ifdef JTK_PHRASE_HOST_BUILD
#include <unordered_map>
#include <vector>

struct JtkPhHostSet {
    uint32_t flags = 0, n_slots = 0, n_distinct = 0, has1 = 0;
    std::vector<uint32_t> first2, first1;
    std::vector<JtkPhEdge> edges;
    std::vector<JtkPhInfo> info;   // [states]
};

// 0, or what is wrong with the arguments
inline const char* jtk_ph_build(const uint8_t* bytes, const uint32_t* off, const uint8_t* group, int64_t n, uint32_t flags, JtkPhHostSet* out) {
    if (flags & ~(JTK_PHRASE_FOLD_ASCII | JTK_PHRASE_WORD_BOUNDS)) return "phrase set: flags out of JTK_PHRASE_FOLD_ASCII | JTK_PHRASE_WORD_BOUNDS";
    if (n < 0 || n > JTK_PH_MAX_PHRASES) return "phrase set: 0 .. 65536 phrases";
    if (n > 0 && (!bytes || !off)) return "phrase set: bytes or off is NULL";
    for (int64_t i = 0; i < n; i++) {
        if (off[i + 1] <= off[i] || off[i + 1] - off[i] > JTK_PH_MAX_LEN) return "phrase set: a phrase has 1 to 64 bytes";
        if (off[i + 1] - off[0] > JTK_PH_MAX_BYTES) return "phrase set: the phrases have at most 1 MiB of bytes";
        if (group && group[i] > 31) return "phrase set: a group is in 0 .. 31";
    }
    JtkPhHostSet s;
    s.flags = flags;
    s.first2.assign(65536 / 32, 0);
    s.first1.assign(256 / 32, 0);
    s.info.push_back(JtkPhInfo{0, 0, JTK_PH_EMPTY, 0});
    std::unordered_map<uint32_t, uint32_t> next;                 // state << 8 | byte -> state
    std::vector<uint8_t> children(1, 0);
    for (int64_t i = 0; i < n; i++) {
        const uint32_t len = off[i + 1] - off[i];
        uint32_t state = 0, b01 = 0;
        for (uint32_t k = 0; k < len; k++) {
            uint32_t b = bytes[off[i] + k];
            if (flags & JTK_PHRASE_FOLD_ASCII) b = jtk_ph_fold_byte(b);
            if (k < 2) b01 = (b01 << 8) | b;
            const auto at = next.emplace((state << 8) | b, (uint32_t)s.info.size());
            if (at.second) {
                children[state] = 1;
                s.info.push_back(JtkPhInfo{0, 0, JTK_PH_EMPTY, k + 1});
                children.push_back(0);
            }
            state = at.first->second;
        }
        if (len == 1) { s.first1[b01 >> 5] |= 1u << (b01 & 31u); s.has1 = 1; }
        else s.first2[b01 >> 5] |= 1u << (b01 & 31u);
        JtkPhInfo& t = s.info[state];
        if (!t.terminal) { t.terminal = 1; t.index = (uint32_t)i; s.n_distinct++; }   // (i ascends: the first is the smallest)
        t.group_mask |= 1u << (group ? group[i] : 0);
    }
    s.n_slots = next.size() < 8 ? 16u : (uint32_t)(2 * next.size());
    s.edges.assign(s.n_slots, JtkPhEdge{JTK_PH_EMPTY, 0});
    for (const auto& kv : next) {
        uint32_t at = jtk_ph_home(kv.first, s.n_slots);
        while (s.edges[at].key != JTK_PH_EMPTY) at = at + 1u == s.n_slots ? 0u : at + 1u;
        s.edges[at] = JtkPhEdge{kv.first, kv.second | (s.info[kv.second].terminal ? JTK_PH_V_TERMINAL : 0u) | (children[kv.second] ? JTK_PH_V_CHILDREN : 0u)};
    }
    *out = std::move(s);
    return nullptr;
}
#endif  // JTK_PHRASE_HOST_BUILD

#endif  // JTK_PHRASE_RULES_H
