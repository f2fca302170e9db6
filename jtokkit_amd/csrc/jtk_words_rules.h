// jtk_words_rules.h -- word-level quality signals of a document (jtk_batch_word_stats): the rule the device kernels
// (jtk_words.hip) and the CPU walk tests/words_sim share.  The quality half of Gopher's filter (Rae et al., "Scaling Language
// Models", table A1) as datatrove's GopherQualityFilter, RedPajama-v2's rps_doc_* signals, Dolma's Gopher tagger and FineWeb's
// line rules compute it: word count and mean word length, the symbol-to-word ratios of '#' and ellipses, the share of words with a
// letter, the stop-word test, and the shares of lines that start with a bullet or end with an ellipsis.  A pass over the TEXT of
// the last encode.  Integer only: every count is exact.
//
// The rule:
//   text        document d of the batch is the bytes x[a, e), a = doc_off[d], e = doc_off[d + 1].  Nothing crosses a document
//               edge.  A document with status < 0 gets 0 in every output.  The rule is defined for well-formed UTF-8; on
//               ill-formed bytes every count is some value and no access leaves the text.
//   characters  a character is a byte b with (b & 0xC0) != 0x80 (the weight of JTK_UNIT_CODEPOINT, jtk_charpos_rules.h).  Its
//               class is jtk_class_of_cp of its code point: L, N, W (White_Space) or O; a continuation byte belongs to the
//               nearest character before it.  A byte >= 0x80 that starts no well-formed sequence is class O.
//   words       a word is a maximal run of characters that are not W: Python's str.split() with White_Space as the separator
//               set.  It is ALPHA when it holds at least one L character, SYMBOL-ONLY when it holds neither L nor N.
//   counts      n_words; word_chars = the characters of all words; n_alpha_words; n_symbol_words; symbol_word_chars = the
//               characters of the symbol-only words.  datatrove's mean word length is (word_chars - symbol_word_chars) /
//               (n_words - n_symbol_words), Gopher's alpha fraction n_alpha_words / n_words.
//   symbols     n_hash = the bytes 0x23.  n_ellipsis = the sum over the maximal runs of 0x2E of floor(run length / 3), plus the
//               occurrences of U+2026: Python's text.count("...") + text.count("…").
//   stop words  up to JTK_WD_MAX_STOP words of 1 .. JTK_WD_MAX_STOP_LEN bytes, each well-formed UTF-8 without a White_Space
//               character (anything else is refused).  A word of the text IS stop word i when its bytes equal it exactly; with
//               JTK_WORDS_FOLD_ASCII the bytes 'A'..'Z' of the TEXT are folded to 'a'..'z' before the comparison (the list is taken
//               as it is).  stop_mask has bit i set when stop word i occurs in the document; n_stop_hits counts the words of the
//               text that are some stop word, each once, however often the list repeats it.  "the," , "bathe" and "then" are not
//               "the": a tokenizer that splits punctuation off a word (datatrove's word tokenizers, NLTK) finds "the" in "the,"
//               and this rule does not.
//   lines       over the units of jtk_batch_line_units(unit = JTK_LINES_LINE, JTK_LINES_TRIM) on the same encode -- exactly the
//               trimmed non-blank lines: n_lines; n_bullet_lines, the unit begins with U+2022 or '-'; n_ellipsis_lines, it ends
//               with "..." or U+2026; n_terminal_lines, its last byte is one of . ! ? " ; n_short_lines, it has fewer than
//               short_line_chars characters (short_line_chars <= 0: the output is written as 0).
//
// How the kernels walk the text (and the walk of tests/words_sim with them).  The text is cut into granules of JTK_WD_GRANULE =
// 16 bytes at multiples of 16 of the batch (one lane each), JTK_WD_WAVE_BYTES = 1024 (a wave) and tiles of JTK_WD_TILE = 4096 (a
// workgroup); pass B scans JTK_WD_SCAN_STEP tiles at a step.  The EDGE and REF planes are those of jtk_lines_rules.h.  A granule
// is classified ONCE into bit masks (bit i = byte i): live, lead, nw (byte of a word), L, LN, hash, dot, u2026 -- jtk_wd_classify,
// which looks at most 4 bytes back and 4 bytes ahead of the granule to finish the characters that straddle its ends.  The rest
// is mask algebra:
//   events      a word starts at a byte of nw whose predecessor is not (or at an edge), and ends symmetrically.
//   carries     "the word has an L-or-N so far" (forward), "it will have one" and "it will have an L" (backward) are three-state
//               transforms of a granule: SET, RESET (a W or an edge behind the last L / N), ID.  Inside the granule they are a
//               segmented fill (jtk_wd_fill_up / _down: four shift-and-or steps); across lanes the carry into a lane is the
//               transform of the nearest lane that is not ID: two ballots and a bit scan (jtk_wd_carry_before / _behind).
//   dots        the carry is the length modulo 3 of the dot run that ends at the granule's last byte: a transform "fix r" or,
//               for a granule of 16 linked dots, "add 1" (JTK_WD_DOT_*).  Inside, the carry is shifted in as c virtual dots and
//               the triples are marked by a chain of six shift-and-and steps (jtk_wd_ellipses).
//   stop words  decided at a word's END from the 8 bytes before it: the granule and the upper half of the one before it.  The
//               word's length comes from the start bits of the granule, or from `trail`, the number of word bytes at the end of the
//               granule before (jtk_wd_trail); a word longer than 8 bytes is no stop word, so no lane looks further.
// Pass A writes a tile's summary word (the four transforms and the trail of its last granule), pass B scans them, pass C repeats
// pass A's work with the carries and adds the events to their documents.  No workgroup waits for another.
#ifndef JTK_WORDS_RULES_H
#define JTK_WORDS_RULES_H

#include <stdint.h>

#include "jtk_common.h"

#ifndef JTK_WORDS_FOLD_ASCII
#define JTK_WORDS_FOLD_ASCII 1u    // (as in include/jtokkit_amd.h)
#endif
#define JTK_WD_MAX_STOP 32
#define JTK_WD_MAX_STOP_LEN 8

#define JTK_WD_GRANULE 16
#define JTK_WD_WAVE_BYTES (64 * JTK_WD_GRANULE)
#define JTK_WD_TILE (4 * JTK_WD_WAVE_BYTES)
#define JTK_WD_TILE_GRANULES (JTK_WD_TILE / JTK_WD_GRANULE)
#define JTK_WD_SCAN_STEP 1024      // tiles per step of pass B

// a three-state transform
#define JTK_WD_T_ID 0u
#define JTK_WD_T_RESET 1u
#define JTK_WD_T_SET 2u
// a dot transform: bit 2 = it fixes the run length modulo 3 to bits 0-1; else bits 0-1 are added to it
#define JTK_WD_DOT_FIX 4u

JTK_HD uint32_t jtk_wd_then(uint32_t a, uint32_t b) { return b != JTK_WD_T_ID ? b : a; }               // a, then b
JTK_HD uint32_t jtk_wd_apply(uint32_t t, uint32_t s) { return t == JTK_WD_T_ID ? s : (t == JTK_WD_T_SET ? 1u : 0u); }
JTK_HD uint32_t jtk_wd_dot_then(uint32_t a, uint32_t b) {
    if (b & JTK_WD_DOT_FIX) return b;
    return (a & JTK_WD_DOT_FIX) | (((a & 3u) + (b & 3u)) % 3u);
}
JTK_HD uint32_t jtk_wd_dot_apply(uint32_t t, uint32_t c) { return (t & JTK_WD_DOT_FIX) ? (t & 3u) : (c + (t & 3u)) % 3u; }

// Across the 64 lanes of a wave (or 64 tiles of pass B): `non` has the lanes whose transform is not ID, `set` those that SET.
// The state before lane l is decided by the nearest lane below it that is not ID, behind it by the nearest above; cin: the state
// before (behind) the wave.  And the wave's own transform, forward and backward.
JTK_HD uint32_t jtk_wd_carry_before(uint64_t set, uint64_t non, int lane, uint32_t cin) {
    const uint64_t below = non & ((1ull << lane) - 1ull);
    return below ? (uint32_t)((set >> (63 - jtk_clz64(below))) & 1ull) : cin;
}
JTK_HD uint32_t jtk_wd_carry_behind(uint64_t set, uint64_t non, int lane, uint32_t cin) {
    const uint64_t above = lane >= 63 ? 0ull : non & ~((2ull << lane) - 1ull);
    return above ? (uint32_t)((set >> jtk_ctz64(above)) & 1ull) : cin;
}
JTK_HD uint32_t jtk_wd_wave_fwd(uint64_t set, uint64_t non) {
    return non ? (((set >> (63 - jtk_clz64(non))) & 1ull) ? JTK_WD_T_SET : JTK_WD_T_RESET) : JTK_WD_T_ID;
}
JTK_HD uint32_t jtk_wd_wave_bwd(uint64_t set, uint64_t non) {
    return non ? (((set >> jtk_ctz64(non)) & 1ull) ? JTK_WD_T_SET : JTK_WD_T_RESET) : JTK_WD_T_ID;
}
// dots: `fix` has the lanes whose transform fixes, r_at_fix is the value of the nearest such lane below lane l (the caller fetches
// it: one shuffle); every lane that does not fix adds 1 (16, 1024 and 4096 are all 1 modulo 3)
static_assert(JTK_WD_GRANULE % 3 == 1 && JTK_WD_WAVE_BYTES % 3 == 1 && JTK_WD_TILE % 3 == 1, "a span of linked dots adds 1");
JTK_HD int jtk_wd_dot_src(uint64_t fix, int lane) {             // the lane to fetch from; -1: none below
    const uint64_t below = fix & ((1ull << lane) - 1ull);
    return below ? 63 - jtk_clz64(below) : -1;
}
JTK_HD uint32_t jtk_wd_dot_before(int src, uint32_t r_at_src, int lane, uint32_t cin) {
    return src >= 0 ? (r_at_src + (uint32_t)(lane - 1 - src)) % 3u : (cin + (uint32_t)lane) % 3u;
}
JTK_HD uint32_t jtk_wd_dot_wave(uint64_t fix, uint32_t r_at_last_fix) {          // r_at_last_fix: of the highest lane that fixes
    return fix ? JTK_WD_DOT_FIX | ((r_at_last_fix + (uint32_t)jtk_clz64(fix)) % 3u) : (64u % 3u);
}

// a tile's summary word: fwd LN | bwd LN << 2 | bwd L << 4 | dot << 6 | trail << 9; its carry word: the three states in bits 0-2
// (fwd LN, bwd LN, bwd L), the dot carry in bits 3-4
JTK_HD uint32_t jtk_wd_tile_word(uint32_t f_ln, uint32_t b_ln, uint32_t b_l, uint32_t dot, uint32_t trail) {
    return f_ln | (b_ln << 2) | (b_l << 4) | (dot << 6) | (trail << 9);
}
JTK_HD uint32_t jtk_wd_word_trail(uint32_t w) { return (w >> 9) & 31u; }

// ---- fills over the 16 bits of a granule.  up: g(i) |= g(i - 1) unless `blocked` has bit i; down: g(i) |= g(i + 1) likewise
JTK_HD uint32_t jtk_wd_fill_up(uint32_t g, uint32_t blocked) {
    uint32_t p = ~blocked;
    g |= p & (g << 1); p &= p << 1;
    g |= p & (g << 2); p &= p << 2;
    g |= p & (g << 4); p &= p << 4;
    g |= p & (g << 8);
    return g & 0xFFFFu;
}
JTK_HD uint32_t jtk_wd_fill_down(uint32_t g, uint32_t blocked) {
    uint32_t p = ~blocked & 0xFFFFu;
    g &= 0xFFFFu;
    g |= p & (g >> 1); p &= p >> 1;
    g |= p & (g >> 2); p &= p >> 2;
    g |= p & (g >> 4); p &= p >> 4;
    g |= p & (g >> 8);
    return g;
}
// the bits below the lowest bit of m, above its highest; all 16 when m is 0
JTK_HD uint32_t jtk_wd_below_first(uint32_t m) { return m ? ((m & (0u - m)) - 1u) & 0xFFFFu : 0xFFFFu; }
JTK_HD uint32_t jtk_wd_above_last(uint32_t m) { return m ? 0xFFFFu & ~((2u << (31 - __builtin_clz(m))) - 1u) : 0xFFFFu; }

// the bytes of a granule inside a refused document (what jtk_ln_refused_mask computes by a loop): the edges that start a refused
// document, filled up to the next edge; r_in: is the byte before the granule refused
JTK_HD uint32_t jtk_wd_refused_mask(uint32_t edge, uint32_t ref, uint32_t r_in) {
    return jtk_wd_fill_up(edge & ref, edge) | (r_in ? jtk_wd_below_first(edge) : 0u);
}

// ---- a granule
struct JtkWdGran {
    uint32_t live, lead, nw, L, LN, hash, dot, u2026;
    uint32_t next_nw;              // is the byte behind the granule, by its class alone, a byte of a word
};

JTK_HD uint32_t jtk_wd_byte(const uint32_t* w6, int k) { return (w6[(k + 4) >> 2] >> (8 * ((k + 4) & 3))) & 0xFFu; }   // k in -4 .. 19
// the code point of the character whose lead is byte k (-4 <= k <= 16); 0xFFFFFFFF for a byte that starts none
JTK_HD uint32_t jtk_wd_cp_at(const uint32_t* w6, int k) {
    const uint32_t b0 = jtk_wd_byte(w6, k);
    if (b0 < 0x80u) return b0;
    if (b0 < 0xC0u || k > 16) return 0xFFFFFFFFu;
    const uint32_t b1 = jtk_wd_byte(w6, k + 1) & 0x3Fu;
    if (b0 < 0xE0u) return ((b0 & 0x1Fu) << 6) | b1;
    const uint32_t b2 = jtk_wd_byte(w6, k + 2) & 0x3Fu;
    if (b0 < 0xF0u) return ((b0 & 0x0Fu) << 12) | (b1 << 6) | b2;
    return ((b0 & 0x07u) << 18) | (b1 << 12) | (b2 << 6) | (jtk_wd_byte(w6, k + 3) & 0x3Fu);
}
JTK_HD uint32_t jtk_wd_class_of(const JtkUcTables& uc, uint32_t cp) { return cp < 0x80u ? jtk_class_of_ascii(cp) : jtk_class_of_cp(uc, cp); }

// w6: the 4 bytes before the granule, its 16 bytes, the 4 bytes behind it (0 where the text has none); valid: its bytes inside
// the text; refused: jtk_wd_refused_mask
JTK_HD JtkWdGran jtk_wd_classify(const JtkUcTables& uc, const uint32_t* w6, int valid, uint32_t refused) {
    JtkWdGran g{0, 0, 0, 0, 0, 0, 0, 0, 0};
    uint32_t cur = JTK_CLS_O, w = 0;
    if ((jtk_wd_byte(w6, 0) & 0xC0u) == 0x80u) {                 // the character that reaches into the granule
        uint32_t cp = jtk_wd_cp_at(w6, -1);                      // (every index a constant: the window stays in registers)
        if ((jtk_wd_byte(w6, -1) & 0xC0u) == 0x80u) cp = (jtk_wd_byte(w6, -2) & 0xC0u) == 0x80u ? jtk_wd_cp_at(w6, -3) : jtk_wd_cp_at(w6, -2);
        cur = jtk_wd_class_of(uc, cp);
    }
#pragma unroll
    for (int i = 0; i < JTK_WD_GRANULE; i++) {
        const uint32_t b = jtk_wd_byte(w6, i), bit = 1u << i;
        if ((b & 0xC0u) != 0x80u) {
            g.lead |= bit;
            if (b < 0x80u) {
                cur = jtk_class_of_ascii(b);
                if (b == 0x23u) g.hash |= bit;
                if (b == 0x2Eu) g.dot |= bit;
            } else {
                const uint32_t cp = jtk_wd_cp_at(w6, i);
                cur = jtk_wd_class_of(uc, cp);
                if (cp == 0x2026u) g.u2026 |= bit;
            }
            if (cur == JTK_CLS_L) g.L |= bit;
            if (cur == JTK_CLS_L || cur == JTK_CLS_N) g.LN |= bit;
        }
        if (cur == JTK_CLS_W) w |= bit;
    }
    const uint32_t nb = jtk_wd_byte(w6, 16);
    if ((nb & 0xC0u) != 0x80u) cur = jtk_wd_class_of(uc, jtk_wd_cp_at(w6, 16));
    g.next_nw = cur != JTK_CLS_W ? 1u : 0u;
    g.live = ((1u << valid) - 1u) & ~refused;
    g.nw = ~w & g.live;
    g.lead &= g.live; g.L &= g.live; g.LN &= g.live; g.hash &= g.live; g.dot &= g.live; g.u2026 &= g.live;
    return g;
}

// edge: a document starts AT byte i; eend: a document ends BEHIND byte i.  prev_nw: the byte before the granule is a byte of a word
// of the same document (trail of the granule before > 0 and no edge at byte 0)
JTK_HD uint32_t jtk_wd_starts(const JtkWdGran& g, uint32_t edge, uint32_t prev_nw) { return g.nw & (edge | ~((g.nw << 1) | prev_nw)); }
JTK_HD uint32_t jtk_wd_ends(const JtkWdGran& g, uint32_t eend) { return g.nw & (eend | ~((g.nw >> 1) | (g.next_nw << 15))); }

// the three-state transform of a seed mask filled forward (blocked into byte i from below: not a word byte, or an edge) and
// backward (blocked from above: not a word byte, or a document's end behind it)
JTK_HD uint32_t jtk_wd_t_fwd(uint32_t seed, uint32_t blocked) {
    if (jtk_wd_fill_up(seed, blocked) & 0x8000u) return JTK_WD_T_SET;
    return (blocked & 0xFFFFu) ? JTK_WD_T_RESET : JTK_WD_T_ID;
}
JTK_HD uint32_t jtk_wd_t_bwd(uint32_t seed, uint32_t blocked) {
    if (jtk_wd_fill_down(seed, blocked) & 1u) return JTK_WD_T_SET;
    return (blocked & 0xFFFFu) ? JTK_WD_T_RESET : JTK_WD_T_ID;
}
// per byte: has the word an item of `seed` at or before it (cin: the state before the granule); at or behind it
JTK_HD uint32_t jtk_wd_seen_fwd(uint32_t seed, uint32_t blocked, uint32_t cin) {
    return jtk_wd_fill_up(seed, blocked) | (cin ? jtk_wd_below_first(blocked & 0xFFFFu) : 0u);
}
JTK_HD uint32_t jtk_wd_seen_bwd(uint32_t seed, uint32_t blocked, uint32_t cin) {
    return jtk_wd_fill_down(seed, blocked) | (cin ? jtk_wd_above_last(blocked & 0xFFFFu) : 0u);
}

// the word bytes at the granule's end that belong to the word (of one document) its last byte is in: 0 .. 16
JTK_HD uint32_t jtk_wd_trail(const JtkWdGran& g, uint32_t edge) {
    // a byte stops the run when it is no word byte, or when the byte above it starts a document
    const uint32_t stop = (~g.nw | (edge >> 1)) & 0xFFFFu;
    if (!(g.nw & 0x8000u)) return 0u;
    const uint32_t low = stop & 0x7FFFu;                         // (bit 15 itself is a word byte; an edge above it is the next granule's)
    return low ? 15u - (uint32_t)(31 - __builtin_clz(low)) : 16u;
}

// ---- dots.  c: the length modulo 3 of the dot run that ends at the byte before the granule (0 behind an edge at byte 0).  The
// bits of the result: one per ellipsis, at the byte where its triple starts (byte 0 for one that starts before the granule)
JTK_HD uint32_t jtk_wd_ellipses(uint32_t dot, uint32_t edge, uint32_t c) {
    if (edge & 1u) c = 0;
    const uint32_t d = (dot << c) | ((1u << c) - 1u), e = edge << c;
    const uint32_t link = d & (d << 1) & ~e;                     // byte i continues the run of byte i - 1
    const uint32_t d3 = d & (link >> 1) & (link >> 2);           // a triple can start at i
    uint32_t m = d & ~link & d3, marks = 0;
#pragma unroll
    for (int k = 0; k < 6; k++) {
        marks |= m;
        m = (m << 3) & link & d3;
    }
    return (marks >> c) | ((marks & ((1u << c) - 1u)) ? 1u : 0u);
}
// the granule's dot transform (valid == 16; a shorter granule is the text's last and its transform is not used)
JTK_HD uint32_t jtk_wd_dot_t(uint32_t dot, uint32_t edge) {
    if (!(dot & 0x8000u)) return JTK_WD_DOT_FIX;
    const uint32_t link = dot & (dot << 1) & ~edge;              // (bit 0: never linked here)
    const uint32_t heads = dot & ~link & 0xFFFEu;                // run starts the granule decides alone
    if (heads) return JTK_WD_DOT_FIX | ((16u - (uint32_t)(31 - __builtin_clz(heads))) % 3u);
    return (edge & 1u) ? (JTK_WD_DOT_FIX | (16u % 3u)) : (16u % 3u);
}

// ---- stop words
struct JtkWdStops {
    uint64_t key[JTK_WD_MAX_STOP]; // the words sorted by length, their bytes little-endian from bit 0
    uint8_t idx[JTK_WD_MAX_STOP];  // the word's index in the caller's list
    uint8_t first[JTK_WD_MAX_STOP_LEN + 2];     // key[first[n] .. first[n + 1]) are the words of n bytes
    uint32_t fold;
};
JTK_HD uint64_t jtk_wd_fold(uint64_t x) {                        // 'A'..'Z' -> 'a'..'z' in every byte
    const uint64_t y = x & 0x7F7F7F7F7F7F7F7Full;
    const uint64_t up = (y + 0x3F3F3F3F3F3F3F3Full) & ~(y + 0x2525252525252525ull) & ~x & 0x8080808080808080ull;
    return x | (up >> 2);
}
// the 8 bytes that end with byte i of the granule, byte i in bits 56-63: p23 = bytes 8..15 of the granule before, x01 / x23 = the
// granule's halves, all little-endian
JTK_HD uint64_t jtk_wd_tail8(uint64_t p23, uint64_t x01, uint64_t x23, int i) {
    const uint64_t lo = i < 8 ? p23 : x01, hi = i < 8 ? x01 : x23;
    const int j = (i & 7) + 1;                                   // bytes of hi that take part
    return j == 8 ? hi : (lo >> (8 * j)) | (hi << (64 - 8 * j));
}
// The word that ends at byte i: its length from the start bits at or below i, else from the trail of the granule before
// (prev_trail; 0 behind an edge at byte 0).  0: longer than 8 bytes.  *key: its bytes, as JtkWdStops has them.
JTK_HD uint32_t jtk_wd_word_at_end(uint32_t starts, uint32_t prev_trail, uint64_t p23, uint64_t x01, uint64_t x23, int i, uint32_t fold,
                                   uint64_t* key) {
    const uint32_t below = starts & ((2u << i) - 1u);
    const uint32_t len = below ? (uint32_t)i - (uint32_t)(31 - __builtin_clz(below)) + 1u : (uint32_t)i + 1u + prev_trail;
    if (len > JTK_WD_MAX_STOP_LEN) return 0u;
    uint64_t k = jtk_wd_tail8(p23, x01, x23, i) >> (8 * (8 - len));
    if (fold) k = jtk_wd_fold(k);
    *key = k;
    return len;
}
// the bits of the list's words that equal (len, key); 0: none
JTK_HD uint32_t jtk_wd_stop_bits(const uint64_t* keys, const uint8_t* idx, const uint8_t* first, uint32_t len, uint64_t key) {
    uint32_t bits = 0;
    for (uint32_t j = first[len]; j < first[len + 1]; j++)
        if (keys[j] == key) bits |= 1u << idx[j];
    return bits;
}

// ---- lines: a unit [b, e) of the held list, e > b; t = its first 3 and last 3 bytes (0 where it has fewer)
#define JTK_WD_LINE_BULLET 1u
#define JTK_WD_LINE_ELLIPSIS 2u
#define JTK_WD_LINE_TERMINAL 4u
JTK_HD uint32_t jtk_wd_line_flags(uint32_t h0, uint32_t h1, uint32_t h2, uint32_t t0, uint32_t t1, uint32_t t2, int64_t len) {
    uint32_t f = 0;
    if (h0 == 0x2Du || (len >= 3 && h0 == 0xE2u && h1 == 0x80u && h2 == 0xA2u)) f |= JTK_WD_LINE_BULLET;
    if (len >= 3 && ((t0 == 0x2Eu && t1 == 0x2Eu && t2 == 0x2Eu) || (t0 == 0xE2u && t1 == 0x80u && t2 == 0xA6u))) f |= JTK_WD_LINE_ELLIPSIS;
    if (t2 == 0x2Eu || t2 == 0x21u || t2 == 0x3Fu || t2 == 0x22u) f |= JTK_WD_LINE_TERMINAL;
    return f;
}

#endif  // JTK_WORDS_RULES_H
