// jtk_lines_rules.h -- duplicate lines and paragraphs inside a document (jtk_batch_line_units, jtk_batch_line_repeats): the rule
// the device kernels (jtk_lines.hip) and the CPU test shim tests/lines_sim share.  The line-level half of Gopher's repetition
// filters (Rae et al., "Scaling Language Models", table A1), which RedPajama-v2, Dolma and FineWeb / datatrove carry: the
// fraction of a document's lines, and of its paragraphs, that are duplicates -- counted in units and in characters.  A pass over
// the TEXT of the last encode, not over its tokens.  Integer only: every result is exact.
//
// The rule, all arithmetic modulo 2^64; G = JTK_MH_G, mix = the splitmix64 finaliser (jtk_fim_mix):
//   text        document d of the batch is the bytes x[a, e), a = doc_off[d], e = doc_off[d + 1].  A document with status < 0
//               has no units, whatever its text.
//   parameters  seed, doc_index_base, unit = JTK_LINES_LINE (0) or JTK_LINES_PARAGRAPH (1), flags out of JTK_LINES_MARK_FIRST
//               (1u) and JTK_LINES_TRIM (2u); anything else is refused.
//   bytes       the only line break is 0x0A.  W, the blank set, is empty without TRIM and {0x20, 0x09, 0x0D} with it.  A byte is
//               INK when it is neither 0x0A nor in W.
//   units       a raw line is a maximal run of bytes of the document without 0x0A (the document's start and end bound raw
//               lines: nothing crosses a document edge); it is blank when it has no ink.  LINE: for each non-blank raw line,
//               [its first ink byte, its last ink byte + 1).  PARAGRAPH: for each maximal run of consecutive non-blank raw lines,
//               [the first ink byte of the first line, the last ink byte of the last line + 1); the bytes in between, line
//               breaks and blanks included, are part of the unit unchanged.
//   per byte    (the form the kernels take) an ink byte p STARTS a unit when its document has no earlier ink byte, or when the
//               number of 0x0A between the previous ink byte and p is >= 1 (LINE) or >= 2 (PARAGRAPH); it ENDS a unit when the
//               same holds towards the next ink byte, or there is none.  The carry from byte to byte is "no ink yet in this
//               document" (JTK_LN_NOINK) or "newlines since the last ink, saturated at 2".
//   what this   without TRIM: re.split("\n+") for LINE and re.split("\n{2,}") for PARAGRAPH on a document stripped of leading and
//   matches     trailing newlines -- what datatrove's Gopher repetition filter does after strip() (its strip also takes other
//               white space off the document's ends; TRIM does that, and for every line).  With TRIM, CRLF text and lines that
//               differ only in indentation or trailing blanks behave as RedPajama-v2's normalised lines do (its normalisation
//               also lower-cases and drops punctuation; this rule does not).  No more is claimed.
//   hash        key = mix(seed + G * (unit + 161)) (MinHash has n + 1, the n-gram set n + 33, n-gram repeats n + 97, n <= 32: no
//               shared key family; FIM's mix(seed + G * (g + 1)) runs over document indices g and is a family of draws, not of
//               keys that are compared with these).  key_D = jtk_rp_doc_key(key, doc_index_base, d).  H = H * G + byte + 1 over
//               the unit's bytes, from 0;  k = mix(H ^ key_D), and G where that is 0.  Two units of ONE document are the same
//               when their k are equal; units of different documents are never compared.
//   per unit    u (units of a document in text order): first(u) = the smallest document-relative index with u's k, count(u) the
//               number of units with it (as in jtk_repeat_rules.h).  A repeat: first(u) < u; with JTK_LINES_MARK_FIRST: count(u)
//               >= 2.  chars of a byte range = its bytes b with (b & 0xC0) != 0x80 (the weight of JTK_UNIT_CODEPOINT in
//               jtk_charpos_rules.h; defined for any bytes).
//   results     per unit, in document order then text order: begin, end (batch byte positions), flag (1 for a repeat).  Per
//               document: unit_off [n_docs + 1]; n_dup, dup_bytes, dup_chars over the flagged units; unit_bytes, unit_chars over
//               all units; doc_chars over [a, e) (whatever the status); top_count = the largest count (0 without units),
//               top_first = the document-relative index of the first unit with that count (-1 without units).
//
// What the device may deviate in, and the bound (as jtk_repeat_rules.h states it): one table holds the units of a GROUP of
// documents and is keyed by k alone, so two units of different documents whose k coincide -- under different key_D: probability
// 2^-64 per pair -- would be conflated.  For a table holding m units the expected number of such pairs is at most m^2 / 2^65.
//
// How the kernels walk the text (and the shim with them).  The batch's text is cut into granules of JTK_LN_GRANULE = 16 bytes
// at multiples of 16 of the batch (one lane each), JTK_LN_WAVE_BYTES = 1024 (a wave) and tiles of JTK_LN_TILE = 4096 (a
// workgroup).  Two bit planes over the text say where a non-empty document starts (the EDGE plane; one more bit at the end of
// the last document) and whether the document that starts there is refused (the REF plane).  Three things are carried along
// the text, each as an associative summary so that no lane ever walks further than its granule:
//   the carry   a transform on {NOINK, 0, 1, 2} (jtk_ln_then / jtk_ln_apply): an ink byte fixes 0, a document edge fixes NOINK, a
//               newline adds 1 up to 2.  Forward it decides the starts, run backward over the same bytes it decides the ends.
//   the hash    P(q) = H of the batch's bytes [0, q): (m1, h1) o (m2, h2) = (m1 m2, h1 m2 + h2) with m = G^length.  H of the unit
//               [b, e) is P(e) - P(b) * G^(e - b): exact modulo 2^64.  G^(e - b) takes at most 64 squarings.
//   the counts  units started and chars before q.
// Pass A writes a tile's summaries (jtk_ln_tile_word: both transforms and, for the one ink byte whose start the tile cannot decide
// alone -- the first, with no document edge before it --, the newlines before it); pass B, one workgroup, scans the summaries
// JTK_LN_SCAN_STEP tiles at a step; pass C repeats pass A's work with the carries and writes every unit's begin, P, chars at its
// start byte and end, P, chars at its end byte: the unit index of an end byte is the number of starts up to it, minus 1.  Then one
// lane per unit: k and chars.  No workgroup waits for another: every carry crosses a kernel boundary.
//
// The table and the groups are jtk_repeat_rules.h's (JtkRpTable, jtk_rp_claim, jtk_rp_find, jtk_rp_is_repeat, jtk_rp_top_pack),
// with unit indices of the batch in place of token positions; jtk_ln_group_end plans from unit_off.
#ifndef JTK_LINES_RULES_H
#define JTK_LINES_RULES_H

#include <stdint.h>

#include "jtk_repeat_rules.h"

#define JTK_LN_HD JTK_RP_HD

#ifndef JTK_LINES_LINE
#define JTK_LINES_LINE 0           // (as in include/jtokkit_amd.h)
#define JTK_LINES_PARAGRAPH 1
#define JTK_LINES_MARK_FIRST 1u
#define JTK_LINES_TRIM 2u
#endif
static_assert(JTK_LINES_MARK_FIRST == JTK_REPEAT_MARK_FIRST, "jtk_rp_is_repeat takes the flags as they are");

#define JTK_LN_GRANULE 16
#define JTK_LN_WAVE_BYTES (64 * JTK_LN_GRANULE)
#define JTK_LN_TILE (4 * JTK_LN_WAVE_BYTES)
#define JTK_LN_TILE_GRANULES (JTK_LN_TILE / JTK_LN_GRANULE)
#define JTK_LN_SCAN_STEP 1024      // tiles per step of pass B
#define JTK_LN_KEY_C 161
#define JTK_LN_MAX_DOC_UNITS JTK_RP_MAX_DOC_TOKENS
#define JTK_LN_UNIT_BYTES 48       // held per unit: begin, end, k, chars, and the two prefixes at the end byte

// the carry
#define JTK_LN_NOINK 3u            // no ink yet in this document; 0, 1, 2: newlines since the last ink
#define JTK_LN_T_ID 0u             // a transform: bit 4 = it fixes the state, bits 2-3 = to what; else bits 0-1 = newlines to add
#define JTK_LN_T_NL 1u
#define JTK_LN_T_INK 16u
#define JTK_LN_T_EDGE (16u | (JTK_LN_NOINK << 2))

JTK_LN_HD bool jtk_ln_params_ok(int32_t unit, uint32_t flags) {
    return (unit == JTK_LINES_LINE || unit == JTK_LINES_PARAGRAPH) && (flags & ~(JTK_LINES_MARK_FIRST | JTK_LINES_TRIM)) == 0;
}
JTK_LN_HD uint64_t jtk_ln_key(uint64_t seed, int32_t unit) { return jtk_fim_mix(seed + JTK_MH_G * ((uint64_t)unit + (uint64_t)JTK_LN_KEY_C)); }
JTK_LN_HD uint32_t jtk_ln_threshold(int32_t unit) { return unit == JTK_LINES_PARAGRAPH ? 2u : 1u; }

JTK_LN_HD uint32_t jtk_ln_fix(uint32_t state) { return 16u | (state << 2); }
JTK_LN_HD uint32_t jtk_ln_apply(uint32_t t, uint32_t s) {
    if (t & 16u) return (t >> 2) & 3u;
    if (s == JTK_LN_NOINK) return s;
    const uint32_t x = s + (t & 3u);
    return x > 2u ? 2u : x;
}
// a, then b
JTK_LN_HD uint32_t jtk_ln_then(uint32_t a, uint32_t b) {
    if (b & 16u) return b;
    if (a & 16u) return jtk_ln_fix(jtk_ln_apply(b, (a >> 2) & 3u));
    const uint32_t x = (a & 3u) + (b & 3u);
    return x > 2u ? 2u : x;
}
// does an ink byte that sees state s before it (behind it, for an end) start (end) a unit?
JTK_LN_HD bool jtk_ln_breaks(uint32_t s, uint32_t thr) { return s == JTK_LN_NOINK || s >= thr; }

// ---- a granule: bit i of every mask is byte i
struct JtkLnGran {
    uint32_t ink, nl, nonc;        // ink and newline bytes that count (valid, not in a refused document); bytes with a char weight
};
// `refused`: the bytes of the granule that lie in a refused document (jtk_ln_refused_mask)
JTK_LN_HD JtkLnGran jtk_ln_classify(const uint32_t* w4, int valid, uint32_t flags, uint32_t refused) {
    JtkLnGran g{0, 0, 0};
#pragma unroll
    for (int i = 0; i < JTK_LN_GRANULE; i++) {
        if (i >= valid) break;
        const uint32_t b = (w4[i >> 2] >> (8 * (i & 3))) & 0xFFu;
        const bool nl = b == 0x0Au;
        const bool blank = (flags & JTK_LINES_TRIM) && (b == 0x20u || b == 0x09u || b == 0x0Du);
        if (nl) g.nl |= 1u << i;
        else if (!blank) g.ink |= 1u << i;
        if ((b & 0xC0u) != 0x80u) g.nonc |= 1u << i;
    }
    g.ink &= ~refused;
    g.nl &= ~refused;
    return g;
}
// the bytes of a granule inside a refused document: r_in says whether the byte before the granule is (or, at a tile's start,
// whether the document there is); edge / ref are the granule's bits of the two planes.  *r_out: the same for the next granule.
JTK_LN_HD uint32_t jtk_ln_refused_mask(uint32_t edge, uint32_t ref, uint32_t r_in, uint32_t* r_out) {
    uint32_t m = 0, r = r_in;
#pragma unroll
    for (int i = 0; i < JTK_LN_GRANULE; i++) {
        if ((edge >> i) & 1u) r = (ref >> i) & 1u;
        m |= r << i;
    }
    *r_out = r;
    return m;
}
// the granule's transform forward (edge: a document starts AT byte i) and backward (eend: a document ends BEHIND byte i)
JTK_LN_HD uint32_t jtk_ln_gran_fwd(const JtkLnGran& g, uint32_t edge) {
    uint32_t t = JTK_LN_T_ID;
#pragma unroll
    for (int i = 0; i < JTK_LN_GRANULE; i++) {
        if ((edge >> i) & 1u) t = JTK_LN_T_EDGE;
        if ((g.ink >> i) & 1u) t = JTK_LN_T_INK;
        else if ((g.nl >> i) & 1u) t = jtk_ln_then(t, JTK_LN_T_NL);
    }
    return t;
}
JTK_LN_HD uint32_t jtk_ln_gran_bwd(const JtkLnGran& g, uint32_t eend) {
    uint32_t t = JTK_LN_T_ID;
#pragma unroll
    for (int i = JTK_LN_GRANULE - 1; i >= 0; i--) {
        if ((eend >> i) & 1u) t = JTK_LN_T_EDGE;
        if ((g.ink >> i) & 1u) t = JTK_LN_T_INK;
        else if ((g.nl >> i) & 1u) t = jtk_ln_then(t, JTK_LN_T_NL);
    }
    return t;
}
// the start bits of a granule whose bytes follow the transform t_in (from the tile's start in pass A: an ink byte that it does
// not decide is reported in *open as 4 | the newlines before it, and has no bit; from a known state in pass C: t_in fixes)
JTK_LN_HD uint32_t jtk_ln_starts(const JtkLnGran& g, uint32_t edge, uint32_t t_in, uint32_t thr, uint32_t* open) {
    uint32_t t = t_in, bits = 0;
#pragma unroll
    for (int i = 0; i < JTK_LN_GRANULE; i++) {
        if ((edge >> i) & 1u) t = JTK_LN_T_EDGE;
        if ((g.ink >> i) & 1u) {
            if (t & 16u) bits |= (uint32_t)jtk_ln_breaks((t >> 2) & 3u, thr) << i;
            else *open = 4u | (t & 3u);
            t = JTK_LN_T_INK;
        } else if ((g.nl >> i) & 1u) {
            t = jtk_ln_then(t, JTK_LN_T_NL);
        }
    }
    return bits;
}
// the end bits of a granule behind which the state (backward) is s_in
JTK_LN_HD uint32_t jtk_ln_ends(const JtkLnGran& g, uint32_t eend, uint32_t s_in, uint32_t thr) {
    uint32_t s = s_in, bits = 0;
#pragma unroll
    for (int i = JTK_LN_GRANULE - 1; i >= 0; i--) {
        if ((eend >> i) & 1u) s = JTK_LN_NOINK;
        if ((g.ink >> i) & 1u) {
            bits |= (uint32_t)jtk_ln_breaks(s, thr) << i;
            s = 0;
        } else if ((g.nl >> i) & 1u) {
            s = jtk_ln_apply(JTK_LN_T_NL, s);
        }
    }
    return bits;
}
// does the tile's open ink byte (jtk_ln_starts) start a unit, the state before the tile being s?
JTK_LN_HD uint32_t jtk_ln_open_starts(uint32_t open, uint32_t s, uint32_t thr) {
    return (open & 4u) && jtk_ln_breaks(jtk_ln_apply(open & 3u, s), thr) ? 1u : 0u;
}
// a tile's summary word: forward transform | backward transform << 5 | open << 10
JTK_LN_HD uint32_t jtk_ln_tile_word(uint32_t tf, uint32_t tb, uint32_t open) { return tf | (tb << 5) | (open << 10); }
JTK_LN_HD uint32_t jtk_ln_word_fwd(uint32_t w) { return w & 31u; }
JTK_LN_HD uint32_t jtk_ln_word_bwd(uint32_t w) { return (w >> 5) & 31u; }
JTK_LN_HD uint32_t jtk_ln_word_open(uint32_t w) { return (w >> 10) & 7u; }

// ---- the hash
JTK_LN_HD constexpr uint64_t jtk_ln_pow(uint64_t e) {              // G^e: at most 64 squarings
    uint64_t r = 1, g = JTK_MH_G;
    while (e) {
        if (e & 1u) r *= g;
        g *= g;
        e >>= 1;
    }
    return r;
}
JTK_LN_HD uint64_t jtk_ln_step(uint64_t h, uint32_t byte) { return h * JTK_MH_G + (uint64_t)byte + 1ull; }
// H of the 16 bytes of a granule, from 0 (bytes behind the text's end are whatever was loaded: no prefix that is used holds them)
JTK_LN_HD uint64_t jtk_ln_gran_hash(const uint32_t* w4) {
    uint64_t h = 0;
#pragma unroll
    for (int i = 0; i < JTK_LN_GRANULE; i++) h = jtk_ln_step(h, (w4[i >> 2] >> (8 * (i & 3))) & 0xFFu);
    return h;
}
// H of [b, e) from the prefixes P(b), P(e)
JTK_LN_HD uint64_t jtk_ln_range_hash(uint64_t pb, uint64_t pe, int64_t len) { return pe - pb * jtk_ln_pow((uint64_t)len); }
JTK_LN_HD uint64_t jtk_ln_finish(uint64_t h, uint64_t key_d) {
    const uint64_t k = jtk_fim_mix(h ^ key_d);
    return k ? k : JTK_MH_G;
}

// ---- documents and groups
// the document of unit u of the batch: the d with unit_off[d] <= u < unit_off[d + 1]
JTK_LN_HD int64_t jtk_ln_doc_of_unit(const int64_t* unit_off, int64_t n_docs, int64_t u) { return jtk_first_gt(unit_off, 1, n_docs + 1, u) - 1; }
// the last d in [0, n_docs] with doc_off[d] <= q: the non-empty document that holds byte q; n_docs at the text's end; -1 before
// the first document
JTK_LN_HD int64_t jtk_ln_doc_at(const int64_t* doc_off, int64_t n_docs, int64_t q) { return jtk_first_gt(doc_off, 0, n_docs + 1, q) - 1; }

// The group that starts at document d0 < n_docs: one past its last document, and *m = its units (jtk_rp_group_end with unit
// counts: a refused document has none by the time unit_off exists).
inline int64_t jtk_ln_group_end(const int64_t* unit_off, int64_t n_docs, int64_t d0, int64_t budget_bytes, int64_t* m) {
    int64_t have = 0, d = d0;
    for (; d < n_docs; d++) {
        const int64_t md = unit_off[d + 1] - unit_off[d];
        if (d > d0 && jtk_rp_table_bytes(have + md) > budget_bytes) break;
        have += md;
    }
    *m = have;
    return d;
}

#endif  // JTK_LINES_RULES_H
