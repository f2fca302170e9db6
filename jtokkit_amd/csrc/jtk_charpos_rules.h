// jtk_charpos_rules.h -- character positions of the batch text (jtk_batch_char_index, _char_positions, _byte_positions,
// _token_char_offsets): the rule that the device kernels (jtk_charpos.hip) and the CPU test shim tests/charpos_sim share.
// Every other position the library hands out is a byte position in String.getBytes(UTF_8); this converts between those and
// indices into a Java String (UTF-16 units) or a Python str (code points).
//
// The rule is per byte and defined for ANY bytes.  The weight w(x) of a byte x:
//   JTK_CP_UNIT_CODEPOINT   1 if (x & 0xC0) != 0x80 (x is no continuation byte), else 0
//   JTK_CP_UNIT_UTF16       the code-point weight, plus 1 if x >= 0xF0 (a 4-byte lead is a surrogate pair)
//   JTK_CP_UNIT_BYTE        1
// For a WELL-FORMED document the sums below are the indices of new String(bytes, UTF_8) (UTF16) and of bytes.decode("utf-8")
// (CODEPOINT).  For a document that is not well-formed they are still the sums of the weights, not what a decoder that
// substitutes U+FFFD would count; JTK_ENCODE_VALIDATE_UTF8 finds such documents (status JTK_ERR_BAD_UTF8).
//
// Document d is [a, e) = [doc_off[d], doc_off[d + 1]).  U(a, q) = the sum of w(text[i]) over a <= i < q.  A position q in
// [a, e] is a BOUNDARY if q == a, q == e, or text[q] is no continuation byte.
//   snap(p)        JTK_CP_FLOOR: the nearest boundary at or before p; JTK_CP_CEIL: at or after p; within 3 bytes of p and
//                  inside [a, e].  Without one within 3 bytes (text that is not well-formed) snap(p) = p.
//   forward        char_index(d, p, unit, round) = U(a, snap(p)) for a <= p <= e; -1 for p outside [a, e] or a bad d.  FLOOR is
//                  the index of the character that holds byte p (tiktoken's convention for a token that starts inside a
//                  character), CEIL counts a partly covered character in: the exclusive end.
//   inverse        byte_pos(d, k, unit) = the largest boundary q in [a, e] with U(a, q) <= k; -1 for k < 0, e for k >= U(a, e).
//                  A UTF-16 index that points at a low surrogate floors to the start of its 4-byte character.
//   doc_units[d]   U(a, e): String.length(), len(str).
//   document of p  without a document given, the last d with doc_off[d] <= p: a position on a document edge belongs to the
//                  document that starts there, n_bytes to the last document.
//
// How it is computed: a rank / select index over the batch text, counted from the start of the text (not per document):
//   sup[k]   int64   units before superblock k (JTK_CP_SUPER = 4096 bytes); sup[n_sup] = the total
//   sub[j]   uint16  units before block j (JTK_CP_BLOCK = 64 bytes) inside its superblock (at most 63 * 64 * 2)
// rank(q) = sup + sub + a masked word-at-a-time count of the < 64 bytes of q's own block (jtk_cp_rank); the inverse is a search
// over sup, then over the superblock's sub entries, then over the block's words and bytes (jtk_cp_select).  Bytes at or past
// n_bytes count 0 and no read goes past the 16-byte granule that holds byte n_bytes - 1.  The text is 16-byte aligned.
#ifndef JTK_CHARPOS_RULES_H
#define JTK_CHARPOS_RULES_H

#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define JTK_CP_HD __host__ __device__ inline
#else
#define JTK_CP_HD inline
#endif

#define JTK_CP_UNIT_BYTE 0                                  // = JTK_UNIT_BYTE, JTK_UNIT_UTF16, JTK_UNIT_CODEPOINT of jtokkit_amd.h
#define JTK_CP_UNIT_UTF16 1
#define JTK_CP_UNIT_CODEPOINT 2
#define JTK_CP_FLOOR 0                                      // = JTK_CHAR_FLOOR, JTK_CHAR_CEIL
#define JTK_CP_CEIL 1

#define JTK_CP_SUPER 4096                                   // bytes per superblock
#define JTK_CP_BLOCK 64                                     // bytes per block
#define JTK_CP_SUPER_SHIFT 12
#define JTK_CP_BLOCK_SHIFT 6
#define JTK_CP_BLOCKS_PER_SUPER (JTK_CP_SUPER / JTK_CP_BLOCK)

struct alignas(16) JtkCpQuad { uint32_t w[4]; };            // 16 bytes of text, byte i of the granule in bits 8 (i % 4) .. of w[i / 4]

// the index and the text it was built over
struct JtkCharIndex {
    const uint8_t* text;        // 16-byte aligned; readable up to the next multiple of 16 past n_bytes
    int64_t n_bytes;
    const int64_t* sup;         // [n_sup + 1]
    const uint16_t* sub;        // [n_sup * JTK_CP_BLOCKS_PER_SUPER]
    int64_t n_sup;              // ceil(n_bytes / JTK_CP_SUPER)
    int unit;
};

JTK_CP_HD bool jtk_cp_valid_unit(int unit) { return unit == JTK_CP_UNIT_BYTE || unit == JTK_CP_UNIT_UTF16 || unit == JTK_CP_UNIT_CODEPOINT; }
JTK_CP_HD bool jtk_cp_valid_round(int round) { return round == JTK_CP_FLOOR || round == JTK_CP_CEIL; }

JTK_CP_HD bool jtk_cp_is_cont(uint8_t x) { return (x & 0xC0u) == 0x80u; }

JTK_CP_HD uint32_t jtk_cp_weight(uint8_t x, int unit) {
    if (unit == JTK_CP_UNIT_BYTE) return 1u;
    return (jtk_cp_is_cont(x) ? 0u : 1u) + ((unit == JTK_CP_UNIT_UTF16 && x >= 0xF0u) ? 1u : 0u);
}

JTK_CP_HD uint32_t jtk_cp_popc(uint32_t v) { return (uint32_t)__builtin_popcount(v); }   // (what __popc is on the device)

// bit 7 of every byte of v that is a continuation byte / that is >= 0xF0
JTK_CP_HD uint32_t jtk_cp_cont_bits(uint32_t v) { return (v & 0x80808080u) & ~((v << 1) & 0x80808080u); }
JTK_CP_HD uint32_t jtk_cp_f0_bits(uint32_t v) { return v & (v << 1) & (v << 2) & (v << 3) & 0x80808080u; }

// the units of the first `valid` bytes (0 .. 4) of a 4-byte word
JTK_CP_HD uint32_t jtk_cp_word_units(uint32_t v, int valid, int unit) {
    if (valid <= 0) return 0u;
    const uint32_t m = valid >= 4 ? 0x80808080u : (0x80808080u & ((1u << (8 * valid)) - 1u));
    if (unit == JTK_CP_UNIT_BYTE) return (uint32_t)(valid >= 4 ? 4 : valid);
    uint32_t n = jtk_cp_popc(~jtk_cp_cont_bits(v) & m);
    if (unit == JTK_CP_UNIT_UTF16) n += jtk_cp_popc(jtk_cp_f0_bits(v) & m);
    return n;
}

// the units of the first `valid` bytes (any value; 16 or more: all) of a 16-byte granule
JTK_CP_HD uint32_t jtk_cp_quad_units(const JtkCpQuad& g, int64_t valid, int unit) {
    uint32_t n = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int64_t left = valid - 4 * k;
        n += jtk_cp_word_units(g.w[k], left >= 4 ? 4 : (int)(left > 0 ? left : 0), unit);
    }
    return n;
}

JTK_CP_HD JtkCpQuad jtk_cp_load_quad(const uint8_t* text, int64_t off) { return *reinterpret_cast<const JtkCpQuad*>(text + off); }

// ---- snap: p in [a, e]
JTK_CP_HD bool jtk_cp_is_boundary(const uint8_t* text, int64_t a, int64_t e, int64_t q) {
    return q == a || q == e || !jtk_cp_is_cont(text[q]);               // (text[e] is never read)
}
JTK_CP_HD int64_t jtk_cp_snap(const uint8_t* text, int64_t a, int64_t e, int64_t p, int round) {
    if (round == JTK_CP_FLOOR) {
        for (int64_t q = p; q >= a && q >= p - 3; q--)
            if (jtk_cp_is_boundary(text, a, e, q)) return q;
    } else {
        for (int64_t q = p; q <= e && q <= p + 3; q++)
            if (jtk_cp_is_boundary(text, a, e, q)) return q;
    }
    return p;
}

// ---- document [a, e) of the offsets, clamped into [0, n_bytes] and to e >= a (offsets that an encode refused read nothing
// outside the text)
JTK_CP_HD int64_t jtk_cp_clamp(int64_t v, int64_t n_bytes) { return v < 0 ? 0 : v > n_bytes ? n_bytes : v; }
JTK_CP_HD void jtk_cp_doc_range(const int64_t* doc_off, int64_t d, int64_t n_bytes, int64_t* a, int64_t* e) {
    *a = jtk_cp_clamp(doc_off[d], n_bytes);
    const int64_t x = jtk_cp_clamp(doc_off[d + 1], n_bytes);
    *e = x < *a ? *a : x;
}
// the document of position p: the last d in [0, n_docs) with doc_off[d] <= p; -1 without one or for p outside [0, n_bytes]
JTK_CP_HD int64_t jtk_cp_doc_of(const int64_t* doc_off, int64_t n_docs, int64_t n_bytes, int64_t p) {
    if (p < 0 || p > n_bytes || n_docs <= 0) return -1;
    int64_t lo = 0, hi = n_docs;                                       // the first d in [0, n_docs) with doc_off[d] > p
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (doc_off[mid] > p) hi = mid; else lo = mid + 1;
    }
    return lo - 1;
}

// ---- rank: the units of text[0, q), 0 <= q <= n_bytes
JTK_CP_HD int64_t jtk_cp_rank(const JtkCharIndex& ix, int64_t q) {
    int64_t r = ix.sup[q >> JTK_CP_SUPER_SHIFT];
    if ((q & (JTK_CP_SUPER - 1)) == 0) return r;                       // (q == n_sup * JTK_CP_SUPER has no sub entry)
    r += ix.sub[q >> JTK_CP_BLOCK_SHIFT];
    const int64_t b0 = q & ~(int64_t)(JTK_CP_BLOCK - 1);
    for (int64_t g = b0; g < q; g += 16) r += jtk_cp_quad_units(jtk_cp_load_quad(ix.text, g), q - g, ix.unit);
    return r;
}

// ---- forward: document d (checked), position p
JTK_CP_HD int64_t jtk_cp_char_index(const JtkCharIndex& ix, const int64_t* doc_off, const int64_t* dunit, int64_t n_docs, int64_t d,
                                    int64_t p, int round) {
    if (d < 0 || d >= n_docs) return -1;
    int64_t a, e;
    jtk_cp_doc_range(doc_off, d, ix.n_bytes, &a, &e);
    if (p < a || p > e) return -1;
    return jtk_cp_rank(ix, jtk_cp_snap(ix.text, a, e, p, round)) - dunit[d];
}

// ---- inverse: the largest boundary q of document d with U(a, q) <= k
JTK_CP_HD int64_t jtk_cp_byte_pos(const JtkCharIndex& ix, const int64_t* doc_off, const int64_t* dunit, int64_t n_docs, int64_t d,
                                  int64_t k) {
    if (d < 0 || d >= n_docs || k < 0) return -1;
    int64_t a, e;
    jtk_cp_doc_range(doc_off, d, ix.n_bytes, &a, &e);
    if (k >= dunit[d + 1] - dunit[d]) return e;
    // rank(a) <= T < rank(e), so a < e.  The answer is the largest q with rank(q) <= T: rank(q + 1) > T makes text[q] a byte
    // with a weight, which no continuation byte has (JTK_CP_UNIT_BYTE: see the end).
    const int64_t T = dunit[d] + k;
    int64_t lo = a >> JTK_CP_SUPER_SHIFT, hi = ((e - 1) >> JTK_CP_SUPER_SHIFT) + 1;     // the first superblock of the document's with sup > T
    const int64_t s_first = lo;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (ix.sup[mid] > T) hi = mid; else lo = mid + 1;
    }
    const int64_t s = lo - 1 < s_first ? s_first : lo - 1;
    const int64_t rem = T - ix.sup[s];
    int64_t jl = s * JTK_CP_BLOCKS_PER_SUPER, jh = jl + JTK_CP_BLOCKS_PER_SUPER;          // the first block of s (and of the document) with sub > rem
    if (jl < (a >> JTK_CP_BLOCK_SHIFT)) jl = a >> JTK_CP_BLOCK_SHIFT;
    if (jh > ((e - 1) >> JTK_CP_BLOCK_SHIFT) + 1) jh = ((e - 1) >> JTK_CP_BLOCK_SHIFT) + 1;
    const int64_t j_first = jl;
    while (jl < jh) {
        const int64_t mid = (jl + jh) >> 1;
        if ((int64_t)ix.sub[mid] > rem) jh = mid; else jl = mid + 1;
    }
    const int64_t j = jl - 1 < j_first ? j_first : jl - 1;
    const int64_t start = j << JTK_CP_BLOCK_SHIFT;
    const int64_t end = start + JTK_CP_BLOCK < e ? start + JTK_CP_BLOCK : e;
    int64_t run = ix.sup[s] + ix.sub[j];                               // rank(start)
    int64_t q = end;
    for (int64_t g = start; g < end && q == end; g += 16) {
        const JtkCpQuad quad = jtk_cp_load_quad(ix.text, g);
#pragma unroll
        for (int k4 = 0; k4 < 4; k4++) {                               // (unrolled: the words stay in registers)
            const int64_t w0 = g + 4 * k4;
            if (q != end || w0 >= end) continue;
            const int64_t left = end - w0;
            const uint32_t wc = jtk_cp_word_units(quad.w[k4], left >= 4 ? 4 : (int)left, ix.unit);
            if (run + wc <= T) { run += wc; continue; }
            for (int i = 0; i < 4 && w0 + i < end; i++) {
                const uint32_t w = jtk_cp_weight((uint8_t)(quad.w[k4] >> (8 * i)), ix.unit);
                if (run + w > T) { q = w0 + i; break; }
                run += w;
            }
        }
    }
    if (q < a) q = a;
    if (ix.unit == JTK_CP_UNIT_BYTE)                                      // every byte has a weight: back to the character's first byte
        while (q > a && q < e && jtk_cp_is_cont(ix.text[q])) q--;
    return q;
}

#endif
