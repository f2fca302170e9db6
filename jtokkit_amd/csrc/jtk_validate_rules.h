// jtk_validate_rules.h -- JTK_ENCODE_VALIDATE_UTF8: the per-byte rule that the device kernel (k_validate_utf8, jtk_kernels.hip) and
// the CPU test shim tests/validate_sim share.  A document is well-formed when it is what String.getBytes(UTF_8) can produce:
// the sequences of Unicode Table 3-7 -- a lead C2..DF and one continuation byte (80..BF); E0 A0..BF, E1..EC 80..BF, ED 80..9F,
// EE..EF 80..BF and one more continuation byte; F0 90..BF, F1..F3 80..BF, F4 80..8F and two more -- so shortest form, no
// surrogates, nothing above U+10FFFF, and no sequence cut by the document's end.  C0, C1 and F5..FF are never leads.
//
// The rule is a function of ONE position p and a bounded window around it (3 bytes back, 3 ahead), so that one lane per byte
// can judge it: a document is malformed exactly when some byte of it is bad.
//   a byte below 80               never bad
//   a lead byte (C0..FF)          bad when it is no lead of the table, when one of the len - 1 bytes after it is no continuation
//                                 byte or lies in another document (or past the end), or when its second byte is outside the
//                                 table's range for this lead
//   a continuation byte (80..BF)  bad unless the nearest byte before it that is no continuation byte lies at most
//                                 JTK_UTF8_MAX_BACK back IN THE SAME DOCUMENT, is a lead of the table, and leads a sequence long
//                                 enough to cover p.  (Whether that sequence is well-formed is the lead's own verdict.)
// at(q): the byte at q, 0 outside the text.  ds(q): a document starts at q, or q is at or past the end of the text.  Empty
// documents own no byte and are never flagged; the caller maps a bad byte to the non-empty document that holds it.
#ifndef JTK_VALIDATE_RULES_H
#define JTK_VALIDATE_RULES_H

#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define JTK_V8_HD __host__ __device__ inline
#else
#define JTK_V8_HD inline
#endif

#define JTK_UTF8_LEAD_MIN 0xC2u          // C0, C1: overlong forms of ASCII
#define JTK_UTF8_LEAD_MAX 0xF4u          // F5..FF: above U+10FFFF, or no UTF-8 at all
#define JTK_UTF8_E0_C1_MIN 0xA0u         // E0 80..9F: overlong
#define JTK_UTF8_ED_C1_MAX 0x9Fu         // ED A0..BF: surrogates
#define JTK_UTF8_F0_C1_MIN 0x90u         // F0 80..8F: overlong
#define JTK_UTF8_F4_C1_MAX 0x8Fu         // F4 90..BF: above U+10FFFF
#define JTK_UTF8_MAX_BACK 3              // a continuation byte's lead is at most this far back

JTK_V8_HD bool jtk_utf8_is_cont(uint32_t c) { return (c & 0xC0u) == 0x80u; }

// the length of the sequence that the byte c (no continuation byte, >= 0x80) leads; 0: it leads none
JTK_V8_HD int jtk_utf8_lead_len(uint32_t c) {
    if (c < JTK_UTF8_LEAD_MIN || c > JTK_UTF8_LEAD_MAX) return 0;
    return c >= 0xF0u ? 4 : (c >= 0xE0u ? 3 : 2);
}

template <class At, class Ds>
JTK_V8_HD bool jtk_utf8_byte_bad(int64_t p, At at, Ds ds) {
    const uint32_t b = at(p);
    if (b < 0x80u) return false;
    if (jtk_utf8_is_cont(b)) {
        // find the lead (at most JTK_UTF8_MAX_BACK back, same document) and check it is long enough to cover this byte
        int64_t q = p;
        for (int k = 1; k <= JTK_UTF8_MAX_BACK; k++) {
            if (ds(q)) return true;                 // p..q start a document: no lead before them
            q--;
            const uint32_t c = at(q);
            if (jtk_utf8_is_cont(c)) continue;
            return !(jtk_utf8_lead_len(c) > k);
        }
        return true;
    }
    const int len = jtk_utf8_lead_len(b);
    if (len == 0) return true;
    for (int k = 1; k < len; k++)
        if (ds(p + k) || !jtk_utf8_is_cont(at(p + k))) return true;
    const uint32_t c1 = at(p + 1);
    if (b == 0xE0u && c1 < JTK_UTF8_E0_C1_MIN) return true;          // overlong
    if (b == 0xEDu && c1 > JTK_UTF8_ED_C1_MAX) return true;          // surrogates
    if (b == 0xF0u && c1 < JTK_UTF8_F0_C1_MIN) return true;          // overlong
    if (b == 0xF4u && c1 > JTK_UTF8_F4_C1_MAX) return true;          // > U+10FFFF
    return false;
}

#endif
