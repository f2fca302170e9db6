// jtk_maxtok_rules.h -- the rules of Encoding.encode(text, maxTokens) (GptBytePairEncoding.java:43-45, 79-100) that the host
// and the device share: the early exit of the batch entry points (when the tokens of a document's leading bytes are certain
// to be the head of its full token list) and the back-off to a code-point boundary.  jtk_abi.cpp (host), jtk_decode.hip
// (k_truncate), jtk_maxtok.hip (the device early exit) and the CPU test shim tests/maxtok_sim include it.
#ifndef JTK_MAXTOK_RULES_H
#define JTK_MAXTOK_RULES_H

#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define JTK_MT_HD __host__ __device__ inline
#else
#define JTK_MT_HD inline
#endif

// A safe piece start lies at least this many bytes before the cut: every look-ahead of the patterns (a contraction, the
// character after a white-space run) is shorter.
#define JTK_MAXTOK_MARGIN 16

// Leading bytes encoded in the first round: 8 per wanted token + 64; each later round takes 4x more.
JTK_MT_HD int64_t jtk_maxtok_first_prefix(int64_t max_tokens) {
    return max_tokens > ((int64_t)1 << 40) ? (int64_t)1 << 44 : 8 * max_tokens + 64;
}
JTK_MT_HD int64_t jtk_maxtok_next_prefix(int64_t P) { return P > ((int64_t)1 << 40) ? P : P * 4; }
// The bytes of a document of `len` bytes that a round with prefix size P encodes; past one chunk (`cb`) it goes whole.
JTK_MT_HD int64_t jtk_maxtok_prefix_bytes(int64_t len, int64_t P, int64_t cb) {
    const int64_t p = len < P ? len : P;
    return p > cb ? len : p;
}

// A byte that may begin a white-space character: the ASCII ones, and the lead bytes of U+0085/U+00A0 (C2), U+1680 (E1),
// U+2000..U+205F (E2) and U+3000 (E3).  Conservative on purpose: it only ever makes the early exit look further.
JTK_MT_HD bool jtk_maybe_space(uint8_t c) {
    return (c >= 0x09 && c <= 0x0D) || c == 0x20 || c == 0xC2 || c == 0xE1 || c == 0xE2 || c == 0xE3;
}

// A piece start q (text[q] = c0, text[q + 1] = c1) that does not sit inside a white-space run that might reach the cut
// (`\s*[\r\n]+` and `\s+(?!\S)` look to the END of the run): c0 is no white space, or one ASCII white-space character
// followed by something else.
JTK_MT_HD bool jtk_maxtok_safe_start(uint8_t c0, uint8_t c1) {
    return !jtk_maybe_space(c0) || (c0 < 0x80 && !jtk_maybe_space(c1));
}

// The last safe piece start q of a prefix of p bytes: 0 < q <= p - JTK_MAXTOK_MARGIN (0: none).  mask bit (base + i) is set
// when a piece starts at prefix byte i; t = the prefix.
JTK_MT_HD int64_t jtk_maxtok_last_safe_start(const uint64_t* mask, int64_t base, const uint8_t* t, int64_t p) {
    for (int64_t pos = base + p - JTK_MAXTOK_MARGIN; pos > base;) {
        uint64_t w = mask[pos >> 6];
        const int sh = (int)(pos & 63);
        w = sh == 63 ? w : (w & ((2ull << sh) - 1));                 // bits 0..sh
        const int64_t wbase = pos & ~(int64_t)63;
        while (w) {
            const int bit = 63 - __builtin_clzll(w);
            const int64_t cand = wbase + bit;
            if (cand <= base) return 0;
            if (jtk_maxtok_safe_start(t[cand - base], t[cand - base + 1])) return cand - base;
            w &= ~(1ull << bit);
        }
        pos = wbase - 1;
    }
    return 0;
}

// The prefix decides the document when it holds at least max_tokens tokens and the first max_tokens of them (sum_bytes
// bytes) all end at or before the last safe piece start q: pieces before q are matched exactly as in the whole text and
// pieces encode independently.
JTK_MT_HD bool jtk_maxtok_decided(int64_t n_tokens, int64_t max_tokens, int64_t sum_bytes, int64_t q) {
    return q > 0 && n_tokens >= max_tokens && sum_bytes <= q;
}

// The back-off of GptBytePairEncoding.java:90-100: drop trailing tokens until decode(tokens) -- the byte prefix [0, nb) of
// the text -- is a prefix of the text as a String: nb is a code-point boundary, or the cut character decodes to one U+FFFD
// and the text has U+FFFD there.  keep tokens of nb bytes to start with; tok_len(k) = byte length of token k.
// Result: kept count; if `ok`, the text from `from` on holds what the decoded text lacks, of which `units` UTF-16 units
// are common to both (0 at a boundary, 1 for the U+FFFD).
struct JtkBackoff {
    int64_t keep;
    int64_t from;
    int units;
    bool ok;
};
template <class TokLen>
JTK_MT_HD JtkBackoff jtk_maxtok_backoff(const uint8_t* tx, int64_t len, int64_t keep, int64_t nb, TokLen tok_len) {
    for (;; keep--) {
        if (nb == len || (tx[nb] & 0xC0) != 0x80) return JtkBackoff{keep, nb, 0, true};
        int64_t c = nb;
        while (c > 0 && (tx[c] & 0xC0) == 0x80) c--;
        if (c + 2 < len && tx[c] == 0xEF && tx[c + 1] == 0xBF && tx[c + 2] == 0xBD) return JtkBackoff{keep, c, 1, true};
        if (keep == 0) return JtkBackoff{0, 0, 0, false};
        nb -= tok_len(keep - 1);
    }
}

// Does tx[from, end) hold more than k UTF-16 units?  (Looks at the first few characters only: the document may be long.)
JTK_MT_HD bool jtk_more_units_than(const uint8_t* tx, int64_t from, int64_t end, int64_t k) {
    int64_t u = 0;
    for (int64_t i = from; i < end; i++)
        if ((tx[i] & 0xC0) != 0x80) { u += (tx[i] >= 0xF0) ? 2 : 1; if (u > k) return true; }
    return false;
}

#endif
