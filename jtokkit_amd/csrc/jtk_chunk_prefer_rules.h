// jtk_chunk_prefer_rules.h -- token-budget chunks that end at paragraph, line, sentence and word boundaries
// (jtk_batch_chunk_prefer): the rule the device kernels (jtk_chunk_prefer.hip) and the CPU test shim tests/chunk_prefer_sim
// share.  It extends jtk_chunk_rules.h: the same documents, the same B(i), the same back-off when no boundary is found.
//
// A document has tokens t_0 .. t_{n-1}.  D is the concatenation of their byte strings as jtk_decode gives them (a special id
// contributes its literal): the text, except after jtk_batch_encode_pieces.  p_i is the start of token i in D.  For
// 0 < i < n: y = D[p_i] and x(k) = D[p_i - k] for k = 1..3, "none" (-1) when p_i - k < 0 -- the lookback never leaves the
// document.  ws = {0x20, 0x09 .. 0x0D}.
//
// level(i) for 0 < i < n is 0 (SPLIT) if !B(i); else the highest class below that holds and is enabled in the mask `prefer`,
// or 1 (CHAR) if none does:
//   2 WORD       JTK_CUT_WORD       y in ws or x(1) in ws
//   3 SENTENCE   JTK_CUT_SENTENCE   (x(1) in {. ! ?} and y in ws) or (x(1) in ws and x(2) in {. ! ?}) or
//                                   x(3) x(2) x(1) in {E3 80 82, EF BC 81, EF BC 9F}  (the ideographic full stop, fullwidth ! ?)
//   4 LINE       JTK_CUT_LINE       x(1) = \n and y not in {\n, \r}
//   5 PARAGRAPH  JTK_CUT_PARAGRAPH  LINE holds and (x(2) = \n or (x(2) = \r and x(3) = \n))
// Level 6 (DOC_END) is the document's edge: i = 0 and i = n.
//
// With N = chunk_tokens, 0 <= overlap < N and 1 <= min_tokens <= N:
//
//   s = 0
//   while s < n:
//       hi = min(s + N, n)
//       if hi == n: e = n, end_level = 6
//       else:
//           lo = min(s + min_tokens, hi)
//           m  = max level(i), i in [lo, hi]
//           e  = the largest i in [lo, hi] with level(i) == m       if m >= 1
//                jtk_chunk_end(s, n, N, B)                          if m == 0   (the back-off of jtk_chunk_rules.h)
//           end_level = level(e)
//       emit (s, e, split = !(B(s) && B(e)), end_level)
//       if e == n: break
//       R = [max(e - overlap, s + 1), e)
//       m = max level(i), i in R   (0 for an empty R)
//       s = the smallest i in R with level(i) == m  if m >= 1, else e
//
// With prefer == 0 and min_tokens == 1 this is jtk_chunk_walk cut for cut.  Chunks stay exact slices of encode(doc), have at
// most N tokens, always make progress, and with overlap 0 concatenate to encode(doc).
#ifndef JTK_CHUNK_PREFER_RULES_H
#define JTK_CHUNK_PREFER_RULES_H

#include "../../include/jtokkit_amd.h"
#include "jtk_chunk_rules.h"

JTK_CK_HD bool jtk_cut_ws(int c) { return c == 0x20 || (c >= 0x09 && c <= 0x0D); }
JTK_CK_HD bool jtk_cut_stop(int c) { return c == '.' || c == '!' || c == '?'; }

// level(i) from the bytes around the cut: y = D[p_i], x1..x3 = D[p_i - 1 .. p_i - 3] (-1: none).
JTK_CK_HD int jtk_cut_level(uint32_t prefer, int y, int x1, int x2, int x3) {
    if ((y & 0xC0) == 0x80) return JTK_LEVEL_SPLIT;
    const bool line = x1 == '\n' && y != '\n' && y != '\r';
    if ((prefer & JTK_CUT_PARAGRAPH) && line && (x2 == '\n' || (x2 == '\r' && x3 == '\n'))) return JTK_LEVEL_PARAGRAPH;
    if ((prefer & JTK_CUT_LINE) && line) return JTK_LEVEL_LINE;
    if (prefer & JTK_CUT_SENTENCE) {
        if ((jtk_cut_stop(x1) && jtk_cut_ws(y)) || (jtk_cut_ws(x1) && jtk_cut_stop(x2))) return JTK_LEVEL_SENTENCE;
        if ((x3 == 0xE3 && x2 == 0x80 && x1 == 0x82) || (x3 == 0xEF && x2 == 0xBC && (x1 == 0x81 || x1 == 0x9F)))
            return JTK_LEVEL_SENTENCE;
    }
    if ((prefer & JTK_CUT_WORD) && (jtk_cut_ws(y) || jtk_cut_ws(x1))) return JTK_LEVEL_WORD;
    return JTK_LEVEL_CHAR;
}

// The highest level that `prefer` can give: a window search may stop once it has seen it.
JTK_CK_HD int jtk_cut_top_level(uint32_t prefer) {
    return (prefer & JTK_CUT_PARAGRAPH) ? JTK_LEVEL_PARAGRAPH : (prefer & JTK_CUT_LINE) ? JTK_LEVEL_LINE
         : (prefer & JTK_CUT_SENTENCE) ? JTK_LEVEL_SENTENCE : (prefer & JTK_CUT_WORD) ? JTK_LEVEL_WORD : JTK_LEVEL_CHAR;
}

// The maximum of lvl over the cuts [a, b) and, in *at, the last (last = true) or first cut that has it; 0 and *at untouched
// for an empty range or when every cut is SPLIT.  This is the "window search" of the walk: the kernels bring their own (word
// by word in one lane, a reduction in a workgroup) and must agree with it.
template <class Lvl>
JTK_CK_HD int jtk_cut_scan(int64_t a, int64_t b, bool last, Lvl lvl, int64_t* at) {
    int m = 0;
    if (last) {
        for (int64_t i = b - 1; i >= a; i--) { const int l = lvl(i); if (l > m) { m = l; *at = i; } }
    } else {
        for (int64_t i = a; i < b; i++) { const int l = lvl(i); if (l > m) { m = l; *at = i; } }
    }
    return m;
}

// The end of the chunk that starts at s, s + N < n: `lvl(i)` is asked only for 0 < i < n; win(a, b, last, at) is jtk_cut_scan.
template <class Lvl, class Win>
JTK_CK_HD int64_t jtk_chunk_prefer_end(int64_t s, int64_t n, int64_t N, int64_t min_tokens, Lvl lvl, Win win) {
    const int64_t hi = s + N, lo = (min_tokens < N) ? s + min_tokens : hi;
    int64_t e = hi;
    if (win(lo, hi + 1, true, &e) >= 1) return e;
    return jtk_chunk_end(s, n, N, [&](int64_t i) { return lvl(i) != 0; });
}

// The start of the chunk after (s, e), e < n.
template <class Win>
JTK_CK_HD int64_t jtk_chunk_prefer_next_start(int64_t s, int64_t e, int64_t overlap, Win win) {
    int64_t r = e;
    win((e - overlap > s + 1) ? e - overlap : s + 1, e, false, &r);
    return r;
}

// The whole rule for one document: emit(k, s, e, split, end_level) for every chunk k; returns the chunk count (0 for n == 0).
template <class Lvl, class Win, class Emit>
JTK_CK_HD int64_t jtk_chunk_prefer_walk(int64_t n, int64_t N, int64_t overlap, int64_t min_tokens, Lvl lvl, Win win, Emit emit) {
    auto b = [&](int64_t i) { return i <= 0 || i >= n || lvl(i) != 0; };
    int64_t k = 0;
    for (int64_t s = 0; s < n; k++) {
        const bool last = n - s <= N;
        const int64_t e = last ? n : jtk_chunk_prefer_end(s, n, N, min_tokens, lvl, win);
        emit(k, s, e, !(b(s) && b(e)), last ? (int)JTK_LEVEL_DOC_END : lvl(e));
        if (last) { k++; break; }
        s = jtk_chunk_prefer_next_start(s, e, overlap, win);
    }
    return k;
}
// ... with the plain window search
template <class Lvl, class Emit>
JTK_CK_HD int64_t jtk_chunk_prefer_walk(int64_t n, int64_t N, int64_t overlap, int64_t min_tokens, Lvl lvl, Emit emit) {
    return jtk_chunk_prefer_walk(n, N, overlap, min_tokens, lvl,
                                 [&](int64_t a, int64_t b, bool last, int64_t* at) { return jtk_cut_scan(a, b, last, lvl, at); }, emit);
}

#endif
