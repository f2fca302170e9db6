// jtk_chunk_rules.h -- token-budget chunking of a document's token list (jtk_batch_chunk): the rule the device kernels
// (jtk_chunk.hip) and the CPU test shim tests/chunk_sim share.
//
// A document has tokens t_0 .. t_{n-1}: exactly what the batch encode produced for it.  B(i), "a character boundary before
// token i", is true for i = 0 and i = n, and otherwise when the first byte of t_i's byte string is not a UTF-8 continuation
// byte (10xxxxxx) -- the same question as whether the text byte at that cut is one, since the tokens decode to the text.
// With a chunk size N >= 1 and an overlap 0 <= overlap < N:
//
//   s = 0
//   while s < n:
//       e = jtk_chunk_end(s, n, N, B)                 largest i in (s, min(s + N, n)] with B(i), or min(s + N, n)
//       emit (s, e, split = !(B(s) && B(e)))          split: the chunk starts or ends inside a character
//       if e == n: break
//       s = jtk_chunk_next_start(s, e, overlap, n, B) e, or with overlap the smallest i in [max(e - overlap, s + 1), e]
//                                                     with B(i) (e if none)
//
// The back-off at a cut is the one of GptBytePairEncoding.java:90-100 (drop trailing tokens until the bytes end on a
// code-point boundary), except that a cut inside a U+FFFD of the text is not accepted: every chunk must stand alone as
// text.  The chunks are exact slices of encode(doc) -- NOT the result of repeated encode(rest, N) calls on the remaining
// text --: they cost one encode plus one pass and do not depend on where the text was cut.  Every chunk has at most N
// tokens, progress is guaranteed (e > s), and with overlap 0 the chunks concatenate to encode(doc).
#ifndef JTK_CHUNK_RULES_H
#define JTK_CHUNK_RULES_H

#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define JTK_CK_HD __host__ __device__ inline
#else
#define JTK_CK_HD inline
#endif

// B(i) with the two ends of the document: `bnd(i)` is asked only for 0 < i < n.
template <class Bnd>
JTK_CK_HD bool jtk_chunk_b(int64_t i, int64_t n, Bnd bnd) {
    return i <= 0 || i >= n || bnd(i);
}

// The end of the chunk that starts at s.
template <class Bnd>
JTK_CK_HD int64_t jtk_chunk_end(int64_t s, int64_t n, int64_t N, Bnd bnd) {
    const int64_t hi = (n - s < N) ? n : s + N;
    for (int64_t i = hi; i > s; i--)
        if (jtk_chunk_b(i, n, bnd)) return i;
    return hi;
}

// The start of the chunk after (s, e), e < n.
template <class Bnd>
JTK_CK_HD int64_t jtk_chunk_next_start(int64_t s, int64_t e, int64_t overlap, int64_t n, Bnd bnd) {
    if (overlap == 0) return e;
    for (int64_t i = (e - overlap > s + 1) ? e - overlap : s + 1; i < e; i++)
        if (jtk_chunk_b(i, n, bnd)) return i;
    return e;
}

template <class Bnd>
JTK_CK_HD bool jtk_chunk_split(int64_t s, int64_t e, int64_t n, Bnd bnd) {
    return !(jtk_chunk_b(s, n, bnd) && jtk_chunk_b(e, n, bnd));
}

// The whole rule for one document: emit(k, s, e, split) for every chunk k; returns the chunk count (0 for n == 0).
template <class Bnd, class Emit>
JTK_CK_HD int64_t jtk_chunk_walk(int64_t n, int64_t N, int64_t overlap, Bnd bnd, Emit emit) {
    int64_t k = 0;
    for (int64_t s = 0; s < n; k++) {
        const int64_t e = jtk_chunk_end(s, n, N, bnd);
        emit(k, s, e, jtk_chunk_split(s, e, n, bnd));
        if (e == n) { k++; break; }
        s = jtk_chunk_next_start(s, e, overlap, n, bnd);
    }
    return k;
}

#endif
