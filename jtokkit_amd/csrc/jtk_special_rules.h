// jtk_special_rules.h -- which special-token literals an allow-special encode (JTK_ENCODE_ALLOW_SPECIAL) takes as ids.
// Shared by the kernels of jtk_special.hip and the CPU shim of the test tier (tests/special_sim), so that both run the same
// rule.
//
// The rule (tiktoken's encode(doc, allowed_special=A), with leftmost-longest as the tie-break): scan from the document's
// start; the next match is the leftmost position where some allowed literal occurs entirely inside the document, and of the
// literals that match there the longest; scanning resumes after it, so matches never overlap.
//
// Candidates: per position p, the longest allowed literal that matches at p and ends inside the document
// (jtk_special_scan_at).  In position order, the greedy scan keeps the first candidate, then every candidate that starts at or
// after the end of the last one kept.  In parallel: candidate i is kept for certain when no earlier candidate ends after its
// start (its start is at or past the prefix maximum of the earlier ends, which bounds the greedy frontier); only candidates
// that start fewer than maxlen bytes before it can end after it (jtk_special_certain).  The candidates between two certain
// ones overlap some earlier candidate -- chains, which need self-overlapping literals such as aa / aaa -- and are decided by
// the greedy walk from the certain one before them (jtk_special_walk).  A document's first candidate is always certain, and a
// chain never leaves its document (literals end inside their document).
#ifndef JTK_SPECIAL_RULES_H
#define JTK_SPECIAL_RULES_H

#include <stdint.h>

#if defined(__HIPCC__)
#define JTK_SR_FN __host__ __device__ inline
#else
#define JTK_SR_FN inline
#endif

// The literals matching at p that end at or before `end`: *best_len / *best_idx = the longest allowed one (0 / -1: none);
// returns whether some literal that is NOT allowed matches there.  Literal i is blob[off[i], off[i + 1]); at(q) = text byte q.
template <class At>
JTK_SR_FN bool jtk_special_scan_at(int64_t p, int64_t end, At at, int n_lits, const uint32_t* off, const uint8_t* blob,
                                   const uint8_t* allowed, int* best_len, int* best_idx) {
    bool disallowed = false;
    *best_len = 0;
    *best_idx = -1;
    const uint32_t b0 = at(p);
    for (int i = 0; i < n_lits; i++) {
        const uint32_t o = off[i];
        const int len = (int)(off[i + 1] - o);
        if (len < 1 || p + len > end || blob[o] != b0) continue;
        bool eq = true;
        for (int j = 1; j < len && eq; j++) eq = at(p + j) == blob[o + j];
        if (!eq) continue;
        if (!allowed[i]) disallowed = true;
        else if (len > *best_len) { *best_len = len; *best_idx = i; }
    }
    return disallowed;
}

// Candidate i (candidates in position order: start s(i), end e(i)) is kept for certain: no earlier candidate ends after its
// start.  maxlen: the longest allowed literal.
template <class S, class E>
JTK_SR_FN bool jtk_special_certain(int64_t i, int64_t maxlen, S s, E e) {
    const int64_t p = s(i);
    for (int64_t j = i - 1; j >= 0 && s(j) > p - maxlen; j--)
        if (e(j) > p) return false;
    return true;
}

// The greedy walk from the certain candidate i (kept) over the candidates after it up to the next certain one (or n):
// keep(j, kept) for each.
template <class S, class E, class C, class K>
JTK_SR_FN void jtk_special_walk(int64_t i, int64_t n, S s, E e, C certain, K keep) {
    int64_t frontier = e(i);
    for (int64_t j = i + 1; j < n && !certain(j); j++) {
        const bool k = s(j) >= frontier;
        if (k) frontier = e(j);
        keep(j, k);
    }
}

#endif
