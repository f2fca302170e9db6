// jtk_fim_rules.h -- the fill-in-the-middle transformation of a batch encode (JTK_ENCODE_FIM): the rule the device kernels
// (jtk_fim.hip) and the CPU test shim tests/fim_sim share.  Bavarian et al., "Efficient Training of Language Models to Fill
// in the Middle": a document is cut at two random positions of its TEXT into prefix, middle and suffix, the three parts are
// encoded separately (so the model sees tokens broken at the cuts), and they are emitted around three sentinel ids.
//
// The rule, per document d of `len` bytes, g = doc_index_base + d its index in the corpus:
//   mix(x)      the splitmix64 finaliser: x ^= x >> 30, x *= 0xBF58476D1CE4E5B9, x ^= x >> 27, x *= 0x94D049BB133111EB,
//               x ^= x >> 31.
//   draw(g, k)  = mix(mix(seed + 0x9E3779B97F4A7C15 * (g + 1)) + k), all modulo 2^64: counter-based and stateless, so a
//               document's outcome depends on (seed, g, its bytes) and never on the batch around it.
//   kind        0 (untouched) when len == 0; 0 when (draw(g, 0) >> 32) >= fim_rate and fim_rate != 0xFFFFFFFF; otherwise 2
//               (SPM) when (draw(g, 1) >> 32) < spm_rate or spm_rate == 0xFFFFFFFF; otherwise 1 (PSM).  The rates are in
//               units of 2^-32; 0xFFFFFFFF means always.
//   cuts        p_k = mulhi64(draw(g, 2 + k), len + 1), k = 0, 1: uniform over [0, len].  Each is then snapped to a character
//               start: while 0 < p < len, the byte at p is 0x80..0xBF and fewer than 3 steps have been taken, p -= 1.  The
//               result stands whatever byte it lands on (ill-formed text is encoded as the bytes it is).  a = min, b = max.
//   parts       prefix [0, a), middle [a, b), suffix [b, len): three sub-documents in text order, any of them may be empty.
//               For kind 0 they are [0, len), [len, len), [len, len): the whole document and two empty ones.
//   result      status = the lowest of the three parts' statuses; a document with status < 0 has no tokens.  Otherwise
//               kind 0: enc(document), exactly the call without the flag.
//               kind 1: PRE enc(prefix) SUF enc(suffix) MID enc(middle)                                   (PSM)
//               kind 2: PRE SUF enc(suffix) MID enc(prefix) enc(middle)                                   (SPM)
//               In both layouts the middle is the last part_tok[1] tokens of the document.
// Cutting by byte position and snapping makes a long character a slightly likelier cut point than a uniform draw over
// characters would.
#ifndef JTK_FIM_RULES_H
#define JTK_FIM_RULES_H

#include <stdint.h>

#include "jtk_device_prims.h"      // jtk_first_gt

#if defined(__HIPCC__) || defined(__HIP__)
#define JTK_FIM_HD __host__ __device__ inline
#else
#define JTK_FIM_HD inline
#endif

#define JTK_FIM_ALWAYS 0xFFFFFFFFu
#define JTK_FIM_NONE 0        // kind
#define JTK_FIM_PSM 1
#define JTK_FIM_SPM 2
#define JTK_FIM_PRE (-1)      // jtk_fim_cell: the cell holds a sentinel
#define JTK_FIM_MID (-2)
#define JTK_FIM_SUF (-3)
#define JTK_FIM_TILE 1024     // output cells per workgroup step of the gather (256 lanes x 4)

JTK_FIM_HD uint64_t jtk_fim_mix(uint64_t x) {
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27; x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x;
}

// the per-document key of the draws
JTK_FIM_HD uint64_t jtk_fim_key(uint64_t seed, int64_t g) { return jtk_fim_mix(seed + 0x9E3779B97F4A7C15ull * ((uint64_t)g + 1ull)); }
JTK_FIM_HD uint64_t jtk_fim_draw(uint64_t key, uint64_t k) { return jtk_fim_mix(key + k); }

JTK_FIM_HD uint64_t jtk_fim_mulhi(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return (uint64_t)(((unsigned __int128)a * (unsigned __int128)b) >> 64);
#endif
}

JTK_FIM_HD int jtk_fim_kind(uint64_t key, int64_t len, uint32_t fim_rate, uint32_t spm_rate) {
    if (len == 0) return JTK_FIM_NONE;
    if (fim_rate != JTK_FIM_ALWAYS && (uint32_t)(jtk_fim_draw(key, 0) >> 32) >= fim_rate) return JTK_FIM_NONE;
    if (spm_rate == JTK_FIM_ALWAYS || (uint32_t)(jtk_fim_draw(key, 1) >> 32) < spm_rate) return JTK_FIM_SPM;
    return JTK_FIM_PSM;
}

// cut k (0 or 1) of a document of len bytes, snapped; at(i) = byte i of the document, asked only for 0 < i < len
template <class At>
JTK_FIM_HD int64_t jtk_fim_cut(uint64_t key, int k, int64_t len, At at) {
    int64_t p = (int64_t)jtk_fim_mulhi(jtk_fim_draw(key, 2u + (uint64_t)k), (uint64_t)len + 1ull);
    for (int step = 0; step < 3 && p < len && p > 0 && (at(p) & 0xC0u) == 0x80u; step++) p--;
    return p;
}

// kind and cuts [a, b] of one document
template <class At>
JTK_FIM_HD int jtk_fim_doc(uint64_t seed, int64_t g, int64_t len, uint32_t fim_rate, uint32_t spm_rate, At at, int64_t* a, int64_t* b) {
    const uint64_t key = jtk_fim_key(seed, g);
    const int kind = jtk_fim_kind(key, len, fim_rate, spm_rate);
    if (kind == JTK_FIM_NONE) { *a = len; *b = len; return kind; }
    const int64_t p0 = jtk_fim_cut(key, 0, len, at), p1 = jtk_fim_cut(key, 1, len, at);
    *a = p0 < p1 ? p0 : p1;
    *b = p0 < p1 ? p1 : p0;
    return kind;
}

// ---- per offset / per document, as the kernels take them (one lane each)
// entry d (0 <= d <= n_docs) of the caller's offsets breaks the rule: non-decreasing within [0, n_bytes], from 0 to n_bytes
JTK_FIM_HD bool jtk_fim_offset_bad(const int64_t* doc_off, int64_t n_docs, int64_t n_bytes, int64_t d) {
    const int64_t q = doc_off[d];
    return q < 0 || q > n_bytes || (d > 0 && doc_off[d - 1] > q) || (d == 0 && q != 0) || (d == n_docs && q != n_bytes);
}

// kind[d], cut[d][2] and sub_off[3d .. 3d + 2] of document d < n_docs (sub_off[3 n_docs] = doc_off[n_docs] is the caller's).
// Reads the draws and up to 6 bytes of text.  A document whose own range is not inside [0, n_bytes] stays whole and its text
// is not read: the sub-documents then break the rule where the documents do, and the pipeline reports them as it always does.
JTK_FIM_HD void jtk_fim_cuts_doc(const uint8_t* text, const int64_t* doc_off, int64_t n_bytes, int64_t d, uint64_t seed, int64_t doc_index_base,
                                 uint32_t fim_rate, uint32_t spm_rate, uint8_t* kind, int64_t* cut, int64_t* sub_off) {
    const int64_t q = doc_off[d], end = doc_off[d + 1];
    int64_t a = end - q, b = end - q;
    int k = JTK_FIM_NONE;
    if (q >= 0 && q <= end && end <= n_bytes) {
        const uint8_t* doc = text + q;
        k = jtk_fim_doc(seed, doc_index_base + d, end - q, fim_rate, spm_rate, [&](int64_t i) -> uint32_t { return doc[i]; }, &a, &b);
    }
    kind[d] = (uint8_t)k;
    cut[2 * d] = a;
    cut[2 * d + 1] = b;
    sub_off[3 * d] = q;
    sub_off[3 * d + 1] = q + a;
    sub_off[3 * d + 2] = q + b;
}

// status[d] (the lowest of the three parts') and part_tok[d][3] of document d from the sub-documents' result; returns its tokens
// in the final result.  bad: the batch's offsets broke the rule -- then nothing of the sub-documents' result is followed.
JTK_FIM_HD int64_t jtk_fim_count_doc(int64_t d, bool bad, const uint8_t* kind, const int64_t* sub_tok_off, const int32_t* sub_status,
                                     int32_t* status, int64_t* part_tok) {
    int32_t st = 0;
    int64_t c[3];
    for (int k = 0; k < 3; k++) {
        const int32_t s = sub_status[3 * d + k];
        st = s < st ? s : st;
        c[k] = sub_tok_off[3 * d + k + 1] - sub_tok_off[3 * d + k];
    }
    if (st < 0 || bad) c[0] = c[1] = c[2] = 0;
    status[d] = st;
    part_tok[3 * d] = c[0];
    part_tok[3 * d + 1] = c[1];
    part_tok[3 * d + 2] = c[2];
    return (bad || st < 0) ? 0 : c[0] + c[1] + c[2] + (kind[d] != JTK_FIM_NONE ? 3 : 0);
}

// Cell o (0 <= o < the document's tokens, jtk_fim_count_doc) of a document's result: the part it is copied from (0 prefix, 1 middle, 2 suffix; *idx =
// the token's index inside that part) or the sentinel it holds (JTK_FIM_PRE / _MID / _SUF).
JTK_FIM_HD int jtk_fim_cell(int kind, int64_t c0, int64_t c1, int64_t c2, int64_t o, int64_t* idx) {
    *idx = 0;
    if (kind == JTK_FIM_NONE) {                       // (the whole document is part 0; the other two are empty)
        if (o < c0) { *idx = o; return 0; }
        o -= c0;
        if (o < c1) { *idx = o; return 1; }
        *idx = o - c1;
        return 2;
    }
    if (o == 0) return JTK_FIM_PRE;
    o -= 1;
    if (kind == JTK_FIM_PSM) {
        if (o < c0) { *idx = o; return 0; }
        o -= c0;
        if (o == 0) return JTK_FIM_SUF;
        o -= 1;
        if (o < c2) { *idx = o; return 2; }
        o -= c2;
        if (o == 0) return JTK_FIM_MID;
        *idx = o - 1;
        return 1;
    }
    if (o == 0) return JTK_FIM_SUF;
    o -= 1;
    if (o < c2) { *idx = o; return 2; }
    o -= c2;
    if (o == 0) return JTK_FIM_MID;
    o -= 1;
    if (o < c0) { *idx = o; return 0; }
    *idx = o - c0;
    return 1;
}

// ---- the stitch, as the gather walks it.  The result's cells are taken in tiles of JTK_FIM_TILE, four consecutive cells per
// lane; a lane finds the document of its first cell by one search over tok_off, from its cursor on, and then moves forward.
struct JtkFimView {
    int64_t n_docs;
    const uint8_t* kind;          // [n_docs]
    const int64_t* part_tok;      // [n_docs][3] tokens of prefix, middle, suffix
    const int64_t* tok_off;       // [n_docs + 1] of the result
    const int64_t* sub_tok_off;   // [3 n_docs + 1] of the sub-documents' encode: sub-document 3d + k is part k of document d in
    const int32_t* sub_tokens;    //                text order (prefix, middle, suffix)
    int32_t prefix_id, middle_id, suffix_id;
};

// The cells e0 .. e0 + 3 below total = tok_off[n_docs] (e0 < total): their ids into id[]; returns how many there are.  *d is
// the lane's cursor: a document with tok_off[*d] <= e0 (0 at first), left at the document of the last cell.
JTK_FIM_HD int jtk_fim_cells4(const JtkFimView& v, int64_t e0, int64_t total, int64_t* d_io, int32_t* id) {
    // the document that holds e0: the one before the first k with tok_off[k] > e0 (tok_off[n_docs] = total > e0); it has tokens
    int64_t d = jtk_first_gt(v.tok_off, *d_io, v.n_docs + 1, e0) - 1;
    int64_t loaded = -1, base = 0, c0 = 0, c1 = 0, c2 = 0;
    int kind = 0, n = 0;
    for (int j = 0; j < 4 && e0 + j < total; j++, n++) {
        const int64_t e = e0 + j;
        while (v.tok_off[d + 1] <= e) d++;           // (documents without tokens are passed over)
        if (d != loaded) {
            loaded = d; base = v.tok_off[d]; kind = v.kind[d];
            c0 = v.part_tok[3 * d]; c1 = v.part_tok[3 * d + 1]; c2 = v.part_tok[3 * d + 2];
        }
        int64_t idx;
        const int part = jtk_fim_cell(kind, c0, c1, c2, e - base, &idx);
        id[j] = part == JTK_FIM_PRE ? v.prefix_id : part == JTK_FIM_MID ? v.middle_id : part == JTK_FIM_SUF ? v.suffix_id
                                    : v.sub_tokens[v.sub_tok_off[3 * d + part] + idx];
    }
    *d_io = d;
    return n;
}

#endif  // JTK_FIM_RULES_H
