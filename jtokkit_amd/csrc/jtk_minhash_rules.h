// jtk_minhash_rules.h -- MinHash signatures and LSH band keys over the token n-grams of a batch encode (jtk_batch_minhash,
// jtk_batch_minhash_agree): the rule the device kernels (jtk_minhash.hip) and the CPU test shim tests/minhash_sim share.
// Broder, "On the resemblance and containment of documents"; the way GPT-3, the Pile and RefinedWeb deduplicate: the
// fraction of hash functions under which two documents have the same minimum estimates the Jaccard similarity of their
// shingle sets, and documents that agree on a whole band of r minima are candidates.
//
// The rule, all arithmetic modulo 2^64 unless stated; G = 0x9E3779B97F4A7C15, mix = the splitmix64 finaliser (jtk_fim_mix):
//   key         = mix(seed + G * (n + 1)), n = ngram; draw(j) = mix(key + j).
//   shingles    of a document of l tokens t[0 .. l) (the int32 ids of the encode: special ids, FIM sentinels and pseudo ids
//               count as ids): none when l == 0 (a document with status < 0 has l = 0); otherwise m = min(n, l) and shingle i
//               is t[i .. i + m), 0 <= i <= l - m.  A document shorter than n is one shingle of all its tokens.
//               n_shingles = l - m + 1, or 0.
//   H_i         = sum over j < m of ((uint32)t[i + j] + 1) * G^(m - 1 - j): Horner, H = H * G + id + 1.
//   x_i         = the low 32 bits of mix(H_i ^ key).
//   a_k, b_k    = draw(2k + 1) | 1, draw(2k + 2), k < K = num_hashes.
//   sig[k]      = min over i of ((a_k * x_i + b_k) mod 2^64) >> 32: the multiply-add-shift family, strongly universal on
//               32-bit keys; 0xFFFFFFFF with no shingles.
//   band_key[j] = h after h = draw(2^32 + j), then h = mix(h ^ v) for v = sig[j r .. j r + r - 1] in order; r = K / bands.
//   agree(a, b) = the number of k with sig[a][k] == sig[b][k]; agree / K estimates the Jaccard similarity.
// A signature depends on (seed, ngram, num_hashes, the document's ids) alone: shards of a corpus, batches and devices agree
// by construction.
//
// How the kernels walk a batch (and the shim with them): the batch-wide token array is cut into tiles of JTK_MH_TILE tokens,
// one wave each.  A shingle belongs to the tile its first token is in and reads up to n - 1 tokens past the tile's end (the
// halo).  The tile walks the documents that have tokens in it; for each it takes the minimum over the document's shingles that
// start in the tile, and flushes at the document's end or the tile's: a document that lies inside the tile is stored, one that
// spans tiles is combined by an atomic minimum into a row preset to 0xFFFFFFFF by an earlier kernel.
#ifndef JTK_MINHASH_RULES_H
#define JTK_MINHASH_RULES_H

#include <stdint.h>

#include "jtk_fim_rules.h"         // jtk_fim_mix (and jtk_first_gt through jtk_device_prims.h)

#define JTK_MH_HD JTK_FIM_HD

#define JTK_MH_G 0x9E3779B97F4A7C15ull
#define JTK_MH_MAX_NGRAM 32
#define JTK_MH_MAX_HASHES 256
#define JTK_MH_EMPTY 0xFFFFFFFFu   // sig of a document without shingles
#define JTK_MH_TILE 512            // tokens per wave: the unit of the minimum and of the combine
#define JTK_MH_BLOCK_TILES 4       // tiles (waves) per workgroup
#define JTK_MH_LANE_HASHES 4       // hash functions per lane at most: K <= 64 * 4

JTK_MH_HD bool jtk_mh_params_ok(int32_t ngram, int32_t num_hashes, int32_t bands, uint32_t flags) {
    return flags == 0 && ngram >= 1 && ngram <= JTK_MH_MAX_NGRAM && num_hashes >= 1 && num_hashes <= JTK_MH_MAX_HASHES &&
           bands >= 0 && (bands == 0 || num_hashes % bands == 0);
}

JTK_MH_HD uint64_t jtk_mh_key(uint64_t seed, int32_t ngram) { return jtk_fim_mix(seed + JTK_MH_G * ((uint64_t)ngram + 1ull)); }
JTK_MH_HD uint64_t jtk_mh_draw(uint64_t key, uint64_t j) { return jtk_fim_mix(key + j); }
JTK_MH_HD uint64_t jtk_mh_a(uint64_t key, int k) { return jtk_mh_draw(key, 2ull * (uint64_t)k + 1ull) | 1ull; }
JTK_MH_HD uint64_t jtk_mh_b(uint64_t key, int k) { return jtk_mh_draw(key, 2ull * (uint64_t)k + 2ull); }

// shingles of a document of l tokens, and their length
JTK_MH_HD int64_t jtk_mh_shingle_len(int64_t l, int32_t ngram) { return l < ngram ? l : ngram; }
JTK_MH_HD int64_t jtk_mh_n_shingles(int64_t l, int32_t ngram) { return l <= 0 ? 0 : l - jtk_mh_shingle_len(l, ngram) + 1; }

// x of the shingle t[0 .. m)
JTK_MH_HD uint32_t jtk_mh_x(const int32_t* t, int m, uint64_t key) {
    uint64_t h = 0;
    for (int j = 0; j < m; j++) h = h * JTK_MH_G + (uint64_t)(uint32_t)t[j] + 1ull;
    return (uint32_t)jtk_fim_mix(h ^ key);
}

// ((a * x + b) mod 2^64) >> 32 in the form the device takes it: one 32 x 32 + 64 multiply-add for the low word of a and the
// carry into the high word, one 32-bit multiply for the high word of a
JTK_MH_HD uint32_t jtk_mh_value(uint32_t a_lo, uint32_t a_hi, uint64_t b, uint32_t x) {
    const uint64_t t = (uint64_t)a_lo * (uint64_t)x + b;
    return (uint32_t)(t >> 32) + a_hi * x;
}

// band key j of a signature row
JTK_MH_HD uint64_t jtk_mh_band_key(uint64_t key, const uint32_t* sig_row, int32_t num_hashes, int32_t bands, int32_t j) {
    const int r = num_hashes / bands;
    uint64_t h = jtk_mh_draw(key, 0x100000000ull + (uint64_t)j);
    for (int i = 0; i < r; i++) h = jtk_fim_mix(h ^ (uint64_t)sig_row[j * r + i]);
    return h;
}

// agreement of two rows
JTK_MH_HD int32_t jtk_mh_agree(const uint32_t* a, const uint32_t* b, int32_t num_hashes) {
    int32_t n = 0;
    for (int k = 0; k < num_hashes; k++) n += a[k] == b[k];
    return n;
}

// ---- the walk of one tile [w0, w1) of the batch's tokens, w1 <= total = tok_off[n_docs], w0 < w1.
struct JtkMhView {
    const int32_t* tokens;         // [total]
    const int64_t* tok_off;        // [n_docs + 1]
    const int32_t* status;         // [n_docs]
    int64_t n_docs, total;
    int32_t ngram;
};

// the document that holds token `pos` < total: the one before the first k with tok_off[k] > pos; from document `from` on
JTK_MH_HD int64_t jtk_mh_doc_of(const JtkMhView& v, int64_t from, int64_t pos) {
    return jtk_first_gt(v.tok_off, from, v.n_docs + 1, pos) - 1;
}
// the document that holds `pos`, the end of document d (pos < total): d + 1 unless it is empty
JTK_MH_HD int64_t jtk_mh_next_doc(const JtkMhView& v, int64_t d, int64_t pos) {
    if (d + 2 <= v.n_docs && v.tok_off[d + 2] > pos) return d + 1;
    return jtk_mh_doc_of(v, d + 2, pos);
}

// One step of the walk: the part of document d (which holds pos, w0 <= pos < w1) inside the tile.
struct JtkMhSeg {
    int64_t sh_lo, sh_hi;          // the shingles that start in it: positions [sh_lo, sh_hi) of the token array (may be empty)
    int64_t end;                   // where the walk goes on: min(the document's end, w1)
    int m;                         // tokens per shingle
    bool whole;                    // the document lies inside the tile: its row is stored, not combined
    bool live;                     // status >= 0: a refused document has no shingles whatever tok_off says
};
JTK_MH_HD JtkMhSeg jtk_mh_segment(const JtkMhView& v, int64_t d, int64_t pos, int64_t w0, int64_t w1) {
    const int64_t ds = v.tok_off[d], de = v.tok_off[d + 1];
    JtkMhSeg s;
    s.m = (int)jtk_mh_shingle_len(de - ds, v.ngram);
    s.end = de < w1 ? de : w1;
    const int64_t last = de - s.m + 1;                 // one past the document's last shingle start
    s.sh_lo = pos;
    s.sh_hi = last < s.end ? last : s.end;
    s.whole = ds >= w0 && de <= w1;
    s.live = v.status[d] >= 0;
    return s;
}

// x of the shingle that starts at token position i of document d, or false when none starts there
JTK_MH_HD bool jtk_mh_x_at(const JtkMhView& v, int64_t d, int64_t i, uint64_t key, uint32_t* x) {
    const int64_t de = v.tok_off[d + 1];
    const int m = (int)jtk_mh_shingle_len(de - v.tok_off[d], v.ngram);
    if (i + m > de) return false;
    *x = jtk_mh_x(v.tokens + i, m, key);
    return true;
}

#endif  // JTK_MINHASH_RULES_H
