// jtk_compact_rules.h -- compact token ids: a 16-bit plane plus a plane of the bits above (jtk_batch_compact,
// JTK_ENCODE_COMPACT_IDS, jtk_widen_ids): the rule the device kernel (jtk_compact.hip), the host widening routine
// (jtk_abi.cpp) and the CPU test shim tests/compact_sim share.
//
// The rule.
//   max_id of an encoding: the largest id any result of it can hold.  Three kinds of id reach the token buffer:
//     rank-table ids        <= the table's largest (jtk_build_tables refuses tables above JTK_MAX_ID = 2^17 - 2);
//     pseudo ids            of single bytes the table lacks, largest + 1 ... (<= JTK_MAX_ID too): they STAY in the buffer --
//                           k_flag_unencodable only gives their document JTK_ERR_UNENCODABLE --, so they count;
//     special ids           with JTK_ENCODE_ALLOW_SPECIAL the stitch writes them as given to jtk_encoding_create, which
//                           accepts any id up to JTK_MAX_SPECIAL_ID (2^25 - 1, far above JTK_ID_BITS): every special id of the
//                           encoding counts, whether the batch allows it or not (the format belongs to the encoding).
//   hb (high bits per token): the smallest of {0, 1, 2, 4, 8, 16} with max_id < 2^(16 + hb) -- a power of two, so that no
//     token's high bits straddle a byte, and 32 tokens fill exactly hb words.  id_bits = 16 + hb.
//   A compact result of n tokens:
//     lo   uint16[n]                   lo[i] = id[i] & 0xFFFF
//     hi   uint32[ceil(n * hb / 32)]   (absent when hb == 0) token i's hb bits (id[i] >> 16) at bit (i * hb) % 32 of word
//                                      (i * hb) / 32, little-endian bit order; the unused bits of the last word are zero.
//   tok_off and status are token indices and per-document codes as ever: they address both planes.
//   Shipped encodings: r50k_base, p50k_base, p50k_edit hb = 0 (2 B per token; lo alone is a uint16 token shard);
//   cl100k_base hb = 1 (2.125 B per token).
//
// Ranges.  A stream is compacted in consecutive token ranges [t0, t1) as the chunks of a job finish.  A range restarts at
// jtk_compact_range_start(t0) = t0 rounded down to a multiple of 32 tokens (= hb whole words, 64 bytes of lo): everything below
// t0 is final by then, so the words that hold both ranges' tokens are rewritten whole, and the last word of a range is written
// with zeros above t1 (the next range fills them in).  The planes after the last range equal those of one pass.
#ifndef JTK_COMPACT_RULES_H
#define JTK_COMPACT_RULES_H

#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define JTK_CP_HD __host__ __device__ inline
#else
#define JTK_CP_HD inline
#endif

#define JTK_CP_RANGE_ALIGN 32     // tokens: a range restarts on a multiple of this (whole hi words for every hb)

// high bits per token for the largest id (ids are non-negative int32: max_id < 2^31)
JTK_CP_HD int jtk_compact_hb(int64_t max_id) {
    if (max_id < ((int64_t)1 << 16)) return 0;
    for (int hb = 1; hb < 16; hb *= 2)
        if (max_id < ((int64_t)1 << (16 + hb))) return hb;
    return 16;
}

JTK_CP_HD bool jtk_compact_valid_bits(int id_bits) {
    return id_bits == 16 || id_bits == 17 || id_bits == 18 || id_bits == 20 || id_bits == 24 || id_bits == 32;
}

// plane sizes of n tokens: lo in bytes, hi in 32-bit words
JTK_CP_HD int64_t jtk_compact_lo_bytes(int64_t n) { return n * 2; }
JTK_CP_HD int64_t jtk_compact_hi_words(int64_t n, int hb) { return (n * hb + 31) / 32; }

JTK_CP_HD int64_t jtk_compact_range_start(int64_t t0) { return t0 & ~(int64_t)(JTK_CP_RANGE_ALIGN - 1); }

// one token: its low plane entry, its high bits, and where those go
JTK_CP_HD uint16_t jtk_compact_lo(int32_t id) { return (uint16_t)((uint32_t)id & 0xFFFFu); }
JTK_CP_HD uint32_t jtk_compact_hi_bits(int32_t id, int hb) {
    return hb == 16 ? (uint32_t)id >> 16 : ((uint32_t)id >> 16) & ((1u << hb) - 1u);
}
JTK_CP_HD int64_t jtk_compact_hi_word(int64_t i, int hb) { return (i * hb) >> 5; }
JTK_CP_HD int jtk_compact_hi_shift(int64_t i, int hb) { return (int)((i * hb) & 31); }

// the hi bits of `count` consecutive ids (count * hb <= 32), the first of them token i: what they contribute to word
// jtk_compact_hi_word(i, hb).  A whole word is 32 / hb ids from a token whose shift is 0.
JTK_CP_HD uint32_t jtk_compact_hi_compose(const int32_t* ids, int64_t i, int count, int hb) {
    uint32_t w = 0;
    for (int k = 0; k < count; k++) w |= jtk_compact_hi_bits(ids[k], hb) << jtk_compact_hi_shift(i + k, hb);
    return w;
}

// widening: token i of the planes (hi may be NULL when hb == 0)
JTK_CP_HD int32_t jtk_compact_widen(const uint16_t* lo, const uint32_t* hi, int hb, int64_t i) {
    uint32_t id = lo[i];
    if (hb) {
        const uint32_t w = hi[jtk_compact_hi_word(i, hb)] >> jtk_compact_hi_shift(i, hb);
        id |= (hb == 16 ? w & 0xFFFFu : w & ((1u << hb) - 1u)) << 16;
    }
    return (int32_t)id;
}

// The range [t0, t1) of ids[] (indexed from token 0) into the planes, serially: what the kernel does in parallel, for the host
// (tests/compact_sim).  Reads ids from jtk_compact_range_start(t0) on.
inline void jtk_compact_range_serial(const int32_t* ids, int64_t t0, int64_t t1, uint16_t* lo, uint32_t* hi, int hb) {
    if (t1 <= t0) return;
    const int64_t tb = jtk_compact_range_start(t0);
    for (int64_t i = tb; i < t1; i++) lo[i] = jtk_compact_lo(ids[i]);
    if (!hb) return;
    const int per = 32 / hb;                                  // ids per word
    for (int64_t i = tb; i < t1; i += per) {
        const int64_t left = t1 - i;
        hi[jtk_compact_hi_word(i, hb)] = jtk_compact_hi_compose(ids + i, i, left < per ? (int)left : per, hb);
    }
}

#endif
