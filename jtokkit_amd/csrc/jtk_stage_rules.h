// jtk_stage_rules.h -- where k_pack_tokens keeps a tile's merge results in LDS: the rule the kernel (jtk_kernels.hip) and
// the CPU test shim tests/stage_sim share.
//
// The rule.
//   A pack wave owns ONE array of 16-byte slots: JTK_PACK_SLOTS head slots, then JTK_PACK_OUT_SLOTS slots that are also the
//   JTK_PACK_STAGE words in which a tile of at most that many tokens is assembled (word w of the assembly = word w % 4 of
//   slot JTK_PACK_SLOTS + w / 4).
//   Head: the first JTK_PACK_CAP(b) results of the tile's slice of bin b's queue sit at slot JTK_PACK_OFF(b) + i
//     (k_piece_resolve marks those pieces JTK_PL_STAGED and stores the slot in the list entry).
//   Extension: the assembly words [0, total) of a staged tile (total <= JTK_PACK_STAGE) are written during the steps; the
//     slots above them are free, and a tile of more tokens writes straight to memory, so all of its JTK_PACK_OUT_SLOTS are.
//     The free slots go to the results beyond the heads, bin by bin in the order 0, 1, ..., JTK_NBINS_STAGE - 1: bin b gets
//     n[b] = min(nq[b] - JTK_PACK_CAP(b), what is left) consecutive slots from off[b]; result i of the bin
//     (JTK_PACK_CAP(b) <= i < JTK_PACK_CAP(b) + n[b]) sits at slot off[b] + i - JTK_PACK_CAP(b).  Results beyond that are read
//     from the queue on demand.  (The tiny bin has a staging area of its own and takes no part.)
#ifndef JTK_STAGE_RULES_H
#define JTK_STAGE_RULES_H

#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define JTK_ST_HD __host__ __device__ inline
#else
#define JTK_ST_HD inline
#endif

// the head of a tile's slice of each bin's queue that pack stages in LDS: 32 + 16 + 16 results of the three classes of <= 16
// bytes (staging slots 0..63), 8 of each longer bin (64..95); tiny pieces have a staging area of their own (JTK_PACK_TINY).
// (Three times as much -- enough for every tile of CJK text -- made pack 3 % faster on mixed text and 10 % slower on prose.)
#define JTK_PACK_TINY 128
#define JTK_PACK_SLOTS 96
#define JTK_PACK_CAP(bin) ((bin) == 0 ? 32 : (bin) <= 2 ? 16 : 8)
#define JTK_PACK_OFF(bin) ((bin) == 0 ? 0 : (bin) == 1 ? 32 : (bin) == 2 ? 48 : 64 + ((bin) - 3) * 8)
#ifndef JTK_PACK_STAGE
#define JTK_PACK_STAGE 768                          // tokens of a tile assembled in LDS (ordinary text: a few hundred)
#endif
#define JTK_PACK_OUT_SLOTS (JTK_PACK_STAGE / 4)
#define JTK_NBINS_STAGE 7                           // = JTK_NBINS: every queue but the tiny one

// first slot (counted from the start of the assembly words) that a tile of `total` tokens leaves free
JTK_ST_HD uint32_t jtk_stage_first_free(uint32_t total) {
    return total > (uint32_t)JTK_PACK_STAGE ? 0u : (total + 3u) / 4u;
}

// One bin: `over` results beyond its head, `over_before` = the same summed over the bins before it.  n: how many of them get a
// slot; off: the first of those slots in the array.  (min(before + over, room) - min(before, room): in bin order until the
// room is gone.)
JTK_ST_HD void jtk_stage_place(uint32_t total, uint32_t over_before, uint32_t over, uint32_t* off, uint32_t* n) {
    const uint32_t first = jtk_stage_first_free(total), room = (uint32_t)JTK_PACK_OUT_SLOTS - first;
    const uint32_t a = over_before < room ? over_before : room;
    const uint32_t e = over_before + over < room ? over_before + over : room;
    *off = (uint32_t)JTK_PACK_SLOTS + first + a;
    *n = e - a;
}

JTK_ST_HD uint32_t jtk_stage_over(int bin, uint32_t nq) {
    return nq > (uint32_t)JTK_PACK_CAP(bin) ? nq - (uint32_t)JTK_PACK_CAP(bin) : 0u;
}

// the whole tile: nq[b] results in bin b -> off[b], n[b]
JTK_ST_HD void jtk_stage_rules(uint32_t total, const uint32_t* nq, uint32_t* off, uint32_t* n) {
    uint32_t before = 0;
    for (int b = 0; b < JTK_NBINS_STAGE; b++) {
        const uint32_t over = jtk_stage_over(b, nq[b]);
        jtk_stage_place(total, before, over, &off[b], &n[b]);
        before += over;
    }
}

// What a step needs per bin, in one word: result i of an unstaged entry is in LDS if i < (word >> 16), at slot
// (word & 0xFFFF) + i.
JTK_ST_HD uint32_t jtk_stage_word(int bin, uint32_t off, uint32_t n) {
    return n ? (off - (uint32_t)JTK_PACK_CAP(bin)) | (((uint32_t)JTK_PACK_CAP(bin) + n) << 16) : 0u;
}

#endif
