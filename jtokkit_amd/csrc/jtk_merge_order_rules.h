// jtk_merge_order_rules.h -- which queue entry a lane of a lean merge wave works on: the rule the kernel (lean_window in
// jtk_kernels.hip) and the CPU test shim tests/merge_order_sim share.
//
// Why.  A lean wave steps until its slowest piece has finished, and a piece's steps follow its length.  A wave that
//   takes 64 pieces of one length wastes few steps; 64 consecutive queue entries are a mix of lengths.
// The rule.
//   Passes.  A (bin, shard) queue of `count` entries is worked off in passes by the shard's K workgroups of `lanes` lanes;
//     span = K * lanes entries is what one pass takes when every wave takes 64 entries, as all passes once did.  With
//     `left` entries not yet taken, the next pass has R = jtk_mo_rounds(left, span) rounds: 4 while left >= 4 * span, 2
//     while left >= 2 * span, else 1.  A pass of R rounds takes the next R * span entries: workgroup k the R * lanes from
//     k * R * lanes on, its wave v the WINDOW of 64 * R consecutive entries from v * 64 * R on.  So every wave of every
//     workgroup of an R-round pass has a full window, a queue shorter than 2 * span is taken exactly as before (R = 1: no
//     ordering at all), and a long queue ends in at most one pass of 2 rounds and fewer than two of 1.
//   Order.  Entry i of a window (i = 64 s + l: set s, loaded by lane l) has key[i]: its length class
//     jtk_mo_class(len, lo, nc) in [0, nc), or nc when it needs no merge (JTK_QE_DONE, beyond the queue).  perm[] is the
//     stable ascending order of the keys; round r, lane l works on entry perm[64 r + l] while 64 r + l < n_live, the
//     number of keys below nc.  Entries that need no merge come last and never hold a lane of a live round.
//   With ballots.  The place of entry (s, l) of class c is
//       sum of popcount(B[c'][s']) over (c', s') before (c, s), classes outer, sets inner
//       + popcount(B[c][s] & lanes below l),           B[c][s] = ballot over the lanes of "key[64 s + l] == c":
//     nc * R ballots and popcounts, a running sum that is the same in every lane (jtk_mo_place); no atomics.
#ifndef JTK_MERGE_ORDER_RULES_H
#define JTK_MERGE_ORDER_RULES_H

#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define JTK_MO_HD __host__ __device__ inline
#else
#define JTK_MO_HD inline
#endif

#define JTK_MO_RMAX 4                       // rounds of a window at most
#define JTK_MO_W (64 * JTK_MO_RMAX)         // entries of a window at most
#define JTK_MO_NC_MAX 16                    // length classes of a bin at most (17..32 bytes)

// rounds of the next pass: `left` entries of the queue not yet taken, span = entries of a pass of one round
JTK_MO_HD uint32_t jtk_mo_rounds(uint32_t left, uint32_t span) {
    const uint64_t l = left, s = span;
    return l >= 4u * s ? 4u : l >= 2u * s ? 2u : 1u;
}

// length class of a piece of `len` bytes in a bin whose pieces are lo .. lo + nc - 1 bytes long
JTK_MO_HD uint32_t jtk_mo_class(uint32_t len, uint32_t lo, uint32_t nc) {
    const uint32_t c = len > lo ? len - lo : 0u;
    return c < nc ? c : nc - 1u;
}

// one (class, set) step: the place of lane `lane`'s entry if it is in ballot b, `before` = entries placed by earlier steps
JTK_MO_HD uint32_t jtk_mo_place(uint64_t b, uint32_t lane, uint32_t before) {
    return before + (uint32_t)__builtin_popcountll(b & ((1ull << lane) - 1ull));
}

#if !(defined(__HIPCC__) || defined(__HIP__))
// The whole window on the host, as a wave does it: key[64 * R] (nc = needs no merge) -> place[i] of every entry (the live
// ones first), perm[place[i]] = i; returns n_live.
inline uint32_t jtk_mo_order(const uint8_t* key, uint32_t R, uint32_t nc, uint16_t* place, uint16_t* perm) {
    uint32_t before = 0, n_live = 0;
    for (uint32_t c = 0; c <= nc; c++) {
        for (uint32_t s = 0; s < R; s++) {
            uint64_t b = 0;
            for (uint32_t l = 0; l < 64; l++) b |= (uint64_t)(key[64 * s + l] == c) << l;
            for (uint32_t l = 0; l < 64; l++)
                if ((b >> l) & 1ull) place[64 * s + l] = (uint16_t)jtk_mo_place(b, l, before);
            before += (uint32_t)__builtin_popcountll(b);
        }
        if (c + 1 == nc) n_live = before;
    }
    for (uint32_t i = 0; i < 64 * R; i++) perm[place[i]] = (uint16_t)i;
    return n_live;
}
#endif

#endif
