// jtk_cluster_rules.h -- near-duplicate clusters out of MinHash signatures and LSH band keys (jtk_batch_minhash_cluster): the
// rule the device kernels (jtk_cluster.hip) follow, and the sizes the host plans with.  tests/cluster_ref.py restates the rule
// independently.  Integer only: every result is exact.
//
// Inputs: sig[n][K] uint32 (K in 1..256), band_keys[n][B] uint64 (B in 1..256; B need not divide K here), n_shingles[n] int32 or
// NULL, min_agree in 1..K.  A document d is LIVE when n_shingles is NULL or n_shingles[d] > 0.
//   rep(d, j)     for a live d: the smallest live e with band_keys[e][j] == band_keys[d][j] (so rep(d, j) <= d); -1 for a d
//                 that is not live.  Equality is on all 64 bits and inside ONE band: the same value in two bands makes no bucket.
//                 Every value is a legal key, 0 and 2^64 - 1 included.
//   candidates    (e, d) with e = rep(d, j) < d for some j.
//   verified      a candidate with |{k : sig[e][k] == sig[d][k]}| >= min_agree.
//   labels[d]     the smallest index of d's connected component in the graph of verified pairs; d itself for a document that is
//                 not live or has no verified pair.
// The results are a function of the inputs alone: not of the table's capacity, of which keys collide in it, of how the bands are
// grouped, of the launch shape or of the order in which waves run.
//
// How this differs from HipEncoding.near_duplicates (tests/minhash_ref.py): that rule stable-sorts every band and pairs each
// document with its PREDECESSOR in the bucket; this one pairs each with the bucket's SMALLEST index, which takes one atomic
// minimum per (document, band) and no sort.  Where all members of a bucket verify against each other both give the same
// component.  They can differ on a chain that is not transitive inside one bucket: with a ~ b, b ~ c and not a ~ c in the bucket
// {a, b, c}, the predecessor rule joins all three (a-b, b-c), this rule tests a-b and a-c and leaves c alone -- unless another
// band has b and c in a bucket without a.
//
// The table of one band: `capacity` slots, a power of two, the smallest >= max(64, 2 n) -- sized by n, which bounds the live
// count, so the host never waits for a count --; a slot is a key (0 = empty, jtk_rp_claim's walk from k & (capacity - 1) with
// wrap-around) and a value, the smallest live index that brought the key, preset to all ones.  The key 0 cannot live in a slot:
// a band has one side cell for it, preset like a value.  Bands never share slots.  Bands are taken in groups of consecutive bands
// whose tables fit the byte budget together (JTK_OPT_REPEAT_TABLE_BYTES): insert a group, read its representatives out into
// rep[n][B], then the next group reuses the memory.
#ifndef JTK_CLUSTER_RULES_H
#define JTK_CLUSTER_RULES_H

#include <stdint.h>

#include "jtk_repeat_rules.h"      // jtk_rp_claim, jtk_rp_find: the open-addressing walk; through it JTK_MH_MAX_HASHES

#define JTK_CL_HD JTK_RP_HD
#define JTK_CL_MAX_BANDS 256
#define JTK_CL_NONE 0xFFFFFFFFFFFFFFFFull      // a value or side cell that no document reached

JTK_CL_HD bool jtk_cl_params_ok(int64_t n, int32_t num_hashes, int32_t bands, int32_t min_agree) {
    return n >= 0 && num_hashes >= 1 && num_hashes <= JTK_MH_MAX_HASHES && bands >= 1 && bands <= JTK_CL_MAX_BANDS && min_agree >= 1 &&
           min_agree <= num_hashes;
}
JTK_CL_HD bool jtk_cl_live(const int32_t* n_shingles, int64_t d) { return !n_shingles || n_shingles[d] > 0; }
JTK_CL_HD int64_t jtk_cl_capacity(int64_t n) { return jtk_rp_capacity(n); }
// what one band costs: keys and values of its table, and its side cell for the key 0
JTK_CL_HD int64_t jtk_cl_band_bytes(int64_t n) { return jtk_cl_capacity(n) * 16 + 8; }
// the bands of one group under a byte budget: 0 when not even one band fits
JTK_CL_HD int32_t jtk_cl_group_bands(int64_t n, int32_t bands, int64_t budget_bytes) {
    const int64_t g = budget_bytes / jtk_cl_band_bytes(n);
    return (int32_t)(g < bands ? g : bands);
}

// the tables of a group of g bands in one allocation: key [g * capacity] | val [g * capacity] | zero [g].  One memset of 0 over
// the keys, one of 0xFF over the rest.
struct JtkClTable {
    uint64_t* key;
    uint64_t* val;
    uint64_t* zero;
    int64_t capacity;
};
JTK_CL_HD JtkClTable jtk_cl_table_at(void* base, int64_t capacity, int32_t g) {
    JtkClTable t;
    t.key = (uint64_t*)base;
    t.val = t.key + (int64_t)g * capacity;
    t.zero = t.val + (int64_t)g * capacity;
    t.capacity = capacity;
    return t;
}
// Where the representative of key k of the group's band jj is kept.  insert: cas as for jtk_rp_claim, the cell afterwards takes
// an atomic minimum of d.  lookup: after all inserts of the group.
template <class Cas>
JTK_CL_HD uint64_t* jtk_cl_cell_claim(const JtkClTable& t, int32_t jj, uint64_t k, Cas cas) {
    if (k == 0) return t.zero + jj;
    const int64_t at = (int64_t)jj * t.capacity;
    return t.val + at + jtk_rp_claim(t.key + at, (uint64_t)t.capacity - 1, k, cas);
}
JTK_CL_HD const uint64_t* jtk_cl_cell_find(const JtkClTable& t, int32_t jj, uint64_t k) {
    if (k == 0) return t.zero + jj;
    const int64_t at = (int64_t)jj * t.capacity;
    return t.val + at + jtk_rp_find(t.key + at, (uint64_t)t.capacity - 1, k);
}

#endif  // JTK_CLUSTER_RULES_H
