// jtk_scratch_rules.h -- how a piece that needs bytePairMerge is binned by length, and how large the queues of one chunk's
// scratch set therefore are: the rule k_piece_resolve (jtk_kernels.hip), prepare_set (jtk_abi.cpp) and the CPU test
// (tests/test_scratch_bounds.py) share.  The sizes are proofs, not guards: no kernel checks a queue index against them.
//
// The binning rule.  A piece that is no table entry, is no gap of a custom pattern and has at most JTK_BIN_MAXLEN bytes goes to
//   bin jtk_piece_bin(len): 2..3 bytes JTK_BIN_TINY, 4..8 bin 0, 9..12 bin 1, 13..16 bin 2, then powers of two: 17..32 bin 3,
//   33..64 bin 4, 65..128 bin 5, 129..256 bin 6.  A 1-byte piece is never queued: every byte value has an id (a rank-table
//   entry, or the pseudo id of a byte that is no token), so its whole-piece lookup hits.  Pieces that come from a caller's
//   pattern (k_mark_pieces) are binned by the same function; the text between two matches and longer pieces are not queued.
// The bound.  A piece belongs to the tile its first byte is in.  Pieces do not overlap, so two pieces of at least L bytes start
//   at least L bytes apart, and at most ceil(JTK_TILE / L) of them start inside one tile (the last may straddle into the next
//   tile).  Bin b holds no piece shorter than jtk_bin_min_len(b), so a tile queues at most jtk_bin_tile_cap(b) entries there,
//   and text made of pieces of exactly that length, the first at the tile's byte 0, queues exactly that many.
//   Tile t appends to shard t % JTK_Q_SHARDS, so a shard of a chunk of n_tiles tiles takes the entries of at most
//   jtk_shard_tiles(n_tiles) tiles: jtk_bin_shard_cap(b, n_tiles) entries.  (The tiles of a shard are JTK_Q_SHARDS tiles apart,
//   and the pieces in between can be of any length: every tile of a shard can be at its own bound at once.)
#ifndef JTK_SCRATCH_RULES_H
#define JTK_SCRATCH_RULES_H

#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define JTK_SC_HD __host__ __device__ __forceinline__ constexpr
#else
#define JTK_SC_HD inline constexpr
#endif

#if !defined(JTK_TILE) || !defined(JTK_NBINS) || !defined(JTK_BIN_TINY) || !defined(JTK_Q_SHARDS) || !defined(JTK_QC_STRIDE) || !defined(JTK_BIN_MAXLEN) || !defined(JTK_LONG_CAP)
#error "jtk_scratch_rules.h is a part of jtk_kernels.h: it sizes the arrays from the constants defined there"
#endif
#define JTK_LONG_PIECE_BYTES 16  // sizeof(JtkLongPiece)

// Scratch sets (chunks in flight) of a job of more than one chunk when the caller has not chosen (JTK_OPT_CHUNKS_IN_FLIGHT):
// device-resident input, and host input whose ids stream back to the host, take JTK_SETS_DEFAULT_DEVICE; host input whose
// result stays on the device JTK_SETS_DEFAULT.  At most JTK_SETS_MAX.
#define JTK_SETS_DEFAULT 2
#define JTK_SETS_DEFAULT_DEVICE 3
#define JTK_SETS_MAX 4

// bin of a queued piece of `len` bytes, 2 <= len <= JTK_BIN_MAXLEN: up to 16 bytes three bits per length from a constant
// (k_piece_resolve spells the same expression out where it bins; bins_are_the_rule, jtk_kernels.hip, holds the two together)
JTK_SC_HD uint32_t jtk_piece_bin(uint32_t len) {
    constexpr uint64_t BIN16 = (7ull << 6) | (7ull << 9) | (1ull << 27) | (1ull << 30) | (1ull << 33) | (1ull << 36) |
                               (2ull << 39) | (2ull << 42) | (2ull << 45) | (2ull << 48);
    return len <= 16u ? (uint32_t)(BIN16 >> (3u * len)) & 7u : 30u - (uint32_t)__builtin_clz(len - 1u);
}

// the shortest piece that bin `bin` (0 .. JTK_NBINS - 1, or JTK_BIN_TINY) can hold
JTK_SC_HD uint32_t jtk_bin_min_len(int bin) {
    uint32_t len = 2;
    while (len <= (uint32_t)JTK_BIN_MAXLEN && jtk_piece_bin(len) != (uint32_t)bin) len++;
    return len;
}

// the most entries one tile can queue in `bin`
JTK_SC_HD uint32_t jtk_bin_tile_cap(int bin) {
    return ((uint32_t)JTK_TILE + jtk_bin_min_len(bin) - 1u) / jtk_bin_min_len(bin);
}

// tiles whose entries one queue shard takes, of a chunk of n_tiles tiles (shard 0 has the most)
JTK_SC_HD int64_t jtk_shard_tiles(int64_t n_tiles) { return (n_tiles + JTK_Q_SHARDS - 1) / JTK_Q_SHARDS; }

// the most entries one shard of `bin`'s queue can hold
JTK_SC_HD int64_t jtk_bin_shard_cap(int bin, int64_t n_tiles) { return jtk_shard_tiles(n_tiles) * (int64_t)jtk_bin_tile_cap(bin); }

static_assert(jtk_bin_min_len(JTK_BIN_TINY) == 2 && jtk_bin_min_len(0) == 4 && jtk_bin_min_len(JTK_NBINS - 1) <= JTK_BIN_MAXLEN,
              "every bin has a length that reaches it");
static_assert(jtk_piece_bin(JTK_BIN_MAXLEN) == JTK_NBINS - 1, "the longest queued piece goes to the last bin");
// (the state-machine phases of k_bpe_merge read bins 5 and 6 in aligned pairs of entries: a shard starts at an even entry)
static_assert(jtk_bin_tile_cap(5) % 2 == 0 && jtk_bin_tile_cap(6) % 2 == 0, "shards of the pair-read bins start 16-byte aligned");

// (JTK_BIN_CAP0..6, JTK_TINY_CAP: what k_piece_resolve reserves per tile and bin in LDS -- round figures, which keep its addressing
// cheap: with the exact ones the kernel spilled ten scalar registers)
static_assert(JTK_BIN_CAP0 >= jtk_bin_tile_cap(0) && JTK_BIN_CAP1 >= jtk_bin_tile_cap(1) && JTK_BIN_CAP2 >= jtk_bin_tile_cap(2) &&
              JTK_BIN_CAP3 >= jtk_bin_tile_cap(3) && JTK_BIN_CAP4 >= jtk_bin_tile_cap(4) && JTK_BIN_CAP5 >= jtk_bin_tile_cap(5) &&
              JTK_BIN_CAP6 >= jtk_bin_tile_cap(6) && JTK_TINY_CAP >= jtk_bin_tile_cap(JTK_BIN_TINY), "a tile's LDS slice holds its bound");

// Bytes of one queue entry of `bin`: qm (8) + qd (16); the tiny queue's entries are one 8-byte word.  (Bin 0's entries
// live in qd alone since they carry position and length themselves; its qm array is still carved and counted here.)
JTK_SC_HD int64_t jtk_bin_entry_bytes(int bin) { return bin == JTK_BIN_TINY ? 8 : 24; }

// bytes of all queues of a chunk of n_tiles tiles
JTK_SC_HD int64_t jtk_queue_bytes(int64_t n_tiles) {
    int64_t b = 0;
    for (int bin = 0; bin <= JTK_NBINS; bin++) b += jtk_bin_shard_cap(bin, n_tiles) * JTK_Q_SHARDS * jtk_bin_entry_bytes(bin);
    return b;
}

// Every array of one scratch set, in bytes, for a chunk of n_bytes from its tile-aligned origin: what prepare_set allocates.
// plist, htok and docpre are indexed by byte position (docpre is also the pair-rank scratch and the token count of a giant
// piece, k_bpe_merge: 32 bits per position); the three piece lists hold pieces longer than JTK_BIN_MAXLEN / JTK_LONG_CAP bytes.
struct JtkSetSizes {
    int64_t n_words, n_tiles;
    int64_t mask, qcnt, zeroed, plist, htok, docpre, tile_np, tile_off, q_meta, queues, mid_list, long_list, giant_list;
    constexpr int64_t total() const {
        return zeroed + mask /* piecemask */ + plist + htok + docpre + tile_np + tile_off + q_meta + queues + mid_list + long_list + giant_list;
    }
};

JTK_SC_HD JtkSetSizes jtk_set_sizes(int64_t n_bytes) {
    JtkSetSizes z{};
    z.n_words = (n_bytes + 1 + 63) / 64 + 2;
    z.n_tiles = (n_bytes + 1 + JTK_TILE - 1) / JTK_TILE;
    const int64_t nt = z.n_tiles;
    const int64_t n_long_max = n_bytes / (JTK_BIN_MAXLEN + 1) + 2, n_giant_max = n_bytes / JTK_LONG_CAP + 2;
    z.mask = z.n_words * 8;
    z.qcnt = (int64_t)(JTK_NBINS + 1) * JTK_Q_SHARDS * JTK_QC_STRIDE * 4;
    z.zeroed = z.mask + 32 + z.qcnt;                       // docmask | list counters | queue counters
    z.plist = nt * JTK_TILE * 4;
    z.htok = nt * JTK_TILE * 4 + 64;
    z.docpre = nt * JTK_TILE * 4;
    z.tile_np = (nt * 4 + 15) / 16 * 16 * 2;               // tile_np | tile_tot
    z.tile_off = (nt + 1) * 8;
    z.q_meta = nt * 4 * 16;
    z.queues = jtk_queue_bytes(nt);
    z.mid_list = n_long_max * JTK_LONG_PIECE_BYTES;
    z.long_list = n_long_max * JTK_LONG_PIECE_BYTES;
    z.giant_list = n_giant_max * JTK_LONG_PIECE_BYTES;
    return z;
}

#endif
