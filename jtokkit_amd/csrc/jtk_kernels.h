// jtk_kernels.h -- launch interface of the gfx950 kernels (implemented in jtk_kernels.hip).
#ifndef JTK_KERNELS_H
#define JTK_KERNELS_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "jtk_common.h"
#include "jtk_pack_rules.h"
#include "jtk_label_rules.h"
#include "jtk_stage_rules.h"
#include "jtk_decode_rows_rules.h"
#include "jtk_charpos_rules.h"
#include "jtk_utf16_rules.h"
#include "jtk_stop_rules.h"
#include "jtk_fim_rules.h"
#include "jtk_minhash_rules.h"

#define JTK_SPLIT_TILE 4096      // bytes per pretok_split workgroup
#define JTK_SPLIT_HALO 64
#define JTK_TILE 2048            // bytes per piece_resolve / pack workgroup; token counts are kept per tile
// Pieces that need bytePairMerge are queued by length bin; bin k holds pieces of up to JTK_BIN_SLOTS(k) bytes.
// Queues are dense and sharded: tile t appends its entries to shard t % JTK_Q_SHARDS with one returning
// atomic per tile and bin.  A queue entry is two words in two parallel arrays:
//   qm  (8 bytes)   pos (37 bits) | (len - 1) << 37
//   qd  (16 bytes)  bins 0..2: IN the piece's bytes (<= 16, what piece_resolve hashed), OUT the merge result;
//                   bins 3..6: OUT the merge result (their bytes are read from the text)
// Merge result: (token count - 1) in the top byte | up to seven token ids, 17 bits each from bit 0; a piece that
// became more than seven tokens leaves its tokens in htok (packed from its first byte position).  The merge kernels
// add every piece's token count to tile_tot[tile] (piece_resolve stored the resolved pieces' count there).
#define JTK_QE_POS_MASK ((1ull << 37) - 1ull)
#define JTK_QE_LEN_SHIFT 37
#define JTK_QE_DONE (1ull << 63)       // the piece is a table entry found by k_long_shortcut: its result is in place already
#define JTK_NBINS 7
// Pieces of 2 or 3 bytes that are not table entries need no pair-table lookup at all (at most one merge of a 2-byte token;
// the pair that would follow is the whole piece, which is not an entry).  They get a queue of their own ("bin" JTK_BIN_TINY
// of a piece-list entry) with 8-byte entries that carry the bytes: pos (37 bits) | (len - 2) << 37 | b0 << 40 | b1 << 48 |
// b2 << 56; the merge kernel replaces an entry by its result: up to three token ids, 17 bits each from bit 0 (the first 64
// bits of a merge result word), | (count - 1) << 62.
#define JTK_BIN_TINY 7
#define JTK_TINY_CAP (JTK_TILE / 2)
#define JTK_Q_SHARDS 64
// Every queue counter has a 128-byte line of its own: the tiles' claims are returning atomics, and atomics on one line
// are served one after another (about 14 ns each): with the 512 counters packed into 16 lines the claims of a GiB of mixed
// text -- one per tile and bin -- took 1.8 ms, most of piece_resolve's time.
#define JTK_QC_STRIDE 32
#define JTK_QC(bin, shard) (((bin) * JTK_Q_SHARDS + (shard)) * JTK_QC_STRIDE)
// Bins by length.  A wave of the merge kernel steps until its longest piece is done, so pieces of like length are queued
// together: three classes up to 16 bytes (whose entries carry the piece's bytes), then powers of two.
#define JTK_BIN_CAP0 (JTK_TILE / 4)    // per tile: pieces of 4..8 bytes (2..3-byte pieces: JTK_BIN_TINY)
#define JTK_BIN_CAP1 (JTK_TILE / 8)    //           9..12 bytes
#define JTK_BIN_CAP2 160               //           13..16 bytes (2048 / 13 = 157)
#define JTK_BIN_CAP3 (JTK_TILE / 16)   //           17..32 bytes
#define JTK_BIN_CAP4 (JTK_TILE / 32)   //           33..64 bytes
#define JTK_BIN_CAP5 (JTK_TILE / 64)   //           65..128 bytes
#define JTK_BIN_CAP6 (JTK_TILE / 128)  //           129..256 bytes
// (what pack stages of a tile's results in LDS, JTK_PACK_*: jtk_stage_rules.h)
#define JTK_NBINS_BYTES 3              // bins 0..2: the queue entry carries the piece's bytes
#define JTK_NBINS_LEAN 5               // bins 0..4: lean phases of the merge kernel; 5..6: state-machine phases
#define JTK_BIN_MAXLEN 256            // longer pieces go to the wave-per-piece kernels
#define JTK_M_WGS_PER_SHARD 4
#define JTK_MID_CAP 512          // wave-per-piece kernel, small bin: pieces of 257..512 bytes (up to 256: the bins)
#define JTK_LONG_CAP 8192        // wave-per-piece kernel, large bin
#define JTK_GIANT_CAP (1 << 20)  // workgroup-per-piece kernel with parts in global scratch (= JTK_MAX_PIECE_BYTES)
#define JTK_GIANT_CHUNK 256      // positions per cached chunk minimum
#define JTK_MAX_SPECIALS 65536           // special-token literals live in a device blob: the bounds are sanity checks only
#define JTK_SPECIAL_MAXLEN 65535

#define JTK_UC_LDS_UNITS 768      // capacity of the LDS copy of the Unicode class table (pretok_split), in 16-byte units:
                                  // a copying wave moves whole rows of 64 units, a few at a time
#define JTK_UC_LDS_STAGE1 4352    // bytes of it that hold stage 1 (a multiple of 16); stage 2 follows

struct JtkDeviceTables {
    JtkUcTables uc;
    // The same table as pretok_split stages it in LDS, JTK_UC_LDS_UNITS units of 16 bytes: stage 1 in the first
    // JTK_UC_LDS_STAGE1 bytes, then stage 2, zero-filled to the end.  Null: the table does not fit.
    const uint32_t* uc_lds_image;
    const uint32_t* split_tab;   // [256 * 4] jtk_build_code4_table: the per-byte flag table of pretok_split, 16 bytes per byte value
    const uint32_t* byte_rank;   // [256]
    JtkPairTable pairs;
    JtkTok8Table tok8;
    JtkTok16Table tok16;
    const uint32_t* bp_rank;     // [65536]
    JtkBpLds bp;                 // the same, compressed (staged into LDS by bpe_merge)
    const uint32_t* pair_in_token;   // [2048] bit (b0 << 8 | b1): adjacent inside some table entry
    JtkLongTokTable longtok;         // table entries of > 16 bytes that merging does not reproduce (n == 0 for the shipped tables)
    int kind;
    uint32_t pseudo_base;            // ids from here on stand for single bytes that are no tokens (0: the table has all 256)
    int n_specials;
    uint32_t special_first[8];       // bit b: some special-token literal starts with byte b
    const uint8_t* special_blob;     // the literals back to back
    const uint32_t* special_off;     // [n_specials + 1] into special_blob
};

// piece-list entry.  Resolved piece: token id (bits 0..16) | byte offset in the tile << 17.
// Merged piece: JTK_PL_HARD | byte offset in the tile (bits 0..10) and either its queue entry (bin << 21 | index in
// the tile's slice of the bin's queue << 11) or JTK_PL_NOQUEUE (wave / workgroup kernels: tokens and count in htok).
#define JTK_PL_HARD 0x80000000u
#define JTK_PL_NOQUEUE 0x40000000u
#define JTK_PL_STAGED 0x20000000u        // queued piece whose result is in the head of the tile's queue slice that pack stages in LDS:
                                         // the index field then holds its staging slot (pack_stage_slot), not the index in the bin
#define JTK_PL_OFF_SHIFT 17
#define JTK_PL_QI_SHIFT 11
#define JTK_PL_BIN_SHIFT 21
#define JTK_HT_ID_MASK 0x1FFFFu
#define JTK_HT_CNT_SHIFT 17
#define JTK_HT_CNT_MASK 0x3FFFu
#define JTK_HT_ESCAPE 0x3FFFu            // count does not fit: giant piece, count in docpre[pos + 1]

struct JtkLongPiece {
    int64_t start;
    int64_t len;
};

struct JtkResult {          // of a whole batch (all its chunks)
    int64_t n_tokens;
    int32_t worst_status;
    uint32_t pad;
};

// Device-side working set of ONE CHUNK of an encode call: a run of whole documents of the batch, encoded with one scratch
// set.  A batch is one chunk, or several that flow through a few scratch sets on their own streams (jtk_abi.cpp).
// Positions are relative to the chunk's origin `text` = batch text + text_base (text_base is a multiple of JTK_TILE, so the
// chunk's first document starts `lead` < JTK_TILE bytes in; the bytes before it belong to the previous chunk and start no
// piece here).  doc_off / status / tok_off point at the chunk's first document in the batch-wide arrays.
struct JtkWork {
    const uint8_t* text;
    const int64_t* doc_off; // [n_docs + 1] positions in the whole batch (subtract text_base)
    int64_t text_base;
    int64_t lead;
    int64_t n_bytes;        // from the chunk's origin to the end of its last document
    int64_t n_docs;
    int64_t n_words;        // 64-bit mask words (covers position n_bytes, plus padding)
    int64_t n_tiles;
    uint32_t count_only;    // countTokens(): pack computes the offsets but writes no token ids
    uint32_t inline_scan;   // small single-chunk job: pack adds up the tiles before its own itself and k_tile_scan is not launched
    uint32_t check_special; // encode(): flag documents that contain a special-token literal (done inside pretok_split)
    uint64_t* docmask;      // bit p: a document starts at byte p
    uint64_t* piecemask;    // bit p: a pre-token piece starts at byte p (bit n_bytes is a sentinel)
    uint64_t* gapmask;      // NULL, or (caller-supplied pieces, jtk_batch_encode_pieces) bit p: the "piece" that starts at byte p is
                            // text between two matches of the caller's pattern: it is not encoded (matcher.find() skips it)
    uint32_t* plist;        // [n_tiles * JTK_TILE] per tile, packed from the tile's first word: its pieces in text order,
                            // JTK_PL_* entry per piece (a piece belongs to the tile it starts in)
    uint32_t* tile_np;      // [n_tiles] pieces in each tile's list
    uint32_t* htok;         // [n_tiles * JTK_TILE] tokens of a merged piece without a (big enough) result slot, packed from the
                            // piece's first byte position (k <= len words); word 0 also carries the count k: id | k << 17
                            // (JTK_HT_ESCAPE: the count is in docpre[pos + 1])
    uint32_t* docpre;       // [n_tiles * JTK_TILE] at a document's first byte: tokens of its tile before it (sparse)
    uint32_t* tile_tot;     // [n_tiles] tokens of the tile's pieces: piece_resolve stores the resolved pieces (one token
                            // each), the merge kernels add theirs
    int64_t* tile_off;      // [n_tiles + 1] exclusive scan of tile_tot
    uint64_t* qm[JTK_NBINS];        // [JTK_Q_SHARDS][q_cap[k]] queue entries of bin k: position and length
    uint4* qd[JTK_NBINS];           // [JTK_Q_SHARDS][q_cap[k]] ... : bytes in (bin 0), merge result out
    int64_t q_cap[JTK_NBINS];       // entries per shard
    uint64_t* qt;                   // [JTK_Q_SHARDS][qt_cap] the queue of JTK_BIN_TINY: bytes in, result out
    int64_t qt_cap;
    uint32_t* q_count;              // [JTK_NBINS + 1][JTK_Q_SHARDS], one counter per 128-byte line: JTK_QC(bin, shard)
    uint32_t* q_meta;               // [n_tiles][16]: [k] where in its shard the tile's entries of bin k start, [8 + k] how many
    JtkLongPiece* mid_list; // pieces of 257..JTK_MID_CAP bytes (JTK_BIN_MAXLEN + 1 ..)
    JtkLongPiece* long_list;// longer pieces
    JtkLongPiece* giant_list;// pieces longer than JTK_LONG_CAP
    uint32_t* mid_count;
    uint32_t* long_count;
    uint32_t* n_giant;      // pieces longer than JTK_LONG_CAP (listed by piece_resolve, merged by the last phase of k_bpe_merge_all)
    int32_t* status;        // per document
    int32_t* tokens;        // output of the whole batch, packed (tile_off already includes the earlier chunks' tokens)
    int64_t* tok_off;       // output, n_docs + 1
    const int64_t* job_tokens;   // tokens of the batch's earlier chunks (written by the previous chunk's scan)
    int64_t* job_tokens_next;    // ... including this one (for the next chunk)
    int64_t* set_info;      // [2] (device-visible host memory) first token of this chunk, end of its last
    JtkResult* result;
};

// Device-side working set of one batch decode (jtk_decode.hip).
#define JTK_DEC_TILE 2048        // tokens per decode workgroup
struct JtkDecodeWork {
    const int32_t* ids;         // all sequences' token ids back to back
    const int64_t* seq_off;     // [n_seqs + 1]
    int64_t n_tok, n_seqs, n_tiles;
    const uint32_t* tab_off;    // [n_ids_table + 1] byte offset of every id's byte string in tab_blob (absent id: empty)
    const uint8_t* tab_blob;
    uint32_t n_ids_table;
    uint64_t* seqmask;          // bit t: a sequence starts at token t (zeroed per call)
    uint32_t* tile_bytes;       // [n_tiles]
    int64_t* tile_off;          // [n_tiles + 1]
    uint32_t* seqpre;           // at a sequence's first token: bytes of its tile before it (sparse)
    int32_t* status;            // [n_seqs] (zeroed per call)
    int32_t* worst_status;
    int64_t* total;
    uint8_t* out;               // NULL in the sizing phase
    int64_t* byte_off;          // [n_seqs + 1]
};
// Device-side working set of one decode of an id matrix (jtk_decode_rows.hip; the rule is jtk_decode_rows_rules.h).  Cells are
// numbered t = r * width + c; tiles of JTK_DEC_TILE cells.
struct JtkDecodeRowsWork {
    const void* rows;           // ids of id_bytes (4 or 8) bytes, row r at element r * row_stride; aligned to id_bytes only
    int id_bytes;
    int64_t n_rows, width, row_stride, n_cells, n_tiles;
    const int64_t* begin;       // [n_rows] or NULL
    const int64_t* end;         // [n_rows] or NULL
    JtkDecodeRowsRule rule;
    const uint32_t* tab_off;    // as in JtkDecodeWork
    const uint8_t* tab_blob;
    uint32_t n_ids_table;
    unsigned long long* first_stop;   // [n_rows] first stop column inside the window (set to JTK_DR_NO_STOP per call); NULL
                                      // without stop ids
    uint32_t* tile_bytes;       // [n_tiles]
    int64_t* tile_off;          // [n_tiles + 1]
    int32_t* status;            // [n_rows] (zeroed per call)
    int64_t* total;
    uint8_t* out;
    int64_t* byte_off;          // [n_rows + 1]
    int64_t* cell_byte;         // [n_rows * width] or NULL
};
void jtk_launch_decode_rows_count(const JtkDecodeRowsWork& w, hipStream_t s);     // row ends (with stop ids), count, scan
void jtk_launch_decode_rows_scatter(const JtkDecodeRowsWork& w, hipStream_t s);   // bytes, byte_off, cell_byte
struct JtkTruncWork {
    const int32_t* tokens;      // result of the last batch encode
    const int64_t* tok_off;
    const uint8_t* text;
    const int64_t* doc_off;
    int64_t n_docs;
    const uint32_t* tab_off;    // decode table offsets (token byte lengths)
    int64_t max_tokens;
    int64_t* kept;              // [n_docs] tokens kept per document
    uint8_t* truncated;         // [n_docs] EncodingResult.isTruncated()
};
void jtk_launch_truncate(const JtkTruncWork& w, hipStream_t s);
// Device-side state of jtk_batch_encode_device_max_tokens (jtk_maxtok.hip): the caller's batch and output rows, and the
// rounds of the early exit.  A round takes the documents that are still open (round 1: all), gathers their leading bytes
// back to back into `gather` (slot i = the round's i-th open document, bytes [goff[i], goff[i + 1])), encodes them with
// run_job and decides per chunk which documents are done.
struct JtkMaxTokWork {
    const uint8_t* text;        // caller text (any alignment; only the 16-byte blocks that hold [0, n_bytes) are read)
    const int64_t* doc_off;     // [n_docs + 1] caller offsets into text
    int64_t n_docs, n_bytes;
    int64_t max_tokens;
    int32_t pad_id;
    int32_t round;              // 1, 2, ...
    int32_t* out_tokens;        // [n_docs * max_tokens] rows
    int64_t* out_kept;          // [n_docs]
    uint8_t* out_truncated;     // [n_docs]
    int32_t* out_status;        // [n_docs]
    uint8_t* special;           // [n_docs] encode(): the document holds a special-token literal (round 1)
    uint32_t* bad;              // the offsets are not non-decreasing within [0, n_bytes]
    int64_t* hdr;               // [2] after the plan: open documents of this round (-1: bad offsets), gathered bytes
    int64_t P, cb;              // prefix size of this round; documents whose prefix exceeds cb go whole
    const int64_t* act_in;      // round > 1: the documents of the previous round [n_in] ...
    const uint8_t* again_in;    //            ... and whether each is still open
    int64_t n_in;               // items the plan looks at (round 1: n_docs)
    int64_t* act;               // [n_docs] this round's documents, in document order
    int64_t* goff;              // [n_docs + 1] their prefixes in the gather buffer
    uint8_t* again;             // [n_docs] per slot of this round: still open after the decision
    uint32_t* blk_cnt;          // [n_blk] plan: open documents per block of 1024 items
    int64_t* blk_bytes;         // [n_blk] ... and their prefix bytes
    int64_t* blk_base;          // [2 * n_blk] exclusive scans of both
    int64_t n_blk;
    uint8_t* gather;            // the prefixes (16-byte aligned, 64 bytes of tail)
    int64_t gbytes;             // gathered bytes of this round
    const uint32_t* tab_off;    // decode table offsets (token byte lengths)
    uint32_t n_ids_table;
};
void jtk_launch_maxtok_check(const JtkMaxTokWork& m, hipStream_t s);                              // offsets valid?
void jtk_launch_maxtok_special(const JtkMaxTokWork& m, const JtkDeviceTables& t, hipStream_t s);  // text.contains(literal)
void jtk_launch_maxtok_finish_closed(const JtkMaxTokWork& m, hipStream_t s);                      // round 1: rows needing no encode
void jtk_launch_maxtok_plan(const JtkMaxTokWork& m, hipStream_t s);                               // count, scan, place
void jtk_launch_maxtok_gather(const JtkMaxTokWork& m, int64_t n_act, hipStream_t s);
// per-chunk epilogue of run_job: chunk documents are slots [slot0, slot0 + w.n_docs) of the round
void jtk_launch_maxtok_decide(const JtkWork& w, const JtkMaxTokWork& m, int64_t slot0, hipStream_t s);
// Device-side state of jtk_batch_chunk (jtk_chunk.hip): chunks of at most chunk_tokens tokens of every document of the last
// batch encode, by the rule of jtk_chunk_rules.h.  G(t) = bytes of the batch's tokens before token t (all documents): per tile
// of JTK_DEC_TILE tokens its start tile_off[], and per group of 16 tokens the bytes of its tile before it, sub16[].
struct JtkChunkWork {
    const int32_t* tokens;      // result of the last batch encode
    const int64_t* tok_off;     // [n_docs + 1]
    const int32_t* status;      // [n_docs]
    const int64_t* doc_off;     // [n_docs + 1] the encode's offsets into its text
    int64_t n_docs, n_tok;
    int64_t N, overlap;
    const uint32_t* bnd;        // boundary bit per id: the id's byte string does not start with a continuation byte
    const uint32_t* tab_off;    // decode table offsets (token byte lengths)
    uint32_t n_ids_table;
    int64_t* hdr;               // [0] chunks, [1] tokens (tok_off[n_docs]), [2] long documents
    int64_t* chunk_off;         // [n_docs + 1] chunks per document, then their exclusive scan
    int64_t* long_docs;         // [n_docs] documents with many chunks (a workgroup each)
    int64_t* dbase;             // [n_docs] doc_off[d] - G(tok_off[d])
    uint32_t* tile_bytes;       // [n_tiles]
    int64_t* tile_off;          // [n_tiles + 1]
    uint32_t* sub16;            // [n_tok / 16 + 1]
    int64_t n_tiles;
    // records [n_chunks]
    int64_t* chunk_doc;
    int64_t* tok_begin;
    int32_t* n_tok_out;
    int64_t* byte_begin;
    int64_t* byte_end;
    uint8_t* split;
    int64_t n_chunks;
};
void jtk_launch_chunk_count(const JtkChunkWork& w, hipStream_t s);      // count per document, scan -> hdr
void jtk_launch_chunk_tiles(const JtkChunkWork& w, hipStream_t s);      // tile sums, sub16, tile scan, dbase (needs n_tok)
void jtk_launch_chunk_write(const JtkChunkWork& w, hipStream_t s);      // records (needs n_chunks and the tiles)
void jtk_launch_chunk_rows(const JtkChunkWork& w, int32_t pad_id, int32_t* rows, hipStream_t s);
void jtk_launch_token_offsets(const JtkChunkWork& w, int64_t* byte_pos, hipStream_t s);   // (needs the tiles)
// the one-workgroup exclusive scan (k_ck_scan of jtk_chunk.hip around jtk_block_scan_array): in[0, n) -> out[0, n), the sum
// to out[n] and to *total (may be NULL).  _i64 scans in place.
void jtk_launch_scan_i64(int64_t* inout, int64_t n, int64_t* total, hipStream_t s);
void jtk_launch_scan_u32(const uint32_t* in, int64_t n, int64_t* out, int64_t* total, hipStream_t s);
// Device-side state of jtk_batch_chunk_prefer (jtk_chunk_prefer.hip): the chunk work above (same scratch, same records) plus
// the level plane and the level of every chunk's end, by the rule of jtk_chunk_prefer_rules.h.  A document of more than
// JTK_CP_LONG_TOKENS tokens (and more than one chunk) is walked by a workgroup, any other by one lane.
#define JTK_CP_LONG_TOKENS 8192
struct JtkChunkPreferWork {
    JtkChunkWork w;
    const uint8_t* plane;       // [n_tok] level of the cut before every token (6: first token of a document)
    uint8_t* end_level;         // [n_chunks]
    int64_t min_tokens;
    uint32_t prefer;            // JTK_CUT_* mask
};
// the level plane of w's tokens (reads w.tokens, tok_off, n_docs and the decode table; the token count stays on the device)
void jtk_launch_cut_levels(const JtkChunkWork& w, const uint8_t* tab_blob, uint32_t prefer, uint8_t* plane, hipStream_t s);
void jtk_launch_chunk_prefer_count(const JtkChunkPreferWork& p, hipStream_t s);   // count per document, scan -> hdr (needs the plane)
void jtk_launch_chunk_prefer_write(const JtkChunkPreferWork& p, hipStream_t s);   // records (needs n_chunks and the tiles)
void jtk_launch_chunk_bytes(const JtkChunkWork& w, hipStream_t s);      // byte_begin / byte_end of written records (k_ck_bytes)
// Device-side state of jtk_batch_pack (jtk_pack.hip): the units of the last batch encode packed into rows of L tokens by the
// rule of jtk_pack_rules.h.  The view's P, SEG, RS, flag and nxt point into the scratch below.
struct JtkPackWork {
    JtkPackView v;
    const int32_t* status;      // [n] of the last encode
    int64_t* hdr;               // [0] |S|, [1] SEG[n], [2] RS[n] (whole: rows), [3] the longest segment
    int64_t* P;                 // [n + 1] unit offsets in S
    int64_t* SEG;               // [n + 1]
    int64_t* RS;                // [n + 1] (whole)
    uint8_t* flag;              // [n]     (whole)
    int32_t* up;                // [K][n + 1] (whole): up[k][d] = the head 2^k groups after the group of d; up[0] = nxt
    int K;                      // ceil(log2(n + 1)) lifting levels
    bool drop_last;
    int64_t n_rows, n_seg;
};
void jtk_launch_pack_plan(const JtkPackWork& w, hipStream_t s);        // units, scans, groups -> hdr
void jtk_launch_pack_write(const JtkPackWork& w, int32_t pad_id, int32_t* rows, int32_t* positions, int32_t* cu_seqlens,
                           int64_t* seg_doc, hipStream_t s);           // (needs n_rows, n_seg)
// Labels (jtk_label.hip; the rule is jtk_label_rules.h).  tok_span[n_tok] of the chunk work's tokens from the spans
// [begin[i], end[i]), i < n_spans (needs the tiles of jtk_launch_chunk_tiles); labels[n_rows * L] of the pack work's rows.
void jtk_launch_label_spans(const JtkChunkWork& w, const int64_t* begin, const int64_t* end, int64_t n_spans, int rule,
                            int32_t* tok_span, hipStream_t s);
void jtk_launch_label_pack(const JtkPackWork& w, const JtkLabelView& lv, bool shift, int32_t* labels, hipStream_t s);
// Character positions (jtk_charpos.hip; the rule and the index are jtk_charpos_rules.h).  build: the index of ix.text for ix.unit
// into sup_cnt [n_sup] (scratch), sup [n_sup + 1] and sub [n_sup * 64] (ix.sup / ix.sub point at them), then dunit[d] =
// rank(doc_off[d]) for d = 0 .. n_docs.  The queries take the built index; tokens: begin / end (may be NULL) [n_tok] of the chunk
// work's tokens (needs the tiles of jtk_launch_chunk_tiles).
void jtk_launch_charpos_build(const JtkCharIndex& ix, uint32_t* sup_cnt, int64_t* sup, uint16_t* sub, const int64_t* doc_off,
                              int64_t n_docs, int64_t* dunit, hipStream_t s);
void jtk_launch_charpos_doc_units(const int64_t* doc_off, const int64_t* dunit, int64_t n_docs, int64_t* doc_units, hipStream_t s);
void jtk_launch_charpos_rank(const JtkCharIndex& ix, const int64_t* doc_off, const int64_t* dunit, int64_t n_docs, int round,
                             const int64_t* doc, const int64_t* byte_pos, int64_t n, int64_t* char_pos, hipStream_t s);
void jtk_launch_charpos_select(const JtkCharIndex& ix, const int64_t* doc_off, const int64_t* dunit, int64_t n_docs, const int64_t* doc,
                               const int64_t* char_pos, int64_t n, int64_t* byte_pos, hipStream_t s);
void jtk_launch_charpos_tokens(const JtkChunkWork& w, const JtkCharIndex& ix, const int64_t* dunit, int64_t* begin, int64_t* end,
                               hipStream_t s);
// UTF-16 in and out (jtk_utf16.hip; the rules are jtk_utf16_rules.h).  E: the documents unit_off[0 .. n_docs] of units[n_units]
// to UTF-8 in out, doc_off[n_docs + 1].  D: the sequences byte_off[0 .. n_seqs] of text[n_bytes] (16-byte aligned, readable to
// the next multiple of 16) to UTF-16 units in out, unit_off[n_seqs + 1].  Tiles of 256 lanes: tile_cnt [n_tiles] (scratch),
// tile_off [n_tiles + 1], sub [n_tiles * 256].  count: sub, tile_off and hdr[0] = the size of the output (E: hdr[1], zeroed by
// the caller, != 0 for bad offsets); write (needs out, 16-byte aligned): the output and its offsets.
struct JtkU16EncWork {
    const uint16_t* units;
    int64_t n_units;
    const int64_t* unit_off;
    int64_t n_docs, n_tiles;
    uint32_t* tile_cnt;
    int64_t* tile_off;
    uint16_t* sub;
    int64_t* hdr;
    uint8_t* out;
    int64_t* doc_off;
};
struct JtkU16DecWork {
    const uint8_t* text;
    int64_t n_bytes;
    const int64_t* byte_off;
    int64_t n_seqs, n_tiles;
    uint32_t* tile_cnt;
    int64_t* tile_off;
    uint16_t* sub;
    int64_t* hdr;
    uint16_t* out;
    int64_t* unit_off;
};
void jtk_launch_u16_enc_count(const JtkU16EncWork& w, bool aligned, hipStream_t s);   // aligned: units is 16-byte aligned
void jtk_launch_u16_enc_write(const JtkU16EncWork& w, bool aligned, hipStream_t s);
void jtk_launch_u16_dec_count(const JtkU16DecWork& w, hipStream_t s);
void jtk_launch_u16_dec_write(const JtkU16DecWork& w, hipStream_t s);
// Stop strings over the last decode (jtk_stop.hip; the rule is jtk_stop_rules.h): out (16-byte aligned, readable up to the next
// multiple of 16 past n_bytes) and byte_off of that decode.  keys [2 * n_seqs], all bytes 0xFF before the launch: per sequence
// the smallest match key, then the smallest proper-prefix tail.  Launched only with n_seqs > 0 and n_bytes > 0.
struct JtkStopWork {
    const uint8_t* out;
    int64_t n_bytes;
    const int64_t* byte_off;    // [n_seqs + 1]
    int64_t n_seqs, n_tiles;    // tiles of JTK_STOP_TILE bytes
    const int64_t* from;        // [n_seqs] or NULL
    const int64_t* cell_byte;   // [n_seqs * width] of the rows decode, or NULL
    int64_t width;
    unsigned long long* keys;
    int64_t* stop_pos;          // [n_seqs] each
    int32_t* stop_which;
    int32_t* hold;
    int64_t* stop_col;
    JtkStopSet set;
};
void jtk_launch_stop_find(const JtkStopWork& w, hipStream_t s);      // find (with strings), then finish
// Compact ids (jtk_compact.hip; the rule is jtk_compact_rules.h): the range [t0, t1) of the int32 stream `ids` (indexed from
// token 0) into a uint16 plane and a plane of hb bits per token whose entry 0 is token `origin` (a multiple of 32; 0 for whole
// planes).  Restarts at t0 rounded down to a multiple of 32 and rewrites the words there whole.  d_total != NULL: the range ends
// at min(t1, *d_total).  hi may be NULL when hb == 0.
void jtk_launch_compact(const int32_t* ids, int64_t t0, int64_t t1, const int64_t* d_total, uint16_t* lo, uint32_t* hi,
                        int64_t origin, int hb, hipStream_t s);
// MinHash (jtk_minhash.hip; the rule is jtk_minhash_rules.h).  sig[n_docs * num_hashes], n_shingles[n_docs] (may be NULL) and
// band_keys[n_docs * bands] (may be NULL: no keys) of the documents of v; three kernels at most, in order on s.
void jtk_launch_minhash(const JtkMhView& v, uint64_t seed, int32_t num_hashes, int32_t bands, uint32_t* sig, int32_t* n_shingles,
                        uint64_t* band_keys, hipStream_t s);
// agree[p] = the words on which rows pair_a[p] and pair_b[p] of sig[n_sig * num_hashes] agree; -1 for an index outside [0, n_sig)
void jtk_launch_minhash_agree(const uint32_t* sig, int64_t n_sig, int32_t num_hashes, const int64_t* pair_a, const int64_t* pair_b,
                              int64_t n_pairs, int32_t* agree, hipStream_t s);
// Token n-gram sets and overlap (jtk_ngram.hip; the rule is jtk_ngram_rules.h).  A set is a table of `capacity` (a power of two)
// 64-bit slots, 0 = empty, and a device word that counts its keys.
//   count         *sum += the n-grams of the documents of v (what an insert of them adds at most)
//   insert        every n-gram of v; *count += the keys that were new
//   insert_keys   keys[n], zeros skipped (so an old table can be given: the rehash); count may be NULL
//   overlap       flags[total], n_hit / n_covered / first_hit [n_docs], each may be NULL and is then not written; two kernels at most
void jtk_launch_ngram_count(const JtkMhView& v, uint64_t* sum, hipStream_t s);
void jtk_launch_ngram_insert(const JtkMhView& v, uint64_t seed, uint64_t* table, int64_t capacity, uint64_t* count, hipStream_t s);
void jtk_launch_ngram_insert_keys(const uint64_t* keys, int64_t n, uint64_t* table, int64_t capacity, uint64_t* count_or_null, hipStream_t s);
void jtk_launch_ngram_overlap(const JtkMhView& v, uint64_t seed, const uint64_t* table, int64_t capacity, uint8_t* flags, int32_t* n_hit,
                              int32_t* n_covered, int64_t* first_hit, hipStream_t s);
// Repeated n-grams inside a document (jtk_repeat.hip; the rule is jtk_repeat_rules.h).  `top` is the batch's packed word per document.
//   preset        n_repeat = n_covered = 0 and top = 0 for every document; each may be NULL
//   group         the two passes over the token range [lo, hi) of a group of whole documents, with a table preset by the caller
//                 (key and count 0, first all ones); tok_flags / n_repeat / n_covered / top may each be NULL
//   top           top_count and top_first out of the packed words
struct JtkRpTable;
void jtk_launch_repeat_preset(int64_t n_docs, int32_t* n_repeat, int32_t* n_covered, uint64_t* top, hipStream_t s);
void jtk_launch_repeat_group(const JtkMhView& v, uint64_t seed, uint64_t doc_index_base, uint32_t flags, const JtkRpTable& t, int64_t lo, int64_t hi,
                             uint8_t* tok_flags, int32_t* n_repeat, int32_t* n_covered, uint64_t* top, hipStream_t s);
void jtk_launch_repeat_top(int64_t n_docs, const uint64_t* top, int32_t* top_count, int64_t* top_first, hipStream_t s);
// Duplicate lines and paragraphs inside a document (jtk_lines.hip; the rule and the way the text is walked are jtk_lines_rules.h).
// edge / ref: the two bit planes over the text, preset to 0, (tiles * 256 + 2) * 2 bytes each; sum_*: pass A's summary per tile;
// tile_*: pass B's carries per tile; doc_units / doc_chars [n_docs + 1]: the units and chars before the document that starts at a
// position (entries of empty documents are not used); unit_off / char_off [n_docs + 1]; per unit: begin, end, k (P at the start byte
// until k_ln_keys), chars (the chars before the start byte until then), and P and the chars at the end byte.
struct JtkLnWork {
    const uint8_t* text;
    const int64_t* doc_off;
    const int32_t* status;
    int64_t n_bytes, n_docs, n_units;
    int32_t unit;
    uint32_t flags;
    uint32_t *edge, *ref;
    uint32_t *sum_word, *sum_units, *sum_chars;
    uint64_t* sum_hash;
    uint32_t *tile_cf, *tile_cb;
    int64_t *tile_units, *tile_chars;
    uint64_t* tile_hash;
    int64_t* hdr;
    int64_t *doc_units, *doc_chars, *unit_off, *char_off;
    int64_t *u_begin, *u_end;
    uint64_t* u_k;
    int64_t* u_chars;
    uint64_t* u_pe;
    int64_t* u_ce;
};
struct JtkLnOut {                  // jtk_lines_out of include/jtokkit_amd.h
    int64_t *unit_begin, *unit_end;
    uint8_t* unit_flags;
    int64_t* unit_off;
    int32_t* n_dup;
    int64_t *dup_bytes, *dup_chars, *unit_bytes, *unit_chars, *doc_chars;
    int32_t* top_count;
    int64_t* top_first;
};
//   count         the planes, pass A and pass B: hdr[0] = the units of the batch
//   write         pass C, unit_off / char_off and every unit's k and chars (n_units as counted)
//   preset        the per-document sums and top = 0; unit_off and doc_chars out of the batch's arrays
//   group         the two passes over the units [lo, hi) of a group of whole documents, with a table preset by the caller
int64_t jtk_lines_tiles(int64_t n_bytes);
void jtk_launch_lines_count(const JtkLnWork& w, hipStream_t s);
void jtk_launch_lines_write(const JtkLnWork& w, uint64_t seed, uint64_t doc_index_base, hipStream_t s);
void jtk_launch_lines_preset(const JtkLnWork& w, const JtkLnOut& o, uint64_t* top, hipStream_t s);
void jtk_launch_lines_group(const JtkLnWork& w, uint32_t flags, const JtkRpTable& t, int64_t lo, int64_t hi, const JtkLnOut& o, uint64_t* top,
                            hipStream_t s);
// Device-side state of an allow-special encode (jtk_special.hip, JTK_ENCODE_ALLOW_SPECIAL; the rule is jtk_special_rules.h).
// Candidates (per position, the longest allowed literal there) are found in position order, resolved to the kept matches, and
// the batch is cut into sub-documents that partition the text: per document a segment, then per candidate i two slots
// d + 2i + 1 (its literal) and d + 2i + 2 (the segment after it).  A candidate that is not kept gets two empty slots at the
// start of the next kept match (or the document's end).  The encode pipeline runs on the sub-documents (encodeOrdinary), and
// the stitch writes each document's segment tokens and special ids into the final result.
struct JtkSpecialWork {
    const uint8_t* text;        // the batch text (16-byte aligned, readable up to the next multiple of 16 past n_bytes)
    const int64_t* doc_off;     // [n_docs + 1]
    int64_t n_docs, n_bytes;
    int n_lits;                 // the encoding's special literals: special_off / special_blob of JtkDeviceTables
    const uint32_t* lit_off;
    const uint8_t* lit_blob;
    const uint8_t* allowed;     // [n_lits] literal i is in the allowed set
    const int32_t* lit_id;      // [n_lits] its id
    int64_t maxlen;             // longest allowed literal
    uint32_t check_dis;         // encode(): a literal outside the allowed set anywhere in a document -> JTK_ERR_UNSUPPORTED_SPECIAL
    uint32_t first[8];          // bit b: a literal the find pass looks for starts with byte b
    int64_t* hdr;               // [0] candidates, [1] offsets are bad (not non-decreasing within [0, n_bytes], doc_off[0] != 0),
                                // [2] the find pass has refused a document (a literal outside the allowed set, under encode())
    int64_t* blk;               // [n_blk + 1] candidates per block of JTK_SPECIAL_BLOCK text bytes, then their exclusive scan
    int64_t n_blk;
    int64_t n_cand;             // candidates, in position order:
    int64_t* cand_pos;
    int32_t* cand_len;
    int32_t* cand_id;
    int64_t* cand_doc;
    uint8_t* cand_keep;         // 1 kept for certain, 2 undecided (a chain), then 3 kept / 0 not kept by the walk
    int64_t n_sub;              // n_docs + 2 * n_cand
    int64_t* sub_off;           // [n_sub + 1]
    int32_t* sub_lit;           // [n_sub] -1 segment, -2 empty slot of a candidate not kept, else the special id of a literal
    int64_t* sub_doc;           // [n_sub] its document
    int64_t* doc_first;         // [n_docs] the document's first sub-document
    const int64_t* sub_tok_off; // the pipeline's result on the sub-documents: [n_sub + 1]
    const int32_t* sub_status;  // [n_sub]
    const int32_t* sub_tokens;
    int64_t* cnt;               // [n_sub + 1] tokens per sub-document in the final result, then their exclusive scan
    uint32_t count_only;
    int32_t* status;            // final, [n_docs] (zeroed before the find pass, which records disallowed literals)
    int64_t* tok_off;           // final, [n_docs + 1]
    int32_t* tokens;            // final
    JtkResult* result;          // final (zeroed before the stitch)
};
#define JTK_SPECIAL_BLOCK 4096   // text bytes per find workgroup (256 lanes x 16 bytes)
void jtk_launch_special_find(const JtkSpecialWork& w, hipStream_t s);      // offsets check, candidates per block, scan -> hdr
void jtk_launch_special_write(const JtkSpecialWork& w, hipStream_t s);     // candidates, resolve, sub-documents (needs n_cand)
void jtk_launch_special_stitch(const JtkSpecialWork& w, hipStream_t s);    // status, counts, scan, offsets, ids (after the pipeline)
// Device-side state of a fill-in-the-middle encode (jtk_fim.hip, JTK_ENCODE_FIM; the rule is jtk_fim_rules.h).  Every document
// becomes three sub-documents in text order (prefix, middle, suffix; an untouched document: itself and two empty ones), known
// before anything runs: no find pass and no wait.  The encode pipeline runs on the sub-documents (encodeOrdinary), and the
// stitch writes each document's parts and sentinel ids into the final result in the order of its kind.
struct JtkFimWork {
    const uint8_t* text;        // the batch text
    const int64_t* doc_off;     // [n_docs + 1]
    int64_t n_docs, n_bytes;
    uint64_t seed;
    int64_t doc_index_base;
    uint32_t fim_rate, spm_rate;
    int64_t* hdr;               // [0] != 0: the offsets are bad (not non-decreasing within [0, n_bytes], from 0 to n_bytes)
    uint8_t* kind;              // [n_docs]
    int64_t* cut;               // [n_docs][2] relative to the document
    int64_t* sub_off;           // [3 n_docs + 1]
    const int64_t* sub_tok_off; // the pipeline's result on the sub-documents: [3 n_docs + 1]
    const int32_t* sub_status;  // [3 n_docs]
    int64_t* part_tok;          // [n_docs][3]
    uint32_t count_only;
    int32_t* status;            // final, [n_docs]
    int64_t* tok_off;           // final, [n_docs + 1]: the counts, then their exclusive scan
    int32_t* tokens;            // final
    JtkResult* result;          // final (zeroed before the cuts, which report bad offsets in it)
    JtkFimView v;               // what the gather reads (points at the arrays above and the sub-documents' ids)
};
void jtk_launch_fim_cuts(const JtkFimWork& w, hipStream_t s);      // offsets check, kind, cuts, sub-documents
void jtk_launch_fim_stitch(const JtkFimWork& w, hipStream_t s);    // status, counts, scan, ids (after the pipeline)
void jtk_launch_decode_count(const JtkDecodeWork& w, hipStream_t s);     // mark, count, scan
void jtk_launch_decode_scatter(const JtkDecodeWork& w, hipStream_t s);   // scatter, offsets

// chunk plan of a batch whose offsets are in device memory: out_doc[c], out_off[c] for c = 0..n_chunks
void jtk_launch_plan_chunks(const int64_t* doc_off, int64_t n_docs, int64_t chunk_bytes, int n_chunks, int64_t* out_doc, int64_t* out_off,
                            hipStream_t s);
void jtk_launch_stitch(const int64_t* totals, int rank, int64_t* base_out, const int64_t* tok_off, int64_t n_docs, int64_t* global_off,
                       hipStream_t s);
void jtk_launch_mark_docs(const JtkWork& w, hipStream_t s);
// caller-supplied pieces [begin[i], end[i]) (positions in the whole batch), i = 0..n_pieces-1, instead of pretok_split
void jtk_launch_mark_pieces(const JtkWork& w, const int64_t* begin, const int64_t* end, int64_t n_pieces, hipStream_t s);
void jtk_launch_validate_utf8(const JtkWork& w, hipStream_t s);
void jtk_launch_pretok_split(const JtkWork& w, const JtkDeviceTables& t, hipStream_t s);
void jtk_launch_piece_resolve(const JtkWork& w, const JtkDeviceTables& t, hipStream_t s);
void jtk_launch_long_shortcut(const JtkWork& w, const JtkDeviceTables& t, hipStream_t s);     // only if t.longtok.n
void jtk_launch_bpe_merge(const JtkWork& w, const JtkDeviceTables& t, hipStream_t s);
void jtk_launch_tile_scan(const JtkWork& w, hipStream_t s);
void jtk_launch_pack(const JtkWork& w, hipStream_t s);
void jtk_launch_doc_offsets(const JtkWork& w, hipStream_t s);
void jtk_launch_flag_unencodable(const JtkWork& w, uint32_t pseudo_base, hipStream_t s);

#endif
