/* jtokkit_amd.h -- C ABI of the MI355X-native batch BPE encoder.
 *
 * This is the drop-in boundary for ONE path of JTokkit (reference at /root/reference, paths below
 * relative to lib/src/main/java/com/knuddels/jtokkit/): GptBytePairEncoding.encode() and its
 * callers in the Encoding interface.  The reference has no FFI of its own; these are the entry
 * points a JNI shim behind `com.knuddels.jtokkit.api.Encoding` binds (see INTEGRATION.md for the
 * Java/JNI side).  Plain C: pointers and sizes only, no C++/torch types.
 *
 * Threading (api/EncodingRegistry.java:51,61 "The encoding must be thread-safe"): a jtk_encoding
 * is immutable after creation and may be shared by any number of threads.  A jtk_batch owns one
 * HIP stream plus its device scratch and must be used by one thread at a time; create one per
 * caller thread.
 *
 * Every function that returns int returns JTK_OK (0) or a negative jtk_status.  The message of the
 * last failure on the calling thread is available from jtk_last_error().
 */
#ifndef JTOKKIT_AMD_H
#define JTOKKIT_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Status codes; the comment names the exception the Java shim raises for it. */
typedef enum jtk_status {
    JTK_OK = 0,
    JTK_ERR_INVALID_ARGUMENT = -1,    /* IllegalArgumentException (bad call) */
    JTK_ERR_UNSUPPORTED_SPECIAL = -2, /* UnsupportedOperationException("Encoding special tokens is not
                                         supported yet.")  GptBytePairEncoding.java:52-56 */
    JTK_ERR_UNKNOWN_TOKEN = -3,       /* IllegalArgumentException("Unknown token for decoding: " + id)
                                         GptBytePairEncoding.java:313 */
    JTK_ERR_CAPACITY = -4,            /* caller buffer too small (shim grows and retries) */
    JTK_ERR_BAD_RANK_FILE = -5,       /* IllegalStateException  EncodingFactory.java:142,151,162 */
    JTK_ERR_BAD_UTF8 = -6,            /* input is not what String.getBytes(UTF_8) produces */
    JTK_ERR_NO_DEVICE = -7,           /* no MI355X / HIP runtime: there is NO CPU fallback */
    JTK_ERR_HIP = -8,                 /* a HIP call failed; see jtk_last_error() */
    JTK_ERR_UNSUPPORTED_TABLE = -9,   /* rank table outside what the device path handles (see
                                         jtk_encoding_create) */
    JTK_ERR_PIECE_TOO_LONG = -10,     /* a single unsplittable pre-token piece exceeds JTK_MAX_PIECE_BYTES (1 MiB;
                                         the reference spends O(n^2) on such a piece) */
    JTK_ERR_OUT_OF_MEMORY = -11,
    JTK_ERR_UNENCODABLE = -12         /* IllegalArgumentException("Unknown token for encoding: ...") TokenEncoder.java:66-68: the rank
                                         map lacks a single-byte token and a piece of this document needs it */
} jtk_status;

/* The two split patterns of EncodingFactory.java:63 (= :77, :91) and :105. */
enum { JTK_PATTERN_R50K = 0, JTK_PATTERN_CL100K = 1 };

/* Flags of jtk_batch_encode*. */
enum {
    JTK_ENCODE_ORDINARY = 1u,     /* encodeOrdinary(): skip the special-token check of encode()
                                     (GptBytePairEncoding.java:62-64 vs :47-59) */
    JTK_ENCODE_VALIDATE_UTF8 = 2u,/* also check every document is well-formed UTF-8 (what String.getBytes(UTF_8)
                                     produces); offenders get status JTK_ERR_BAD_UTF8.  Without the flag the
                                     input is trusted: malformed bytes are encoded as the bytes they are.  The flag
                                     changes nothing but the status: an offender's tokens and offsets are those of the
                                     call without it (under JTK_ENCODE_ALLOW_SPECIAL and JTK_ENCODE_FIM an offender has no tokens).  An empty
                                     document is never an offender.  When two codes apply to one document -- under
                                     encode() it holds a special-token literal and a malformed byte -- its status is the
                                     lower one, JTK_ERR_BAD_UTF8.  The rule: jtokkit_amd/csrc/jtk_validate_rules.h */
    JTK_ENCODE_COUNT_ONLY = 4u,   /* Encoding.countTokens() / countTokensOrdinary() (GptBytePairEncoding.java:122-129) for
                                     the whole batch: token offsets (tok_off[d + 1] - tok_off[d] = the count) and
                                     status, but no token ids -- fetch with tokens == NULL */
    JTK_ENCODE_TO_HOST = 8u,      /* jtk_batch_encode / jtk_batch_encode_pieces only: stream the result to pinned host
                                     memory while later chunks are still being encoded; read it in place with
                                     jtk_batch_host_result() */
    JTK_ENCODE_ALLOW_SPECIAL = 16u,/* jtk_batch_encode / jtk_batch_encode_device only: the batch's allowed special-token
                                     literals are encoded as their ids (jtk_batch_set_allowed_special has the rule);
                                     every other entry point that takes flags returns JTK_ERR_INVALID_ARGUMENT for it */
    JTK_ENCODE_COMPACT_IDS = 32u, /* jtk_batch_encode / jtk_batch_encode_pieces, only together with JTK_ENCODE_TO_HOST: the ids
                                     reach pinned host memory as a 16-bit plane plus a plane of the bits above ("compact
                                     token ids" below) -- 2 to 2.125 bytes per token over the link instead of 4; read them
                                     with jtk_batch_host_result_compact().  Anywhere else: JTK_ERR_INVALID_ARGUMENT */
    JTK_ENCODE_FIM = 64u          /* jtk_batch_encode / jtk_batch_encode_device only, together with JTK_ENCODE_ORDINARY and
                                     without JTK_ENCODE_ALLOW_SPECIAL: the fill-in-the-middle transformation by the batch's
                                     parameters (jtk_batch_set_fim has the rule); every other entry point that takes flags
                                     returns JTK_ERR_INVALID_ARGUMENT for it */
};

/* Options of jtk_batch_set_option.  A batch larger than one chunk is cut into runs of whole documents ("chunks") that flow
 * through a few scratch sets, each on its own HIP stream: the copies and kernels of consecutive chunks overlap, and the
 * device scratch is sized by the chunk, not by the batch. */
enum {
    JTK_OPT_CHUNK_BYTES = 1,      /* target bytes of text per chunk, device-resident input (default 1 GiB: large chunks
                                     have fewer launches and kernel tails; env JTK_CHUNK_BYTES).  Scratch: ~30 bytes per
                                     byte of chunk per set */
    JTK_OPT_CHUNKS_IN_FLIGHT = 2, /* scratch sets / streams, 1..4 (default 2, and 3 for host input with JTK_ENCODE_TO_HOST unless chosen
                                     here or by env JTK_CHUNKS_IN_FLIGHT: the host waits once per chunk there, two sets stall) */
    JTK_OPT_HOST_CHUNK_BYTES = 3, /* ... host input (default 32 MiB: the copy of one chunk overlaps the kernels of another;
                                     env JTK_HOST_CHUNK_BYTES) */
    JTK_OPT_REUSE_CHUNK_PLAN = 4, /* 1: jtk_batch_encode_device keeps the chunk plan of the last batch while it is handed the same
                                     offsets array again (same pointer and counts: a step loop) -- no plan kernel, no host
                                     synchronisation in the call.  The caller promises not to change those offsets in place
                                     (if it does: JTK_ERR_INVALID_ARGUMENT as the batch's worst status, never wrong tokens).
                                     Default 0 */
    JTK_OPT_REPEAT_TABLE_BYTES = 5 /* jtk_batch_ngram_repeats: the budget in bytes for the table of one group of documents (20
                                     bytes per slot, two slots per n-gram rounded up to a power of two); at least 1280 (64
                                     slots).  A document that needs more is a group of its own with the table it needs.
                                     Results never depend on it.  Default 256 MiB */
};

typedef struct jtk_encoding jtk_encoding;
typedef struct jtk_batch jtk_batch;

const char* jtk_version(void);
const char* jtk_last_error(void);
/* Number of visible HIP devices, or a negative status. */
int jtk_device_count(void);

/* ---- encoding objects -------------------------------------------------------------------------
 * Replaces EncodingFactory.fromPredefinedParameters (:121-137) + the GptBytePairEncoding
 * constructor (GptBytePairEncoding.java:30-35): parses the `.tiktoken` bytes ("base64 SP rank LF",
 * EncodingFactory.java:139-164), builds the device rank tables and uploads them to `device`.
 * `special_literals[i]` / `special_ids[i]` are the special tokens (EncodingFactory.java:24-53).
 *
 * Tables accepted: any rank map with ids < 131071 (JTK_ERR_UNSUPPORTED_TABLE otherwise).  A map that lacks single-byte tokens
 * is taken as the reference takes it: a document with a piece whose merge leaves such a byte alone gets JTK_ERR_UNENCODABLE
 * (TokenEncoder.java:66-68 throws there); it needs one free id above the table's largest per missing byte.  With a token limit
 * the status is conservative: a document is refused when such a piece lies anywhere in the bytes that were encoded (the whole
 * document, or its leading bytes in jtk_batch_encode_max_tokens), where the reference refuses it only if the piece starts
 * before the limit is reached.  The whole-piece lookup of
 * GptBytePairEncoding.java:81-83 is honoured for pieces of any length: for tables in which merging a token's bytes
 * reproduces the token (every table trained by byte-pair merging; the three shipped ones) it is a pure shortcut, for others
 * the unreproducible entries get a lookup of their own and the exact intra-piece cuts are switched off.
 * Special tokens: any number of literals of any length >= 1 (any first byte), ids < 2^25 (the decode table is dense: 4 bytes
 * of device memory per id up to the largest). */
int jtk_encoding_create(const char* name, int pattern_kind, const uint8_t* tiktoken, size_t tiktoken_len,
                        const char* const* special_literals, const int32_t* special_ids, int n_specials,
                        int device, jtk_encoding** out);
void jtk_encoding_destroy(jtk_encoding* enc);
const char* jtk_encoding_name(const jtk_encoding* enc);          /* Encoding.getName() */
int jtk_encoding_device(const jtk_encoding* enc);
int64_t jtk_encoding_vocab_size(const jtk_encoding* enc);        /* number of rank-table entries */
int64_t jtk_encoding_pair_count(const jtk_encoding* enc);        /* (left,right) -> rank entries */
int jtk_encoding_id_bits(const jtk_encoding* enc);               /* 16 + hb of "compact token ids" below: 16, 17, 18, 20, 24 or 32 */

/* ---- batch encode: the hot path ------------------------------------------------------------------
 * Replaces a loop of Encoding.encode(String) / encodeOrdinary(String) / countTokens(String)
 * (GptBytePairEncoding.java:38-40, 62-64, 122-129) over n_docs documents.
 *
 * Input: the documents' String.getBytes(UTF_8) bytes back to back in `utf8`, document d occupying
 * [doc_off[d], doc_off[d+1]) (doc_off[0] = 0, doc_off[n_docs] = total bytes).
 * Output (after jtk_batch_fetch / in device memory): token ids of all documents back to back in
 * document order, document d occupying [tok_off[d], tok_off[d+1]); status[d] = JTK_OK or
 * JTK_ERR_UNSUPPORTED_SPECIAL / JTK_ERR_BAD_UTF8 / JTK_ERR_PIECE_TOO_LONG for that document.
 *
 * What a batch holds: the result of its last encode and what was derived from it (truncation, chunks, the byte scan, pack,
 * the character index), and the result of its last decode and what was derived from that (UTF-16 units, stops).  Every
 * encode entry point drops the first group, every decode entry point the second, at its point of no return: behind the checks
 * that read only the arguments, before anything the old result lives in is touched.  So a call refused for its arguments
 * leaves the batch as it was, and a call that fails past that point leaves no result: the calls that read one return
 * JTK_ERR_INVALID_ARGUMENT until the next encode (decode) succeeds.
 */
int jtk_batch_create(const jtk_encoding* enc, jtk_batch** out);
void jtk_batch_destroy(jtk_batch* b);
int jtk_batch_set_option(jtk_batch* b, int option, int64_t value);

/* Page-locked host memory (hipHostMalloc).  Host buffers handed to jtk_batch_encode are copied by DMA straight from
 * where they are when they were allocated here (what a Java shim does for its direct ByteBuffers); pageable memory
 * works too but is staged by the HIP runtime at a fraction of the link's rate. */
int jtk_host_alloc(size_t bytes, void** out);
void jtk_host_free(void* p);

/* Host buffers: copies the input to the device chunk by chunk (the copy of a chunk overlaps the kernels of the one
 * before), runs the kernels, leaves the result on the device (and, with JTK_ENCODE_TO_HOST, in pinned host memory).
 * *n_tokens receives the total token count (this call synchronises). */
int jtk_batch_encode(jtk_batch* b, const uint8_t* utf8, const int64_t* doc_off, int64_t n_docs,
                     uint32_t flags, int64_t* n_tokens);

/* Custom split patterns (api/GptBytePairEncodingParams.java:36-46: any java.util.regex.Pattern).  Only the two shipped
 * patterns are evaluated on the device; for any other one the caller runs its own matcher on the host and hands over the
 * matches: piece i is utf8[piece_begin[i], piece_end[i]) (positions in the whole batch; ascending, non-empty, not
 * overlapping, each inside one document).  Bytes that no piece covers are not encoded, as `while (matcher.find())`
 * (GptBytePairEncoding.java:79) skips them.  Whole-piece shortcut, bytePairMerge, token order, offsets, status, flags
 * and results are as for jtk_batch_encode (the special-token check of encode() is done on the host here). */
int jtk_batch_encode_pieces(jtk_batch* b, const uint8_t* utf8, const int64_t* doc_off, int64_t n_docs,
                            const int64_t* piece_begin, const int64_t* piece_end, int64_t n_pieces, uint32_t flags, int64_t* n_tokens);

/* After an encode with JTK_ENCODE_TO_HOST: the result in the batch's pinned host buffers (valid until the next encode
 * on this batch): tokens[n_tokens], tok_off[n_docs + 1], status[n_docs]. */
int jtk_batch_host_result(jtk_batch* b, const int32_t** tokens, const int64_t** tok_off, const int32_t** status);

/* ---- compact token ids: a 16-bit plane plus a plane of the bits above ---------------------------------------------------
 * The format (jtokkit_amd/csrc/jtk_compact_rules.h).  max_id = the largest id a result of the encoding can hold: its rank
 * table's largest id, the pseudo ids of single bytes the table lacks (they stay in the result; their document gets
 * JTK_ERR_UNENCODABLE) and every special id.  hb = the smallest of {0, 1, 2, 4, 8, 16} with max_id < 2^(16 + hb);
 * jtk_encoding_id_bits() = 16 + hb.  A compact result of n tokens is
 *   lo  uint16[n]                  lo[i] = id[i] & 0xFFFF
 *   hi  uint32[ceil(n * hb / 32)]  token i's hb bits (id[i] >> 16) at bit (i * hb) % 32 of word (i * hb) / 32, little-endian
 *                                  bit order; the unused bits of the last word are zero; absent (NULL) when hb == 0
 * and tok_off / status as ever (token indices: they address both planes).  r50k_base, p50k_base, p50k_edit: hb = 0, and lo
 * alone is the uint16 token shard GPT-2-style loaders read; cl100k_base: hb = 1 (2.125 bytes per token).  Widening gives back
 * exactly the int32 ids of the plain result.
 *
 * jtk_batch_host_result_compact: after jtk_batch_encode / _encode_pieces with JTK_ENCODE_TO_HOST | JTK_ENCODE_COMPACT_IDS, the
 *   planes in the batch's pinned host buffers (valid until the next encode on this batch); lo and hi are NULL after a
 *   count-only encode.  Each chunk's id range is compacted on the device behind the chunk's kernels and its two plane ranges
 *   copied up, one chunk behind the kernels like the int32 copy of the plain route; the pinned buffers are sized and grown by
 *   the compact sizes.  JTK_ENCODE_ALLOW_SPECIAL, JTK_ENCODE_VALIDATE_UTF8 and JTK_ENCODE_COUNT_ONLY compose with the flag.
 *   The device-side result stays int32: jtk_batch_fetch, jtk_batch_device_result, jtk_batch_chunk, jtk_batch_pack,
 *   jtk_batch_truncate and jtk_batch_token_offsets work as after the plain encode.  jtk_batch_host_result returns
 *   JTK_ERR_INVALID_ARGUMENT after such an encode (host memory holds no int32 ids).  jtk_encode and the service do not take
 *   the flag.
 * jtk_batch_compact: the planes of the LAST batch encode on `b` (host- or device-input, any flags but JTK_ENCODE_COUNT_ONLY:
 *   JTK_ERR_INVALID_ARGUMENT then, and with no result) into caller-owned device buffers: d_lo[n_tokens] uint16,
 *   d_hi[ceil(n_tokens * hb / 32)] uint32 (may be NULL when hb == 0).  Waits once, for the token count (as jtk_batch_result);
 *   the pass is then queued behind the encode on stream_or_null (a hipStream_t), or on the batch's stream when it is NULL, and
 *   the call does not wait for it.  It reads the ids only: chunk, pack and truncate results are untouched.  16-byte aligned
 *   buffers take the fast path.
 * jtk_widen_ids: out[k] = id of token first + k for k < n, on the host, from planes as above (id_bits = 16 + hb) -- any range,
 *   so that a caller widens one document at a time: first = tok_off[d], n = tok_off[d + 1] - tok_off[d]. */
int jtk_batch_host_result_compact(jtk_batch* b, const uint16_t** lo, const uint32_t** hi, int* id_bits, const int64_t** tok_off,
                                  const int32_t** status);
int jtk_batch_compact(jtk_batch* b, uint16_t* d_lo, uint32_t* d_hi, void* stream_or_null);
int jtk_widen_ids(const uint16_t* lo, const uint32_t* hi, int id_bits, int64_t first, int64_t n, int32_t* out_int32);

/* MinHash signatures and LSH band keys over the token n-grams of the last batch encode, for near-duplicate detection
 * (jtk_minhash.hip; the rule, bit for bit, is csrc/jtk_minhash_rules.h -- integer arithmetic only, so every result is exact).
 *   With G = 0x9E3779B97F4A7C15, mix = the splitmix64 finaliser (as for jtk_fim_params), key = mix(seed + G * (ngram + 1)) and
 *   draw(j) = mix(key + j), all modulo 2^64: a document of l tokens (l = 0 when its status < 0) has the shingles t[i .. i + m),
 *   m = min(ngram, l), 0 <= i <= l - m (none when l == 0; a document shorter than ngram is one shingle); H = H * G + id + 1
 *   over a shingle's ids (as uint32: special ids, FIM sentinels and pseudo ids count), x = the low 32 bits of mix(H ^ key);
 *   sig[d][k] = min over the shingles of ((a_k * x + b_k) mod 2^64) >> 32 with a_k = draw(2k + 1) | 1, b_k = draw(2k + 2), and
 *   0xFFFFFFFF without shingles; band_key[d][j] = h after h = draw(2^32 + j) and h = mix(h ^ v) for the r = num_hashes / bands
 *   words v of band j in order.  The number of k on which two rows agree, over num_hashes, estimates the Jaccard similarity
 *   of the two shingle sets.
 *   A signature depends on (seed, ngram, num_hashes, the document's ids) alone -- not on the batch, the document's index or
 *   the device --, so the shards of a corpus agree by construction and their rows can be gathered into one array.
 * jtk_batch_minhash: works on the LAST batch encode on `b` (host or device input, any flags but JTK_ENCODE_COUNT_ONLY:
 *   JTK_ERR_INVALID_ARGUMENT then, and with no result).  ngram 1..32, num_hashes 1..256, bands 0 (no keys) or a divisor of
 *   num_hashes, flags 0: anything else is JTK_ERR_INVALID_ARGUMENT.  Caller-owned device buffers: d_sig[n_docs * num_hashes]
 *   uint32, d_n_shingles[n_docs] int32 (may be NULL), d_band_keys[n_docs * bands] uint64 (may be NULL, also with bands > 0:
 *   keys are then not computed).  Waits once, for the token count (as jtk_batch_compact); the pass is then queued behind the
 *   encode on stream_or_null, or on the batch's stream when it is NULL, and the call does not wait for it.  It reads the ids,
 *   tok_off and status only and keeps no state in the batch: chunk, pack, truncate and FIM results are untouched.
 * jtk_batch_minhash_agree: d_agree[p] = the number of k < num_hashes with d_sig[d_pair_a[p]][k] == d_sig[d_pair_b[p]][k] for
 *   rows of d_sig[n_sig * num_hashes] -- which may hold signatures gathered from many batches; `b` gives the device and the
 *   default stream only, no encode is needed --, or -1 where an index is outside [0, n_sig): no row is read for such a pair.
 *   Queued, does not wait. */
typedef struct jtk_minhash_params {
    uint64_t seed;
    int32_t ngram;          /* n: 1..32 */
    int32_t num_hashes;     /* K: 1..256 */
    int32_t bands;          /* 0 = no band keys; otherwise divides num_hashes */
    uint32_t flags;         /* 0 */
} jtk_minhash_params;
int jtk_batch_minhash(jtk_batch* b, const jtk_minhash_params* params, uint32_t* d_sig, int32_t* d_n_shingles_or_null,
                      uint64_t* d_band_keys_or_null, void* stream_or_null);
int jtk_batch_minhash_agree(jtk_batch* b, const uint32_t* d_sig, int64_t n_sig, int32_t num_hashes, const int64_t* d_pair_a,
                            const int64_t* d_pair_b, int64_t n_pairs, int32_t* d_agree, void* stream_or_null);

/* Token n-gram sets and overlap, for benchmark decontamination: a corpus document is flagged, and the exact token ranges are
 * marked, where it shares a token n-gram with a set of held-out texts encoded by the same encoder (jtk_ngram.hip; the rule, bit
 * for bit, is csrc/jtk_ngram_rules.h -- integer arithmetic only, so every result is exact).
 *   With G and mix as for jtk_minhash_params and key = mix(seed + G * (ngram + 33)), all modulo 2^64: a document of l tokens has
 *   the n-grams t[i .. i + ngram), 0 <= i <= l - ngram -- none when l < ngram (not MinHash's short-document rule) and none when
 *   its status < 0 --; H = H * G + id + 1 over an n-gram's ids (as uint32: special ids, FIM sentinels and pseudo ids count) and
 *   k = mix(H ^ key), G where that is 0.  The set is the distinct k inserted so far (a 64-bit collision is part of the rule),
 *   kept on the device in a table of `capacity` 64-bit slots, a power of two: home slot k & (capacity - 1), linear probing with
 *   wrap-around, 0 = empty.  Before an insert of at most m new keys into c keys the capacity grows to the smallest power of two
 *   >= max(64, 2 (c + m)) when that is larger (the table is rehashed on the device; it never shrinks); m = n for add_keys, the
 *   number of n-grams of the batch's documents for add_batch.  A new set has 64 slots.
 *   Per token p of a document: JTK_NG_START when an n-gram starts at p and its k is in the set, JTK_NG_COVERED when a
 *   start-flagged i of the same document has p - ngram < i <= p.  Per document: n_hit = the start flags, n_covered = the
 *   covered tokens, first_hit = the document-relative index of the first start, or -1.
 * jtk_ngram_set_create: an empty set on enc's device.  ngram 1..32, flags 0: anything else is JTK_ERR_INVALID_ARGUMENT.  A set
 *   belongs to `enc` (which must outlive it) and takes batches of that encoding object only; it holds no reference to any batch:
 *   destroying a batch, or encoding on it again, leaves the set as it is.  Calls on one set are not thread-safe.
 * jtk_ngram_set_destroy: waits for the set's queued work; NULL is allowed.
 * jtk_ngram_set_add_batch: inserts every n-gram of the LAST batch encode on `b` (host or device input, any flags but
 *   JTK_ENCODE_COUNT_ONLY).  Waits for the token count (as jtk_batch_minhash) and once more for the set's key count and the
 *   batch's n-gram count, which decide the capacity; the insert is then queued on stream_or_null (the batch's stream when NULL),
 *   behind the encode and behind the set's earlier work, and the call does not wait for it.
 * jtk_ngram_set_add_keys: inserts n keys from host memory -- the jtk_ngram_set_keys of a saved set or of another shard's --; a key
 *   that is already in the set is not counted again.  n < 0, keys == NULL with n > 0, and a key of 0 are
 *   JTK_ERR_INVALID_ARGUMENT (the set is then unchanged).  Waits until the keys are in.
 * jtk_ngram_set_size: the number of distinct keys and the capacity (either may be NULL); waits for the set's queued work.
 * jtk_ngram_set_keys: the n_keys keys into keys[cap], in no particular order; cap < n_keys is JTK_ERR_INVALID_ARGUMENT.  Waits.
 * jtk_batch_ngram_overlap: the last batch encode on `b` against `s`, with the set's seed and ngram.  Caller-owned device buffers,
 *   each may be NULL and is then not written: d_tok_flags[n_tokens] uint8 (any alignment; 8-byte aligned takes the fast path),
 *   d_n_hit[n_docs] and d_n_covered[n_docs] int32 (4-byte aligned), d_first_hit[n_docs] int64 (8-byte aligned).  An empty set
 *   is valid: all flags 0, all counts 0, first_hit -1.  Waits once, for the token count; the pass is then queued on
 *   stream_or_null (the batch's stream when NULL) behind the encode and the set's earlier work, and the call does not wait for
 *   it.  It reads the ids, tok_off and status only and keeps no state in the batch: chunk, pack, truncate and FIM results are
 *   untouched.  A later jtk_ngram_set_add_* is ordered behind it.  A NULL set and a batch of another encoding object than the
 *   set's are JTK_ERR_INVALID_ARGUMENT.  jtk_batch_token_offsets turns the covered token runs into byte spans. */
#define JTK_NG_START 1
#define JTK_NG_COVERED 2
typedef struct jtk_ngram_params {
    uint64_t seed;
    int32_t ngram;          /* n: 1..32 */
    uint32_t flags;         /* 0 */
} jtk_ngram_params;
typedef struct jtk_ngram_set jtk_ngram_set;
int jtk_ngram_set_create(const jtk_encoding* enc, const jtk_ngram_params* params, jtk_ngram_set** out);
void jtk_ngram_set_destroy(jtk_ngram_set* s);
int jtk_ngram_set_add_batch(jtk_ngram_set* s, jtk_batch* b, void* stream_or_null);
int jtk_ngram_set_add_keys(jtk_ngram_set* s, const uint64_t* keys, int64_t n);
int jtk_ngram_set_size(const jtk_ngram_set* s, int64_t* n_keys, int64_t* capacity);
int jtk_ngram_set_keys(const jtk_ngram_set* s, uint64_t* keys, int64_t cap);
int jtk_batch_ngram_overlap(jtk_batch* b, const jtk_ngram_set* s, uint8_t* d_tok_flags_or_null, int32_t* d_n_hit_or_null,
                            int32_t* d_n_covered_or_null, int64_t* d_first_hit_or_null, void* stream_or_null);

/* Repeated token n-grams inside a document: the repetition filters of Gopher (Rae et al. 2021, table A1; RedPajama-v2, Dolma,
 * FineWeb / datatrove) on the ids of the last batch encode (jtk_repeat.hip; the rule, bit for bit, is csrc/jtk_repeat_rules.h --
 * integer arithmetic only, so every result is exact).
 *   With G and mix as for jtk_minhash_params, all modulo 2^64: key = mix(seed + G * (ngram + 97)) (MinHash has ngram + 1, the
 *   n-gram set ngram + 33: no shared key family) and key_D = mix(key + G * (D + 1)), D = doc_index_base + d for document d of the
 *   batch (doc_index_base as in jtk_fim_params: a shard gives what the whole corpus would).  A document of l tokens has the
 *   n-grams t[i .. i + ngram), 0 <= i <= l - ngram -- none when l < ngram, none when its status < 0 whatever tokens the encode
 *   left it --; H = H * G + id + 1 over an n-gram's ids (as uint32) and k = mix(H ^ key_D), G where that is 0.  Two n-grams of
 *   one document are the same when their k are equal (a 64-bit collision inside a document is part of the rule); n-grams of
 *   different documents are never compared.  first(i) = the smallest document-relative position with the k of the n-gram at i,
 *   count(i) = the number of positions with it.
 *   Per token p: JTK_RP_START when an n-gram starts at p and is a repeat, JTK_RP_COVERED when a start-flagged i of the same
 *   document has p - ngram < i <= p.  A repeat: first(p) < p (a later occurrence); with JTK_REPEAT_MARK_FIRST: count(p) >= 2, so
 *   the first occurrence is marked as well (as RedPajama-v2 counts it).  datatrove's variant, which skips ngram tokens ahead
 *   behind every repeat it finds, is sequential in the document and not offered.
 *   Per document: n_repeat = the start flags, n_covered = the covered tokens, top_count = the largest count over its n-grams (0
 *   without any), top_first = the smallest first among the n-grams with that count (-1 without any).  Gopher's top-n-gram
 *   fraction is top_count * ngram / l, its duplicate-n-gram fraction n_covered / l.
 *   Deviation: the device keeps the n-grams of a group of documents in one table keyed by k alone, so two n-grams of different
 *   documents with equal k (different key_D: probability 2^-64 per pair) would be conflated; for a table of m n-grams at most
 *   m^2 / 2^65 such pairs are expected -- the order of the false-hit rate the n-gram set accepts.
 * jtk_batch_ngram_repeats: works on the LAST batch encode on `b` (host or device input, any flags but JTK_ENCODE_COUNT_ONLY:
 *   JTK_ERR_INVALID_ARGUMENT then, and with no result).  ngram 1..32, flags 0 or JTK_REPEAT_MARK_FIRST: anything else is
 *   JTK_ERR_INVALID_ARGUMENT, as is a document of 2^31 tokens or more.  Caller-owned device buffers, each may be NULL and is then
 *   not written: d_tok_flags[n_tokens] uint8 (any alignment; 8-byte aligned takes the fast path), d_n_repeat[n_docs],
 *   d_n_covered[n_docs] and d_top_count[n_docs] int32 (4-byte aligned), d_top_first[n_docs] int64 (8-byte aligned); a misaligned
 *   one is JTK_ERR_INVALID_ARGUMENT.  A refused call writes nothing.  The batch is walked in groups of whole consecutive
 *   documents that share one table (20 bytes per slot; capacity the smallest power of two >= max(64, 2 * the group's n-grams)): a
 *   group takes documents while its table stays within JTK_OPT_REPEAT_TABLE_BYTES, a document larger than that is a group of its
 *   own.  The table belongs to the batch, is reused by later calls and freed with it; when it cannot be allocated the call
 *   returns JTK_ERR_OUT_OF_MEMORY and nothing has been written.  Results never depend on the grouping.
 *   Waits twice: for the token count (as jtk_batch_minhash), and for the documents' token offsets and statuses, from which the
 *   groups are planned; the passes are then queued on stream_or_null (the batch's stream when NULL) behind the encode and
 *   behind an earlier call's passes, and the call does not wait for them.  It reads the ids, tok_off and status only: chunk,
 *   pack, truncate, FIM and fetch results are untouched. */
#define JTK_RP_START 1
#define JTK_RP_COVERED 2
#define JTK_REPEAT_MARK_FIRST 1u
typedef struct jtk_repeat_params {
    uint64_t seed;
    uint64_t doc_index_base;
    int32_t ngram;          /* n: 1..32 */
    uint32_t flags;         /* 0 or JTK_REPEAT_MARK_FIRST */
} jtk_repeat_params;        /* 24 bytes */
int jtk_batch_ngram_repeats(jtk_batch* b, const jtk_repeat_params* params, uint8_t* d_tok_flags_or_null, int32_t* d_n_repeat_or_null,
                            int32_t* d_n_covered_or_null, int32_t* d_top_count_or_null, int64_t* d_top_first_or_null, void* stream_or_null);

/* Duplicate lines and paragraphs inside a document: the line-level half of Gopher's repetition filters (Rae et al. 2021, table
 * A1; RedPajama-v2, Dolma, FineWeb / datatrove) on the TEXT of the last batch encode (jtk_lines.hip; the rule, bit for bit, is
 * csrc/jtk_lines_rules.h -- integer arithmetic only, so every result is exact).
 *   Text: document d of the batch is the bytes x[a, e), a = doc_off[d], e = doc_off[d + 1].  A document with status < 0 has no
 *   units, whatever its text.  Parameters: seed, doc_index_base, unit = JTK_LINES_LINE (0) or JTK_LINES_PARAGRAPH (1), flags out
 *   of JTK_LINES_MARK_FIRST (1u) and JTK_LINES_TRIM (2u); anything else is JTK_ERR_INVALID_ARGUMENT.
 *   Bytes: the only line break is 0x0A.  W, the blank set, is empty without JTK_LINES_TRIM and {0x20, 0x09, 0x0D} with it.  A byte
 *   is INK when it is neither 0x0A nor in W.
 *   Units: a raw line is a maximal run of bytes of the document without 0x0A (the document's start and end bound raw lines:
 *   nothing crosses a document edge); it is blank when it has no ink.  LINE: for each non-blank raw line, [its first ink byte, its
 *   last ink byte + 1).  PARAGRAPH: for each maximal run of consecutive non-blank raw lines, [the first ink byte of the first
 *   line, the last ink byte of the last line + 1); the bytes in between, line breaks and blanks included, are part of the unit
 *   unchanged.  Per byte, equivalently: an ink byte p starts a unit when its document has no earlier ink byte, or when the number
 *   of 0x0A between the previous ink byte and p is >= 1 (LINE) or >= 2 (PARAGRAPH); it ends a unit when the same holds towards
 *   the next ink byte, or there is none.
 *   What this matches: without TRIM, re.split("\n+") for LINE and re.split("\n{2,}") for PARAGRAPH on a document stripped of
 *   leading and trailing newlines -- what datatrove's Gopher repetition filter does after strip().  With TRIM, CRLF text and lines
 *   that differ only in indentation or trailing blanks behave as RedPajama-v2's normalised lines do.  No more is claimed.
 *   Hash, all modulo 2^64, G and mix as for jtk_minhash_params: key = mix(seed + G * (unit + 161)) (MinHash has ngram + 1, the
 *   n-gram set ngram + 33, n-gram repeats ngram + 97, ngram <= 32: no shared key family), key_D = mix(key + G * (D + 1)), D =
 *   doc_index_base + d (as for jtk_repeat_params: a shard gives what the whole corpus would).  H = H * G + byte + 1 over the
 *   unit's bytes, from 0; k = mix(H ^ key_D), G where that is 0.  Two units of ONE document are the same when their k are equal
 *   (a 64-bit collision inside a document is part of the rule); units of different documents are never compared.
 *   Per unit u, over a document's units in text order: first(u) = the smallest document-relative index with u's k, count(u) = the
 *   number of units with it.  A repeat: first(u) < u (a later occurrence); with JTK_LINES_MARK_FIRST: count(u) >= 2.  chars of a
 *   byte range = its bytes b with (b & 0xC0) != 0x80 (the weight of JTK_UNIT_CODEPOINT; defined for any bytes).
 *   Results.  Per unit, in document order then text order: begin and end (batch byte positions), flag (1 for a repeat).  Per
 *   document: unit_off [n_docs + 1]; n_dup, dup_bytes, dup_chars over the flagged units; unit_bytes, unit_chars over all units;
 *   doc_chars over [a, e) (whatever the status); top_count = the largest count (0 without units); top_first = the
 *   document-relative index of the first unit with that count (-1 without units).  Gopher's duplicate-line fraction is n_dup /
 *   the document's units, its character fraction dup_chars / doc_chars.
 *   Deviation: the device keeps the units of a group of documents in one table keyed by k alone, so two units of different
 *   documents with equal k (different key_D: probability 2^-64 per pair) would be conflated; for a table of m units at most
 *   m^2 / 2^65 such pairs are expected -- as for jtk_batch_ngram_repeats.
 * Both calls work on the LAST batch encode on `b` under the conditions of jtk_batch_char_index: host or device input, any flags
 *   (JTK_ENCODE_COUNT_ONLY included: the text is read, not the ids) but JTK_ENCODE_FIM; not after jtk_batch_encode_pieces or
 *   jtk_batch_encode_device_max_tokens (JTK_ERR_INVALID_ARGUMENT); device-input text must still be valid and unchanged.
 * jtk_batch_line_units: finds and hashes the units on stream_or_null (the batch's stream when NULL), waits once to read
 *   *n_units, and keeps the list in the batch -- 48 bytes per unit, allocated at the counted size before anything is written to
 *   it, and n_bytes / 4 + 52 bytes per 4096 of text of scratch -- until the next encode or until a call with another (unit, flags &
 *   JTK_LINES_TRIM, seed, doc_index_base).  JTK_ERR_OUT_OF_MEMORY leaves no list.
 * jtk_batch_line_repeats: needs the list of a jtk_batch_line_units call with the same (unit, flags & JTK_LINES_TRIM, seed,
 *   doc_index_base) on the same encode: JTK_ERR_INVALID_ARGUMENT otherwise.  Every pointer of `out` is device memory, may be NULL
 *   and is then not written; int32 arrays 4-byte aligned, int64 arrays 8-byte aligned (JTK_ERR_INVALID_ARGUMENT otherwise), the
 *   flag bytes at any alignment.  A document of 2^31 units or more is JTK_ERR_INVALID_ARGUMENT.  A refused call writes nothing.
 *   The batch is walked in groups of whole documents under JTK_OPT_REPEAT_TABLE_BYTES and shares the table of
 *   jtk_batch_ngram_repeats (a pass of either waits for the one before it); results never depend on the grouping.  Waits once,
 *   for the documents' unit counts, from which the groups are planned; the passes are then queued and the call does not wait for
 *   them.  Chunk, pack, fetch, MinHash and n-gram results are untouched by both calls. */
#define JTK_LINES_LINE 0
#define JTK_LINES_PARAGRAPH 1
#define JTK_LINES_MARK_FIRST 1u
#define JTK_LINES_TRIM 2u
typedef struct jtk_lines_params {
    uint64_t seed;
    uint64_t doc_index_base;
    int32_t unit;           /* JTK_LINES_LINE or JTK_LINES_PARAGRAPH */
    uint32_t flags;         /* JTK_LINES_MARK_FIRST | JTK_LINES_TRIM */
} jtk_lines_params;         /* 24 bytes */
typedef struct jtk_lines_out {      /* device pointers, each may be NULL and is then not written */
    int64_t *unit_begin, *unit_end; /* [n_units] */
    uint8_t* unit_flags;            /* [n_units] */
    int64_t* unit_off;              /* [n_docs + 1] */
    int32_t* n_dup;                 /* [n_docs], as are the following */
    int64_t *dup_bytes, *dup_chars, *unit_bytes, *unit_chars, *doc_chars;
    int32_t* top_count;
    int64_t* top_first;
} jtk_lines_out;
int jtk_batch_line_units(jtk_batch* b, const jtk_lines_params* params, void* stream_or_null, int64_t* n_units);
int jtk_batch_line_repeats(jtk_batch* b, const jtk_lines_params* params, const jtk_lines_out* out, void* stream_or_null);

/* Device buffers already resident in HBM (what bench.py times).  `stream_or_null` = a hipStream_t
 * to order against, or NULL for the batch's own stream: the whole encode is ordered like one operation on that stream
 * (inside, the chunks of a large batch run on the batch's own streams, forked from and joined into it).  With
 * n_tokens == NULL the call does not wait for the result (a batch larger than one chunk waits for the work queued on the
 * stream BEFORE it, once, to read the chunk boundaries from d_doc_off); query later with jtk_batch_result().
 * d_utf8 must be 16-byte aligned and readable up to the next multiple of 16 past n_bytes; d_doc_off is checked on the
 * device: offsets that are out of range or decreasing make JTK_ERR_INVALID_ARGUMENT the batch's worst status. */
int jtk_batch_encode_device(jtk_batch* b, const uint8_t* d_utf8, const int64_t* d_doc_off, int64_t n_docs,
                            int64_t n_bytes, uint32_t flags, void* stream_or_null, int64_t* n_tokens);

/* ---- special tokens as ids (JTK_ENCODE_ALLOW_SPECIAL) -----------------------------------------------------------------
 * A batch has an allowed set of special ids; a new batch allows all of the encoding's specials.  n < 0: all, n == 0: none;
 * an id that is no special id of the encoding is JTK_ERR_INVALID_ARGUMENT (the set is then unchanged).  An id that several
 * literals map to allows all of them.  Waits for the batch's last encode if it may still be running.
 *
 * With the flag, each document is encoded as tiktoken's encode(doc, allowed_special=A, disallowed_special=D) does:
 *   Matching:    from the document's start, the next match is the leftmost position where some allowed literal occurs
 *                entirely inside the document, and of the literals matching there the longest; scanning resumes after it,
 *                so matches never overlap (jtokkit_amd/csrc/jtk_special_rules.h).  tiktoken breaks ties by the order of its
 *                regex alternation; no allowed literal of the four shipped encodings is a prefix of another, so the results
 *                agree there.  For custom sets, leftmost-longest is the rule.
 *   Segments:    the text before, between and after the matches is encoded as encodeOrdinary(segment) -- a split of its
 *                own per segment, not a slice of the whole document's split --, and each match gives its id.
 *   Disallowed:  without JTK_ENCODE_ORDINARY (encode()), a literal outside the allowed set that occurs anywhere in the
 *                document (text.contains, even overlapping an allowed match) gives it JTK_ERR_UNSUPPORTED_SPECIAL and no
 *                tokens; with JTK_ENCODE_ORDINARY such literals are ordinary text.
 *   Empty set:   the results are those of the call without the flag (it is that call).
 *   Flags:       JTK_ENCODE_COUNT_ONLY, JTK_ENCODE_VALIDATE_UTF8 (it judges the whole document: a document is well-formed
 *                when its segments and literals are, for literals that are well-formed UTF-8 themselves) and
 *                JTK_ENCODE_TO_HOST compose with it.  tok_off and status are per document of the call; fetch, device and host
 *                results, jtk_batch_chunk / _chunk_rows / _token_offsets read them as any other (a special token's byte span
 *                is its literal, as the decode table holds it); jtk_batch_truncate returns JTK_ERR_INVALID_ARGUMENT after it.
 *   Waits:       once for the number of literal candidates in the batch, plus the chunk plan's wait of a text larger than
 *                JTK_OPT_CHUNK_BYTES (JTK_OPT_HOST_CHUNK_BYTES for host input) as without the flag -- at most two before the
 *                work is queued; a batch without a match then runs exactly the call without the flag (unless it holds a
 *                literal outside the allowed set under encode(), or JTK_ENCODE_VALIDATE_UTF8 is set: offenders have no
 *                tokens, so the whole path runs).  Host input is
 *                copied down whole before the candidates are found (no overlap of the copy with the kernels), and with
 *                JTK_ENCODE_TO_HOST the result goes to the pinned buffers in one copy behind the last chunk (one more wait,
 *                for its size) instead of chunk by chunk.  JTK_OPT_REUSE_CHUNK_PLAN does not apply to these calls. */
int jtk_batch_set_allowed_special(jtk_batch* b, const int32_t* special_ids, int n);

/* ---- fill-in-the-middle training data (JTK_ENCODE_FIM) ----------------------------------------------------------------------
 * Bavarian et al., "Efficient Training of Language Models to Fill in the Middle": with probability fim_rate a document is cut
 * at two random positions of its text into prefix, middle and suffix, the three parts are encoded separately as
 * encodeOrdinary(part), and the document's tokens become
 *   PSM:  prefix_id enc(prefix) suffix_id enc(suffix) middle_id enc(middle)
 *   SPM:  prefix_id suffix_id enc(suffix) middle_id enc(prefix) enc(middle)       (with probability spm_rate among the cut ones)
 * The rule (jtokkit_amd/csrc/jtk_fim_rules.h), per document d of len bytes, g = doc_index_base + d:
 *   Draws:     mix = the splitmix64 finaliser; draw(g, k) = mix(mix(seed + 0x9E3779B97F4A7C15 * (g + 1)) + k) modulo 2^64.  They
 *              are counter-based: a document's outcome depends on (seed, g, its bytes) only, so a shard of a corpus, encoded
 *              with doc_index_base = the index of its first document, draws what the whole corpus would.
 *   Kind:      0 (untouched: exactly the call without the flag) when len == 0, or when (draw(g, 0) >> 32) >= fim_rate and
 *              fim_rate != 0xFFFFFFFF; else 2 (SPM) when (draw(g, 1) >> 32) < spm_rate or spm_rate == 0xFFFFFFFF; else 1 (PSM).
 *   Cuts:      p_k = the high 64 bits of draw(g, 2 + k) * (len + 1), k = 0, 1, each uniform over [0, len], then moved back to
 *              a character start: while 0 < p < len and the byte at p is 0x80..0xBF, at most 3 times, p -= 1.  a = the lower,
 *              b = the higher; prefix [0, a), middle [a, b), suffix [b, len), any of them may be empty.
 *   Status:    the lowest of the three parts' statuses (JTK_ENCODE_VALIDATE_UTF8 so judges the whole document: its parts are
 *              well-formed exactly when it is); a document with a negative status has no tokens.
 *   Flags:     JTK_ENCODE_ORDINARY is required (encode()'s special-token check would have to look across the cuts);
 *              JTK_ENCODE_VALIDATE_UTF8, JTK_ENCODE_COUNT_ONLY, JTK_ENCODE_TO_HOST and JTK_ENCODE_COMPACT_IDS compose with it as
 *              they do with JTK_ENCODE_ALLOW_SPECIAL (host input goes down whole, the host result in one copy behind the last
 *              chunk); JTK_ENCODE_ALLOW_SPECIAL with it, the flag without parameters set, and the flag at any other entry
 *              point are JTK_ERR_INVALID_ARGUMENT.  JTK_OPT_REUSE_CHUNK_PLAN does not apply.
 *   Afterwards: token positions are no longer positions in the text: jtk_batch_chunk / _chunk_prefer, jtk_batch_token_offsets,
 *              jtk_batch_token_spans, the jtk_batch_char_* calls and jtk_batch_truncate return JTK_ERR_INVALID_ARGUMENT;
 *              fetch, device and host results, jtk_batch_compact and jtk_batch_pack (and its labels without spans) work on
 *              the result as on any other.
 *   Waits:     none of its own: the chunk plan's wait of a text larger than JTK_OPT_CHUNK_BYTES as without the flag, and with
 *              JTK_ENCODE_TO_HOST one for the size of the copy.
 * jtk_batch_set_fim: the parameters of later JTK_ENCODE_FIM encodes on this batch (copied); NULL clears them.  Each of the three
 * ids must be a special id of the encoding (JTK_ERR_INVALID_ARGUMENT otherwise, the parameters are then unchanged).
 * jtk_batch_fim_result: after a JTK_ENCODE_FIM encode (JTK_ERR_INVALID_ARGUMENT otherwise), device pointers valid until the next
 * encode on this batch: kind [n_docs] (0 untouched, 1 PSM, 2 SPM), cut [n_docs][2] (a, b: byte positions relative to the
 * document; len, len for kind 0), part_tok [n_docs][3] (tokens of prefix, middle, suffix; 0 for a document without tokens).
 * The middle is the last part_tok[d][1] tokens of document d in both layouts.  _fetch copies them to host arrays (it waits
 * for the encode).  Any pointer may be NULL. */
typedef struct jtk_fim_params {
    uint64_t seed;
    int64_t doc_index_base;     /* the global index of the batch's document 0 */
    uint32_t fim_rate;          /* in units of 2^-32; 0xFFFFFFFF: always */
    uint32_t spm_rate;          /* in units of 2^-32; 0xFFFFFFFF: always */
    int32_t prefix_id, middle_id, suffix_id;
} jtk_fim_params;
int jtk_batch_set_fim(jtk_batch* b, const jtk_fim_params* params_or_null);
int jtk_batch_fim_result(jtk_batch* b, const uint8_t** d_kind, const int64_t** d_cut, const int64_t** d_part_tok);
int jtk_batch_fim_result_fetch(jtk_batch* b, uint8_t* kind, int64_t* cut, int64_t* part_tok);

/* The batch's own HIP stream (a hipStream_t), e.g. to order a caller's work after a non-synchronising encode. */
void* jtk_batch_stream(jtk_batch* b);

/* Synchronises and reports the totals of the last encode. */
int jtk_batch_result(jtk_batch* b, int64_t* n_tokens, int64_t* n_docs, int32_t* worst_status);

/* Copies the last result to host buffers: tokens[tokens_cap] (JTK_ERR_CAPACITY if too small),
 * tok_off[n_docs + 1], status[n_docs]; any of them may be NULL. */
int jtk_batch_fetch(jtk_batch* b, int32_t* tokens, int64_t tokens_cap, int64_t* tok_off, int32_t* status);

/* Device pointers of the last result (valid until the next encode on this batch).  After a host-input job of <= 128 KiB with
 * JTK_ENCODE_TO_HOST they are addresses of pinned host memory the device can reach (the kernels wrote the result there). */
int jtk_batch_device_result(jtk_batch* b, const int32_t** d_tokens, const int64_t** d_tok_off,
                            const int32_t** d_status);

/* Per-kernel device time of the last encode, measured with HIP events on the stream the kernels
 * ran on (enable first; costs a few event records per encode).  names[i] points to static strings. */
int jtk_batch_set_profiling(jtk_batch* b, int enabled);
int jtk_batch_kernel_times(jtk_batch* b, const char** names, float* ms, int cap, int* n);

/* ---- single-document entry points (what the per-call Encoding methods bind) ---------------------
 * Encoding.encode(String[, maxTokens]) / encodeOrdinary(..) (GptBytePairEncoding.java:38-69):
 * max_tokens < 0 means "no limit"; otherwise the result is clipped to max_tokens and backed off to
 * a code-point boundary exactly as :90-100 does, and *truncated gets EncodingResult.isTruncated().
 * utf8 == NULL mirrors text == null (empty result, :48-50).
 * Flags: JTK_ENCODE_ORDINARY; JTK_ENCODE_VALIDATE_UTF8 without a token limit (max_tokens < 0): a malformed document
 * returns JTK_ERR_BAD_UTF8 with *n_tokens = 0 and no tokens written, a well-formed one is unaffected; with a token limit
 * the flag is ignored (only the document's leading bytes are looked at).  JTK_ENCODE_COUNT_ONLY is ignored;
 * JTK_ENCODE_ALLOW_SPECIAL and JTK_ENCODE_COMPACT_IDS are JTK_ERR_INVALID_ARGUMENT. */
int jtk_encode(jtk_batch* b, const uint8_t* utf8, int64_t len, uint32_t flags, int64_t max_tokens,
               int32_t* tokens, int64_t tokens_cap, int64_t* n_tokens, int* truncated);

/* Encoding.decodeBytes(List<Integer>) (GptBytePairEncoding.java:137-151, 302-314): concatenates the
 * byte strings of `ids`; *len receives the byte count (out may be NULL to size). */
int jtk_decode(const jtk_encoding* enc, const int32_t* ids, int64_t n, uint8_t* out, int64_t cap, int64_t* len);

/* ---- maxTokens for a whole batch, on the device ------------------------------------------------------
 * Encoding.encode(String, int maxTokens) / encodeOrdinary(String, int) (GptBytePairEncoding.java:43-45, 66-69) for
 * every document of the LAST batch encode on `b`: document d keeps the first kept[d] of its tokens
 * ([tok_off[d], tok_off[d] + kept[d]) of the encode result) -- min(maxTokens, count) backed off to a code-point
 * boundary exactly as :90-100 does -- and truncated[d] = EncodingResult.isTruncated() (:97).
 * The input text of that encode must still be where it was (host-buffer encodes keep their own copy). */
int jtk_batch_truncate(jtk_batch* b, int64_t max_tokens);
int jtk_batch_fetch_truncated(jtk_batch* b, int64_t* kept, uint8_t* truncated);           /* [n_docs] each, may be NULL */
int jtk_batch_device_truncated(jtk_batch* b, const int64_t** d_kept, const uint8_t** d_truncated);

/* Encoding.encode(text, maxTokens) / encodeOrdinary(text, maxTokens) for every document WITHOUT encoding the documents whole
 * (the reference stops matching at maxTokens, GptBytePairEncoding.java:83-88): leading bytes of each document are encoded
 * (8 per wanted token + 64, 4x more for the documents that turn out to need it) and a result is taken once it is certain to be the
 * head of the full token list.  Host buffers.  tokens: [n_docs * max_tokens], document d's ids at tokens + d * max_tokens;
 * kept[d] ids are valid; truncated[d] (may be NULL) = EncodingResult.isTruncated(); status[d] (may be NULL) is JTK_OK or
 * JTK_ERR_UNSUPPORTED_SPECIAL.  flags: JTK_ENCODE_ORDINARY or 0.  Afterwards the batch's encode result is that of the last
 * group of leading bytes the call encoded (an internal job, of no use to the caller), or the earlier one if it encoded none. */
int jtk_batch_encode_max_tokens(jtk_batch* b, const uint8_t* utf8, const int64_t* doc_off, int64_t n_docs, uint32_t flags,
                                int64_t max_tokens, int32_t* tokens, int64_t* kept, uint8_t* truncated, int32_t* status);

/* Encoding.encode(String, maxTokens) / encodeOrdinary(String, maxTokens) (GptBytePairEncoding.java:43-45, 66-69, 79-100) for
 * every document of a device-resident batch, with the early exit of jtk_batch_encode_max_tokens, on the device.
 * d_tokens[n_docs * max_tokens]: row d holds document d's first kept[d] ids, then pad_id up to max_tokens.
 *   Results: tokens[:kept], kept, truncated and status equal what jtk_batch_encode_max_tokens returns on the same bytes
 *            (its conservative JTK_ERR_UNENCODABLE rule included).  Rows that get no tokens (special-token and error
 *            documents among them) are all pad_id.  status[d]: JTK_OK, JTK_ERR_UNSUPPORTED_SPECIAL, JTK_ERR_UNENCODABLE ...
 *   flags:   JTK_ENCODE_ORDINARY or 0 (anything else: JTK_ERR_INVALID_ARGUMENT).
 *   Input:   d_utf8 needs no alignment (the library encodes its own aligned copy of the documents' leading bytes); only the
 *            16-byte blocks that hold [0, n_bytes) are read.  d_doc_off[n_docs + 1] is checked on the device: offsets that are
 *            decreasing or outside [0, n_bytes] make the call return JTK_ERR_INVALID_ARGUMENT, and no row is written.
 *   Order:   the work is ordered on stream_or_null (a hipStream_t), or on the batch's stream when it is NULL, like
 *            jtk_batch_encode_device.  The call waits for the device once per round, to read a 16-byte word (open
 *            documents, gathered bytes), plus the chunk plan's wait when the leading bytes span more than one chunk
 *            (JTK_OPT_CHUNK_BYTES).  It returns when all rows are written.
 *   Batch:   afterwards the batch holds no encode result, whether the call succeeded or failed in any round: jtk_batch_fetch /
 *            jtk_batch_truncate fail until the next encode. */
int jtk_batch_encode_device_max_tokens(jtk_batch* b, const uint8_t* d_utf8, const int64_t* d_doc_off, int64_t n_docs,
                                       int64_t n_bytes, uint32_t flags, int64_t max_tokens, int32_t pad_id,
                                       int32_t* d_tokens, int64_t* d_kept, uint8_t* d_truncated, int32_t* d_status,
                                       void* stream_or_null);

/* ---- chunks of a token budget, on the device -------------------------------------------------------------------------
 * Every document of the LAST batch encode on `b` cut into consecutive chunks of at most chunk_tokens (N) of its tokens, each a
 * whole number of characters where the tokens allow it, with the byte span of each: what RAG, embedding and long-context data
 * pipelines do with a limit.  The rule (jtokkit_amd/csrc/jtk_chunk_rules.h): a chunk that starts at token s ends at the last
 * token boundary e in (s, s + N] that is also a character boundary -- the back-off of GptBytePairEncoding.java:90-100, except that
 * a cut inside a U+FFFD of the text is not taken --, or at s + N if there is none (then split = 1: the chunk starts or ends
 * inside a character); the next chunk starts at e, or with overlap > 0 at the first character boundary in
 * [max(e - overlap, s + 1), e].  The last chunk ends at the document's end.  Chunks are exact slices of encode(doc), NOT what
 * repeated encode(rest, N) calls on the remaining text would give; with overlap 0 they concatenate to encode(doc).  Chunk 0
 * equals encode(doc, N).getTokens() whenever that is non-empty and ends on a byte boundary.  Documents that are empty or have a
 * negative status get no chunks.
 *   Input:  the last encode (host- or device-input; not after a JTK_ENCODE_COUNT_ONLY encode, not after
 *           jtk_batch_encode_device_max_tokens: JTK_ERR_INVALID_ARGUMENT); 1 <= chunk_tokens < 2^31, 0 <= overlap < chunk_tokens.
 *   Order:  queued after that encode on stream_or_null (a hipStream_t), or on the batch's stream when it is NULL; the call
 *           waits once, to read *n_chunks (the records are then still being written on that stream).  Does not read the text.
 *   Spans:  byte_begin / byte_end are positions in the batch text: doc_off[d] + the decoded bytes of the document's tokens
 *           before the chunk's first / after its last token.  After jtk_batch_encode_pieces, bytes that no piece covers are
 *           not encoded: spans are then positions in the decoded stream of the document, counted from doc_off[d]. */
int jtk_batch_chunk(jtk_batch* b, int64_t chunk_tokens, int64_t overlap, void* stream_or_null, int64_t* n_chunks);
/* The last jtk_batch_chunk to host buffers (synchronises): chunk_off[n_docs + 1] (document d has chunks
 * [chunk_off[d], chunk_off[d + 1])), and per chunk [n_chunks]: its document, tok_begin (index into the batch's token array),
 * n_tok, byte_begin, byte_end, split.  Any may be NULL. */
int jtk_batch_chunk_fetch(jtk_batch* b, int64_t* chunk_off, int64_t* chunk_doc, int64_t* tok_begin, int32_t* n_tok,
                          int64_t* byte_begin, int64_t* byte_end, uint8_t* split);
/* Device pointers of the same arrays (valid until the next encode or chunk call on this batch). */
int jtk_batch_chunk_device_result(jtk_batch* b, const int64_t** d_chunk_off, const int64_t** d_chunk_doc,
                                  const int64_t** d_tok_begin, const int32_t** d_n_tok, const int64_t** d_byte_begin,
                                  const int64_t** d_byte_end, const uint8_t** d_split);
/* d_rows[n_chunks * chunk_tokens] (device, 4-byte aligned): row c holds chunk c's ids, then pad_id.  Ordered after the chunk
 * call on stream_or_null (or the batch's stream); does not wait. */
int jtk_batch_chunk_rows(jtk_batch* b, int32_t pad_id, int32_t* d_rows, void* stream_or_null);
/* d_byte_pos[n_tokens] (device): for every token of the last encode, its position in the batch text (doc_off[d] + the decoded
 * bytes of the document's tokens before it) -- a tokenizer's offset mapping.  Reuses the byte scan of a jtk_batch_chunk on the
 * same encode; without one it synchronises once for the token count.  Not after a count-only encode. */
int jtk_batch_token_offsets(jtk_batch* b, int64_t* d_byte_pos, void* stream_or_null);

/* ---- chunks that end at paragraph, line, sentence and word boundaries, on the device -----------------------------------
 * jtk_batch_chunk cuts at the last character boundary inside the budget; this call fills the budget and then backs off to the
 * best boundary in a window, as text splitters for RAG and embedding pipelines do.  The rule
 * (jtokkit_amd/csrc/jtk_chunk_prefer_rules.h): every cut between two tokens of a document has a level -- 0 SPLIT (inside a
 * character), 1 CHAR, 2 WORD (white space on either side), 3 SENTENCE (after . ! ? and white space, or after one of the CJK
 * stops U+3002 U+FF01 U+FF1F), 4 LINE (after \n, not before \n or \r), 5 PARAGRAPH (LINE after \n\n or \n\r\n) --, the highest
 * class that holds among those enabled in `prefer`; the document's two ends have level 6.  The bytes are those of the
 * decoded token stream (a special id counts as its literal); a cut's level looks back at most three bytes and never into the
 * document before.  A chunk that starts at token s ends at the document's end if that is within N = chunk_tokens tokens, else
 * at the last cut of the highest level in [s + min_tokens, s + N] (the back-off of jtk_batch_chunk if all are SPLIT); the next
 * chunk starts at the first cut of the highest level in [max(e - overlap, s + 1), e), or at e.  With prefer == 0 and
 * min_tokens == 1 the chunks are those of jtk_batch_chunk.  Chunks are exact slices of encode(doc), have at most N tokens,
 * and with overlap 0 concatenate to encode(doc).
 *   Input, order and spans: as jtk_batch_chunk.  1 <= min_tokens <= chunk_tokens and prefer within 15, else
 *           JTK_ERR_INVALID_ARGUMENT.  Does not read the text: it works after device-input encodes whose text is gone.
 *   Waits:  once to read *n_chunks, as jtk_batch_chunk; before that for the encode itself if the caller has not yet (the
 *           level plane is sized by its token count, as in jtk_batch_token_offsets).
 *   Result: replaces the batch's chunk result: jtk_batch_chunk_fetch, _device_result, _rows and jtk_batch_token_offsets read
 *           it as they read jtk_batch_chunk's; jtk_batch_chunk_levels adds the level of every chunk's end. */
enum { JTK_CUT_WORD = 1u, JTK_CUT_SENTENCE = 2u, JTK_CUT_LINE = 4u, JTK_CUT_PARAGRAPH = 8u };
enum { JTK_LEVEL_SPLIT = 0, JTK_LEVEL_CHAR, JTK_LEVEL_WORD, JTK_LEVEL_SENTENCE, JTK_LEVEL_LINE, JTK_LEVEL_PARAGRAPH, JTK_LEVEL_DOC_END };
int jtk_batch_chunk_prefer(jtk_batch* b, int64_t chunk_tokens, int64_t overlap, int64_t min_tokens, uint32_t prefer,
                           void* stream_or_null, int64_t* n_chunks);
/* end_level[n_chunks] of the last jtk_batch_chunk_prefer: to a host buffer (synchronises) and / or as a device pointer (valid
 * until the next encode or chunk call on this batch); either may be NULL.  JTK_ERR_INVALID_ARGUMENT when the batch's chunk
 * result comes from a plain jtk_batch_chunk. */
int jtk_batch_chunk_levels(jtk_batch* b, uint8_t* end_level_or_null /* host [n_chunks] */, const uint8_t** d_end_level_or_null);
/* d_level[n_tokens] (device): for every token of the last encode the level of the cut before it under `prefer` (within 15), 6
 * for the first token of a document.  Queued after the encode on stream_or_null (or the batch's stream); waits only for the
 * encode, if the caller has not yet (jtk_batch_result).  Leaves the batch's chunk result as it is.  Not after a count-only encode or jtk_batch_encode_device_max_tokens.  Entries of documents with a negative status carry no
 * meaning. */
int jtk_batch_token_cut_levels(jtk_batch* b, uint32_t prefer, uint8_t* d_level /* device [n_tokens] */, void* stream_or_null);

/* ---- character positions: UTF-16 and code-point offsets, on the device -------------------------------------------------
 * Every position above is a byte position in String.getBytes(UTF_8).  These calls convert between the byte positions of the
 * LAST batch encode's text and indices into the documents as a Java String (JTK_UNIT_UTF16: what substring takes) or a Python
 * str (JTK_UNIT_CODEPOINT: what tiktoken's decode_with_offsets and an offset_mapping hold).  The rule
 * (jtokkit_amd/csrc/jtk_charpos_rules.h) is per byte and defined for any bytes: a byte that is no continuation byte
 * ((x & 0xC0) != 0x80) counts 1, a byte >= 0xF0 one more in UTF-16 units (a surrogate pair), every byte 1 with JTK_UNIT_BYTE.
 * The sums equal new String(bytes, UTF_8) indices and Python str indices for WELL-FORMED documents only; for others they are
 * still the sums of these weights (no U+FFFD accounting) -- encode with JTK_ENCODE_VALIDATE_UTF8 to find such documents
 * (JTK_ERR_BAD_UTF8).
 *   Coordinates  byte positions are batch positions (those of byte_begin and jtk_batch_token_offsets); character positions
 *                are relative to their document [a, e) = [doc_off[d], doc_off[d + 1]).
 *   Rounding     a boundary is a, e, or a byte that is no continuation byte.  JTK_CHAR_FLOOR takes the nearest boundary at or
 *                before the position (the index of the character that holds the byte: tiktoken's convention for a token that
 *                starts inside a character), JTK_CHAR_CEIL the nearest at or after it (a partly covered character counts: the
 *                exclusive end); looked for within 3 bytes and inside [a, e], else the position itself.
 *   Forward      d_char_pos[i] = the units of [a, snap(d_byte_pos[i])) of document d_doc_or_null[i] -- without the array, of
 *                the last document with doc_off[d] <= the position (a document edge belongs to the document that starts there,
 *                n_bytes to the last document).  -1 for a position outside [a, e] or a bad document.
 *   Inverse      d_byte_pos[i] = the largest boundary q of document d_doc[i] with at most d_char_pos[i] units in [a, q): -1
 *                for a negative index or a bad document, e for an index at or past the document's length.  A UTF-16 index that
 *                points at a low surrogate gives the first byte of its 4-byte character.
 *   Index        the first call after an encode builds a rank / select index over the text (about 3.3 % of its size) for the
 *                unit; later calls with that unit reuse it, a call with another unit rebuilds it, a new encode of any kind
 *                drops it.  jtk_batch_char_index builds it ahead of time and, with d_doc_units_or_null [n_docs], writes every
 *                document's length (String.length(), len(str)).
 *   Tokens       jtk_batch_token_char_offsets: per token of the last encode, d_begin = FLOOR of its first byte and
 *                d_end_or_null = CEIL of its end, both relative to the token's document.  Reuses the byte scan of a
 *                jtk_batch_chunk / _token_offsets / _token_spans on the same encode; without one it waits once, for the token
 *                count.
 *   Order        queued after the last encode on stream_or_null (or the batch's stream); the calls do not wait (but for the
 *                token count above).  They READ THE TEXT: with device input (jtk_batch_encode_device) the caller's text and
 *                offsets must stay valid and unchanged until these calls have run, as for jtk_batch_truncate.
 *   Errors       JTK_ERR_INVALID_ARGUMENT without an encode result (jtk_batch_encode_device_max_tokens leaves none), for an
 *                unknown unit or rounding, a NULL array with n > 0, after jtk_batch_encode_pieces (its positions are positions
 *                in the decoded stream), and for jtk_batch_token_char_offsets after a count-only encode.  The other three
 *                work after a count-only encode: they read only the text.  n == 0 and n_docs == 0 launch nothing. */
enum { JTK_UNIT_BYTE = 0, JTK_UNIT_UTF16 = 1, JTK_UNIT_CODEPOINT = 2 };
enum { JTK_CHAR_FLOOR = 0, JTK_CHAR_CEIL = 1 };
int jtk_batch_char_index(jtk_batch* b, int unit, int64_t* d_doc_units_or_null /* [n_docs], device */, void* stream_or_null);
int jtk_batch_char_positions(jtk_batch* b, int unit, int round, const int64_t* d_doc_or_null, const int64_t* d_byte_pos,
                             int64_t n, int64_t* d_char_pos, void* stream_or_null);
int jtk_batch_byte_positions(jtk_batch* b, int unit, const int64_t* d_doc, const int64_t* d_char_pos, int64_t n,
                             int64_t* d_byte_pos, void* stream_or_null);
int jtk_batch_token_char_offsets(jtk_batch* b, int unit, int64_t* d_begin, int64_t* d_end_or_null, void* stream_or_null);

/* ---- packed training rows, on the device ---------------------------------------------------------------------------
 * The documents of the LAST batch encode on `b` packed into rows of seq_len (L) tokens, as a pretraining or fine-tuning
 * loader does, with the document boundaries inside every row for a varlen attention call.  The rule
 * (jtokkit_amd/csrc/jtk_pack_rules.h): a document with a negative status contributes nothing; otherwise its unit is its ids
 * followed by sep_id (sep_id >= 0), sep_id followed by its ids (JTK_PACK_SEP_FIRST), or its ids alone (sep_id == -1); a unit
 * of length 0 is dropped.
 *   concat (default)      the units one after another, cut every L cells: n_rows = ceil(|S| / L), the last row padded with
 *                         pad_id -- or floor(|S| / L) with JTK_PACK_DROP_LAST, the partial row omitted.
 *   JTK_PACK_WHOLE_DOCS   each unit cut into items of L tokens (the last holds the rest), placed in order by next-fit: an item
 *                         goes into the current row if it fits in the cells left, else it starts a new row; every row padded to
 *                         L.  No document straddles two rows unless it is longer than a row.  Not with JTK_PACK_DROP_LAST.
 *   Segments              maximal runs of one unit's cells, or of pad cells, inside one row, in row-major order:
 *                         cu_seqlens[n_segments + 1] (int32; cu_seqlens[k + 1] - cu_seqlens[k] = the length of segment k, the
 *                         last entry n_rows * L), seg_doc[n_segments] (its document, -1 for pad), max_seqlen (0 without rows);
 *                         positions[r][c] = the offset of cell c in its segment (0 at every document boundary and row start).
 *   Input:   as jtk_batch_chunk (not after a count-only encode or jtk_batch_encode_device_max_tokens); seq_len >= 1;
 *            sep_id -1 or a rank or special id of the encoding; n_rows * seq_len < 2^31 (cu_seqlens is int32: split the batch
 *            otherwise).  Any violation: JTK_ERR_INVALID_ARGUMENT.
 *   Order:   the plan is queued after that encode on stream_or_null (or the batch's stream) and waits once, for the counts; a
 *            new encode drops it; pack and chunk results do not replace each other. */
enum {
    JTK_PACK_WHOLE_DOCS = 1u,     /* next-fit of whole documents (fine-tuning) instead of one concatenated stream */
    JTK_PACK_SEP_FIRST = 2u,      /* the separator before each document (BOS style) instead of after it (EOS style) */
    JTK_PACK_DROP_LAST = 4u       /* concat: omit a partial last row instead of padding it */
};
int jtk_batch_pack(jtk_batch* b, int64_t seq_len, int32_t sep_id, uint32_t flags, void* stream_or_null,
                   int64_t* n_rows, int64_t* n_segments, int32_t* max_seqlen);
/* The packed rows of the last jtk_batch_pack to device memory: d_rows[n_rows * seq_len] int32 (ids, then pad_id),
 * d_positions[n_rows * seq_len] int32, d_cu_seqlens[n_segments + 1] int32, d_seg_doc[n_segments] int64; all but d_rows may
 * be NULL.  Ordered after the plan on stream_or_null (or the batch's stream); does not wait. */
int jtk_batch_pack_write(jtk_batch* b, int32_t pad_id, int32_t* d_rows, int32_t* d_positions, int32_t* d_cu_seqlens,
                         int64_t* d_seg_doc, void* stream_or_null);
/* The same to host buffers (synchronises); any may be NULL. */
int jtk_batch_pack_fetch(jtk_batch* b, int32_t pad_id, int32_t* rows, int32_t* positions, int32_t* cu_seqlens, int64_t* seg_doc);

/* ---- labels of the packed rows from byte spans of the text, on the device --------------------------------------------
 * Supervised fine-tuning trains on parts of each document only -- the assistant turns of a chat, the completion after a
 * prompt -- and wants a labels tensor beside the rows, ignore_index everywhere else (the -100 labels a collator builds on the
 * host from a tokenizer's offset mapping).  Two passes do it on the device; the rule is jtokkit_amd/csrc/jtk_label_rules.h.
 *   Spans     [span_begin[i], span_end[i]), i < n_spans: byte positions in the batch text (the coordinates of byte_begin /
 *             byte_end of jtk_batch_chunk), sorted and disjoint: begin[i] <= end[i] <= begin[i + 1].  A span may cross
 *             document boundaries: membership goes by byte position alone.  An empty span holds no token.
 *   Tokens    token t of the last encode occupies [p_t, q_t): p_t as jtk_batch_token_offsets defines it (doc_off[d] + the
 *             decoded bytes of the document's tokens before it; a special token taken as an id counts its literal),
 *             q_t = p_t + the token's decoded length.
 *   tok_span  tok_span[t] = the lowest i for which the rule holds, or -1 (all -1 with n_spans == 0):
 *               JTK_SPAN_WHOLE   begin[i] <= p_t && q_t <= end[i]   (no byte outside the span is ever trained on)
 *               JTK_SPAN_START   begin[i] <= p_t && p_t < end[i]    (the usual offset-mapping rule)
 *               JTK_SPAN_ANY     p_t < end[i] && q_t > begin[i]
 *             Spans that are not sorted and disjoint give unspecified values of tok_span (and no access out of bounds).
 *   Labels    the unshifted label of a cell of the packed rows is its id when it holds token t of a document and
 *             tok_span[t] >= 0 (a NULL tok_span: every token is trainable); its id when it is an EOS-style separator
 *             (sep_id >= 0 without JTK_PACK_SEP_FIRST), JTK_LABEL_SEP is set and the unit's last token is trainable -- this
 *             teaches the model to stop; for a unit without tokens JTK_LABEL_SEP labels the separator only when tok_span is
 *             NULL --; ignore_index otherwise: BOS-style separators and pad cells always.  With JTK_LABEL_SHIFT cell (r, c)
 *             gets the unshifted label of cell (r, c + 1) when both lie in the same segment (the same row and the same unit,
 *             as cu_seqlens delimits them), else ignore_index: next-token targets never cross a document boundary, a row
 *             end, or into pad.  Without it labels[r][c] goes with rows[r][c] (models that shift inside their loss). */
enum { JTK_SPAN_WHOLE = 0, JTK_SPAN_START = 1, JTK_SPAN_ANY = 2 };
enum {
    JTK_LABEL_SHIFT = 1u,         /* labels[r][c] = the label of the next cell of the segment (next-token targets) */
    JTK_LABEL_SEP = 2u            /* an EOS-style separator after a trainable last token is a label too */
};
/* d_tok_span[n_tokens] (device, int32) for the tokens of the LAST batch encode on `b` (host- or device-input,
 * JTK_ENCODE_ALLOW_SPECIAL included) from n_spans spans in device memory.
 *   Input:  not after a count-only encode, jtk_batch_encode_pieces (its positions are positions in the decoded stream) or
 *           jtk_batch_encode_device_max_tokens; rule one of JTK_SPAN_*; 0 <= n_spans < 2^31, the arrays non-NULL unless
 *           n_spans == 0.  Any violation: JTK_ERR_INVALID_ARGUMENT.
 *   Order:  queued after that encode on stream_or_null (or the batch's stream), as jtk_batch_token_offsets is.  Reuses the
 *           byte scan of a jtk_batch_chunk or jtk_batch_token_offsets on the same encode; without one it waits once, for the
 *           token count.  No [n_tokens] array of positions is written. */
int jtk_batch_token_spans(jtk_batch* b, const int64_t* d_span_begin, const int64_t* d_span_end, int64_t n_spans,
                          int rule, int32_t* d_tok_span, void* stream_or_null);
/* d_labels[n_rows * seq_len] (device, int32) for the rows of the last jtk_batch_pack, from d_tok_span_or_null (the result of
 * jtk_batch_token_spans on the same encode, or NULL: every token is trainable).  flags: JTK_LABEL_SHIFT, JTK_LABEL_SEP
 * (other bits: JTK_ERR_INVALID_ARGUMENT).  Ordered after the plan on stream_or_null (or the batch's stream); does not wait. */
int jtk_batch_pack_labels(jtk_batch* b, const int32_t* d_tok_span_or_null, int32_t ignore_index, uint32_t flags,
                          int32_t* d_labels, void* stream_or_null);
/* The same to a host buffer labels[n_rows * seq_len] (synchronises); d_tok_span_or_null stays a device pointer. */
int jtk_batch_pack_labels_fetch(jtk_batch* b, const int32_t* d_tok_span_or_null, int32_t ignore_index, uint32_t flags,
                                int32_t* labels);

/* ---- batch decode on the device ---------------------------------------------------------------------
 * Replaces a loop of Encoding.decodeBytes(List<Integer>) (GptBytePairEncoding.java:137-151, 302-314; special-token
 * ids decode to their literals, :308-311) over n_seqs token lists: all ids back to back in `ids`, list q occupying
 * [seq_off[q], seq_off[q+1]).  Result: the byte strings back to back, list q occupying [byte_off[q], byte_off[q+1]);
 * status[q] = JTK_OK or JTK_ERR_UNKNOWN_TOKEN (that list's bytes then omit the unknown ids).  Both calls synchronise
 * and leave the result on the device; *n_bytes receives the total byte count.  jtk_batch_decode checks seq_off (it starts at
 * 0 and never decreases; JTK_ERR_INVALID_ARGUMENT otherwise); jtk_batch_decode_device does not validate d_seq_off, which must
 * hold the same and end at n_ids. */
int jtk_batch_decode(jtk_batch* b, const int32_t* ids, const int64_t* seq_off, int64_t n_seqs, int64_t* n_bytes);
int jtk_batch_decode_device(jtk_batch* b, const int32_t* d_ids, const int64_t* d_seq_off, int64_t n_seqs, int64_t n_ids,
                            void* stream_or_null, int64_t* n_bytes);
/* Copies the last decode to host buffers: out[out_cap] (JTK_ERR_CAPACITY if too small), byte_off[n_seqs + 1],
 * status[n_seqs]; any may be NULL. */
int jtk_batch_decode_fetch(jtk_batch* b, uint8_t* out, int64_t out_cap, int64_t* byte_off, int32_t* status);
/* Device pointers of the last decode (valid until the next decode on this batch). */
int jtk_batch_decode_device_result(jtk_batch* b, const uint8_t** d_out, const int64_t** d_byte_off, const int32_t** d_status);

/* ---- decode of an id matrix on the device --------------------------------------------------------------
 * Replaces a loop of Encoding.decodeBytes(List<Integer>) (GptBytePairEncoding.java:137-151, 302-314) over the rows of a matrix
 * of token ids, as a model's generate() or this library's padded rows (jtk_batch_encode_device_max_tokens, jtk_batch_chunk_rows)
 * hand them out: n_rows x width ids of id_bytes (4 or 8) bytes each, signed, row r starting at element r * row_stride
 * (row_stride >= width); the pointer is aligned to id_bytes, nothing more.  For row r (the rule is jtk_decode_rows_rules.h):
 *   window  [b, e) = begin[r] / end[r] clamped into [0, width]; 0 and width where the array is NULL; empty when e <= b.
 *   stop    s = the first column in [b, e) that holds one of the n_stop (<= JTK_DECODE_MAX_STOP_IDS) stop ids.  The row ends
 *           at e' = s, or at s + 1 with JTK_DECODE_KEEP_STOP; without such a column e' = e.  Stop ids left of b are not seen.
 *           The stop test comes before the pad test: a pad that is a stop id ends the row.
 *   cells   cell c contributes the byte string of its id when b <= c < e' and not (JTK_DECODE_SKIP_PAD and id == pad_id).
 *           A contributing cell whose id has no entry (negative, at or above the table, a hole, any 64-bit value outside
 *           int32: 2^32 + id is not id) contributes nothing and gives its row, and no other, JTK_ERR_UNKNOWN_TOKEN (:313).
 *           A skipped pad, a cell outside [b, e') and a stop id that is not kept never do.
 *   result  as a flat decode's, read with jtk_batch_decode_fetch / jtk_batch_decode_device_result with n_seqs = n_rows: the
 *           rows' bytes back to back, byte_off[n_rows + 1], status[n_rows].  cell_byte[n_rows * width] (optional, dense):
 *           the output position of the first byte of cell (r, c); for a cell without bytes, where the next byte of the matrix
 *           goes -- so cell_byte never decreases, and cell_byte[r * width] == byte_off[r] when b == 0.
 * Without stop ids, begin, end and JTK_DECODE_SKIP_PAD a row decodes exactly as jtk_batch_decode_device decodes it as a list.
 * Both calls synchronise as jtk_batch_decode_device does (once for the size of the output, once at the end) and leave the
 * result on the device; *n_bytes receives the total.  n_rows == 0 and width == 0 are valid (empty rows).  stop_ids is a host
 * array in both.  JTK_ERR_INVALID_ARGUMENT, before any device work: id_bytes not 4 or 8, row_stride < width, a negative size,
 * n_stop outside 0..JTK_DECODE_MAX_STOP_IDS, n_stop > 0 with stop_ids NULL, unknown flag bits, rows NULL with cells.
 * jtk_batch_decode_rows takes the matrix, begin, end and cell_byte_or_null in host memory. */
enum { JTK_DECODE_MAX_STOP_IDS = 8 };
enum {
    JTK_DECODE_SKIP_PAD = 1u,     /* cells that hold pad_id contribute nothing (and are never unknown) */
    JTK_DECODE_KEEP_STOP = 2u     /* the first stop id of a row is decoded too */
};
int jtk_batch_decode_rows_device(jtk_batch* b, const void* d_rows, int id_bytes, int64_t n_rows, int64_t width, int64_t row_stride,
                                 const int64_t* d_begin_or_null, const int64_t* d_end_or_null, int64_t pad_id,
                                 const int64_t* stop_ids, int n_stop, uint32_t flags, int64_t* d_cell_byte_or_null,
                                 void* stream_or_null, int64_t* n_bytes);
int jtk_batch_decode_rows(jtk_batch* b, const void* rows, int id_bytes, int64_t n_rows, int64_t width, int64_t row_stride,
                          const int64_t* begin_or_null, const int64_t* end_or_null, int64_t pad_id, const int64_t* stop_ids,
                          int n_stop, uint32_t flags, int64_t* cell_byte_or_null, int64_t* n_bytes);

/* ---- stop strings over the last decode, on the device -------------------------------------------------
 * Replaces a loop of bytes.find per row and per string over decoded text copied to the host, as a server does for OpenAI's
 * `stop` or vLLM / TGI `stop_sequences`.  A stop string is a property of the decoded text, not of the ids: the search is a
 * post-pass over the LAST decode of the batch, flat or rows, from host or device input (bytes `out`, byte_off[n_seqs + 1]),
 * and changes nothing of it.  n_strings strings back to back in `strings`, string i occupying [str_off[i], str_off[i + 1]),
 * both in host memory, in the caller's order of preference.  For sequence q (the rule is jtk_stop_rules.h):
 *   range   [S, E): S = byte_off[q] + d_from[q] clamped into [0, the sequence's length] (d_from_or_null NULL: 0),
 *           E = byte_off[q + 1].  String i of length L matches at p when S <= p, p + L <= E and the bytes are equal: a match
 *           never reaches into the next sequence, and one that starts before S does not count.
 *   match   the match with the smallest p, among those the smallest i (duplicate strings are allowed): stop_pos[q] = p, a
 *           position in `out` -- the cut text is out[byte_off[q], stop_pos[q]) --, stop_which[q] = i, hold[q] = 0.
 *   none    stop_pos[q] = E, stop_which[q] = -1, hold[q] = E - p* for the smallest p* in [max(S, E - (maxlen - 1)), E) at
 *           which out[p*, E) is a proper prefix of some string, 0 without one: the trailing bytes a streaming server must not
 *           emit yet (always below maxlen, the longest string's length).
 *   column  with d_cell_byte_or_null, the dense cell_byte [n_rows, width] of the rows decode, and a match: stop_col[q] = the
 *           largest column c with cell_byte[q * width + c] <= stop_pos[q], the cell that holds the byte at stop_pos (the
 *           row's kept cells end before it).  -1 without a match or without cell_byte.
 * Positions are bytes; UTF-16 positions of stops are not computed.  jtk_batch_decode_find_stops is ordered after the decode
 * on stream_or_null (or the batch's stream) and does not wait.  Results live in buffers the batch owns, valid until the next
 * jtk_batch_decode_find_stops; a new decode drops them.  n_strings == 0 is valid (no sequence matches, all holds 0), and so
 * are n_seqs == 0 and an empty `out` (nothing is launched).  JTK_ERR_INVALID_ARGUMENT, before any device work: no decode result
 * on the batch, n_strings outside 0..JTK_STOP_MAX_STRINGS, a string that is empty or longer than JTK_STOP_MAX_BYTES, str_off
 * not increasing from 0, NULL arrays with n_strings > 0, and d_cell_byte_or_null with width < 1 or after a decode that is not
 * a rows decode of exactly this width (a flat decode has no cells: cell_byte is refused after it, whatever the width).
 * _fetch copies to host arrays of n_seqs entries (any may be NULL) and synchronises; _device_result hands out the pointers. */
enum { JTK_STOP_MAX_STRINGS = 16, JTK_STOP_MAX_BYTES = 64 };
int jtk_batch_decode_find_stops(jtk_batch* b, const uint8_t* strings, const uint32_t* str_off, int n_strings,
                                const int64_t* d_from_or_null, const int64_t* d_cell_byte_or_null, int64_t width,
                                void* stream_or_null);
int jtk_batch_decode_stops_fetch(jtk_batch* b, int64_t* stop_pos, int32_t* stop_which, int32_t* hold, int64_t* stop_col);
int jtk_batch_decode_stops_device_result(jtk_batch* b, const int64_t** d_stop_pos, const int32_t** d_stop_which,
                                         const int32_t** d_hold, const int64_t** d_stop_col);

/* ---- UTF-16 in and out, on the device ---------------------------------------------------------------------------------
 * A Java String is UTF-16: these entry points take char[] and hand back char[], so that no host codec stands in front of or
 * behind the device passes.  Units are uint16 in the byte order of host and device (little-endian); no BOM handling: a U+FEFF
 * is a character.  Both rules are jtokkit_amd/csrc/jtk_utf16_rules.h.
 *   In (the rule of String.getBytes(UTF_8))   document d is units [unit_off[d], unit_off[d + 1]).  A unit below 0x80 gives 1
 *       byte, below 0x800 2 bytes, any other non-surrogate 3; a high surrogate whose next unit is in the same document and is a
 *       low surrogate gives the 4 bytes of the pair's code point and that low surrogate none; every other surrogate gives the
 *       single byte '?' (a lone high, a lone low, a high that ends its document even if the next document starts with a low,
 *       the first high of high high low).  Units outside [unit_off[0], unit_off[n_docs]) belong to no document.  doc_off[d]
 *       (int64 [n_docs + 1]) = the bytes of the units before unit_off[d].  For the transcoded text the JTK_UNIT_UTF16 length
 *       of every document (jtk_batch_char_index) is its original unit count, so every UTF-16 position the library hands out
 *       after jtk_batch_encode_utf16* is an index into the caller's char[].
 *   jtk_batch_transcode_utf16_device   runs it into buffers the batch owns: UTF-8 text, 16-byte aligned and readable to the next
 *       multiple of 16 (what jtk_batch_encode_device demands of its input), and doc_off.  d_units must be 2-byte aligned
 *       (JTK_ERR_INVALID_ARGUMENT otherwise); a 16-byte aligned d_units takes the fast path, which reads whole 16-byte granules
 *       up to the one that holds the last unit; any other alignment reads the n_units units alone and gives the same result.
 *       d_unit_off is checked on the device: it starts at or above 0, never decreases and ends at or below n_units
 *       (JTK_ERR_INVALID_ARGUMENT otherwise, nothing written).  The call waits once, for the byte count and that check; the
 *       write pass is queued on stream_or_null (or the batch's stream).
 *   jtk_batch_utf8_device_result   device pointers of the last transcode (of this call or inside jtk_batch_encode_utf16*), valid
 *       until the next transcode of the same kind on the batch.
 *   jtk_batch_encode_utf16_device   the transcode, then jtk_batch_encode_device on the owned text on the same stream.  That
 *       text is "the last encode's text" for every post-pass (chunk, pack, labels, character positions, token offsets) and
 *       stays alive until the next jtk_batch_encode_utf16*.  Flags JTK_ENCODE_ORDINARY, _VALIDATE_UTF8, _COUNT_ONLY and
 *       _ALLOW_SPECIAL are accepted; JTK_ENCODE_TO_HOST and JTK_ENCODE_COMPACT_IDS give JTK_ERR_INVALID_ARGUMENT (the result
 *       stays on the device: jtk_batch_fetch, jtk_batch_compact).
 *   jtk_batch_encode_utf16   the same for host buffers; n_units = unit_off[n_docs].  The offsets are validated on the host
 *       before anything is launched; then ONE upload and the device call: it is not chunk-pipelined as jtk_batch_encode is.
 *   Out (the rule of new String(bytes, UTF_8))   jtk_batch_decode_utf16 is a post-pass over the LAST decode of the batch, flat
 *       or rows: sequence q, bytes [byte_off[q], byte_off[q + 1]), becomes units [unit_off[q], unit_off[q + 1]).  Well-formed
 *       characters (Unicode Table 3-7) give their unit, or a surrogate pair for a 4-byte character; every maximal ill-formed
 *       subpart gives one U+FFFD: a lead with the continuation bytes that its row of the table accepts, up to the first byte it
 *       rejects or the end of the sequence; any other byte on its own (a stray continuation byte, C0, C1, F5..FF).  A character
 *       cut by a sequence edge gives U+FFFD on both sides.  This is CPython's bytes.decode("utf-8", "replace"), the codec that
 *       stands for new String(bytes, UTF_8) here (no JVM is at hand).  status is the decode's: a sequence with an unknown id
 *       keeps JTK_ERR_UNKNOWN_TOKEN and transcodes what was decoded.  The call waits as a decode does (once for the size, once
 *       at the end) and leaves units (uint16) and unit_off (int64 [n_seqs + 1]) in buffers the batch owns, valid until the next
 *       jtk_batch_decode_utf16; a new decode drops them.  _fetch and _device_result mirror jtk_batch_decode_fetch and
 *       jtk_batch_decode_device_result. */
int jtk_batch_transcode_utf16_device(jtk_batch* b, const uint16_t* d_units, const int64_t* d_unit_off, int64_t n_docs, int64_t n_units,
                                     void* stream_or_null, int64_t* n_bytes);
int jtk_batch_utf8_device_result(jtk_batch* b, const uint8_t** d_utf8, const int64_t** d_doc_off, int64_t* n_bytes);
int jtk_batch_encode_utf16_device(jtk_batch* b, const uint16_t* d_units, const int64_t* d_unit_off, int64_t n_docs, int64_t n_units,
                                  uint32_t flags, void* stream_or_null, int64_t* n_tokens);
int jtk_batch_encode_utf16(jtk_batch* b, const uint16_t* units, const int64_t* unit_off, int64_t n_docs, uint32_t flags,
                           int64_t* n_tokens);
int jtk_batch_decode_utf16(jtk_batch* b, void* stream_or_null, int64_t* n_units);
int jtk_batch_decode_utf16_fetch(jtk_batch* b, uint16_t* units, int64_t units_cap, int64_t* unit_off, int32_t* status);
int jtk_batch_decode_utf16_device_result(jtk_batch* b, const uint16_t** d_units, const int64_t** d_unit_off, const int32_t** d_status);

/* ---- per-call service: many caller threads, one device batch at a time -------------------------------------------
 * The reference is called per document from many threads (api/Encoding.java; its benchmark is one task per document on a
 * pool of 1..64 threads, benchmark/.../AbstractMultiThreadedBenchmark.java:35-45).  A jtk_service coalesces such callers:
 * whatever is queued when a worker becomes free is encoded as ONE device batch (no timer; while a batch is on the device
 * the next one piles up), and every caller gets its own tokens back.  Thread-safe.  n_workers (default 2) worker threads,
 * each with its own jtk_batch, so that the gathering of one batch overlaps the device time of another.
 *   jtk_service_encode   blocking: Encoding.encode / encodeOrdinary / countTokens (flags as for jtk_batch_encode;
 *                        max_tokens < 0 = no limit) -- same results and status codes as jtk_encode
 *   jtk_service_submit / jtk_service_wait   the same in two halves, so that one thread can keep many documents in flight;
 *                        utf8 and tokens must stay valid until the wait returns; every ticket must be waited for once */
typedef struct jtk_service jtk_service;
typedef struct jtk_ticket jtk_ticket;
int jtk_service_create(const jtk_encoding* enc, int n_workers, jtk_service** out);
void jtk_service_destroy(jtk_service* s);
int jtk_service_encode(jtk_service* s, const uint8_t* utf8, int64_t len, uint32_t flags, int64_t max_tokens,
                       int32_t* tokens, int64_t tokens_cap, int64_t* n_tokens, int* truncated);
int jtk_service_submit(jtk_service* s, const uint8_t* utf8, int64_t len, uint32_t flags, int64_t max_tokens,
                       int32_t* tokens, int64_t tokens_cap, jtk_ticket** ticket);
int jtk_service_wait(jtk_service* s, jtk_ticket* ticket, int64_t* n_tokens, int* truncated);
int jtk_service_done(const jtk_ticket* ticket);     /* 1: the result is in (jtk_service_wait returns at once), 0: not yet -- a poll for callers that must not block */
int jtk_service_stats(jtk_service* s, int64_t* n_batches, int64_t* n_docs);     /* device batches run, documents encoded */
/* What one device batch takes from the queue at most (defaults: 65536 documents, 64 MiB of text; a single larger document still
 * goes alone); the rest stays queued for the next batch.  Bounds the batch's pinned staging.  Values < 1 leave a limit as it is. */
int jtk_service_set_limits(jtk_service* s, int64_t max_docs, int64_t max_bytes);

/* ---- multi-GPU: document shards and the offset stitch ------------------------------------------------------------
 * Documents are independent (every Encoding.encode call is a pure function of one string, GptBytePairEncoding.java:71-103),
 * so a batch shards as contiguous document ranges balanced by bytes, one per GPU / process, each process with its own
 * jtk_encoding (the rank tables are a few MB) and jtk_batch.  The one exchange step is an RCCL all-gather of the per-shard
 * token totals (1 x int64 per rank, over xGMI); the exclusive prefix is the shard's first global token.  RCCL is bound at
 * run time (librccl.so; env JTK_RCCL_LIB), only when a communicator is created. */
typedef struct jtk_comm jtk_comm;

/* bounds[world + 1]: rank r encodes documents [bounds[r], bounds[r + 1]) (host arrays; doc_off has n_docs + 1 entries). */
int jtk_shard_plan(const int64_t* doc_off, int64_t n_docs, int world, int64_t* bounds);
/* ncclGetUniqueId: call on one rank, hand the 128 bytes to every rank by any side channel, then every rank creates its
 * communicator (ncclCommInitRank; collective over the ranks). */
int jtk_comm_unique_id(uint8_t* id128);
int jtk_comm_create(const uint8_t* id128, int world, int rank, int device, jtk_comm** out);
void jtk_comm_destroy(jtk_comm* c);
int jtk_comm_world(const jtk_comm* c);
int jtk_comm_rank(const jtk_comm* c);
/* The stitch, queued on `stream` (e.g. jtk_batch_stream() right after a non-synchronising jtk_batch_encode_device; nothing
 * waits for the host): all-gather of d_tok_off[n_docs] (this shard's token total), base = sum of the lower ranks' totals,
 * d_global_off[d] = d_tok_off[d] + base for d = 0..n_docs (d_global_off may be NULL: totals and base only).
 * *d_totals (world entries) and *d_base (1 entry) are the communicator's device buffers. */
int jtk_comm_stitch(jtk_comm* c, const int64_t* d_tok_off, int64_t n_docs, int64_t* d_global_off, void* stream,
                    const int64_t** d_totals, const int64_t** d_base);
/* Synchronises `stream` and copies the last stitch's totals[world] and base to the host. */
int jtk_comm_fetch(jtk_comm* c, void* stream, int64_t* totals, int64_t* base);

#define JTK_MAX_PIECE_BYTES (1 << 20)

#ifdef __cplusplus
}
#endif
#endif /* JTOKKIT_AMD_H */
