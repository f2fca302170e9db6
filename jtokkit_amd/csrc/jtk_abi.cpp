// jtk_abi.cpp -- the C ABI of include/jtokkit_amd.h: encoding objects, batch scratch, kernel
// orchestration.  Host C++ only; all compute is in jtk_kernels.hip.  There is no CPU fallback:
// without a HIP device every encode entry point fails with JTK_ERR_NO_DEVICE.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <vector>
#include <thread>
#include <chrono>

#include "../../include/jtokkit_amd.h"
#include "jtk_chunk_rules.h"
#include "jtk_chunk_prefer_rules.h"
#include "jtk_compact_rules.h"
#include "jtk_decode_rows_rules.h"
#include "jtk_kernels.h"
#include "jtk_lines_rules.h"
#include "jtk_maxtok_rules.h"
#include "jtk_ngram_rules.h"
#include "jtk_owned.h"
#include "jtk_repeat_rules.h"
#include "jtk_tables.h"

namespace {

thread_local std::string g_err;

int fail(int code, const std::string& msg) { g_err = msg; return code; }

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return fail(e_ == hipErrorOutOfMemory ? JTK_ERR_OUT_OF_MEMORY : JTK_ERR_HIP,           \
                        std::string(#expr) + ": " + hipGetErrorString(e_));                        \
    } while (0)

constexpr int N_STAGES = 8;
const char* const STAGE_NAMES[N_STAGES] = {"mark_docs", "validate_utf8", "pretok_split", "piece_resolve", "bpe_merge",
                                           "tile_scan", "pack", "doc_offsets"};

size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

}  // namespace

int jtk_fail_msg(int code, const std::string& msg) { return fail(code, msg); }      // for jtk_comm.cpp

struct jtk_encoding {
    JtkHostTables host;
    int device = 0;
    DevBuf uc1, uc2, uclds, splittab, brank, pairs, tok8, tok16, bprank, bpbits, bpcum, bpranks, pairin, dec_off, dec_blob, longtok, longblob, specials;
    DevBuf bnd;                      // jtk_batch_chunk: one bit per id of the decode table, set when its byte string does not start
                                     // with a UTF-8 continuation byte (lengths come from dec_off)
    uint32_t n_ids_table = 0;        // ids 0 .. n_ids_table-1 have an entry in the decode table (incl. special tokens)
    int hb = 0;                      // compact ids: high bits per token above the 16-bit plane (jtk_compact_rules.h)
    JtkDeviceTables dt;
    std::vector<uint32_t> tok_len;   // byte length per id (0 = absent), for the maxTokens back-off
};

int64_t jtk_max_tokens_backoff(const jtk_encoding* enc, const uint8_t* utf8, int64_t len, const int32_t* head, int64_t nt,
                               int64_t max_tokens, int* truncated);

// One chunk in flight: a stream and the scratch of the kernels (sized for the largest chunk it has seen).
struct __attribute__((visibility("hidden"))) ChunkSet {      // (internal: no weak symbol of this name leaves the library)
    Stream stream;
    Event ev_scan;                   // this set's tile_scan has run (the next chunk's scan waits for it: token order)
    Event ev_done;                   // this set's last kernel has run
    DevBuf zeroed;                   // docmask | list counters | queue counters
    DevBuf piecemask, gapmask, plist, htok, docpre, tile_np, tile_off, queues, q_meta, mid_list, long_list, giant_list;
    JtkWork work{};
    bool used = false;               // by the current job
};

constexpr int MAX_SETS = 4;
constexpr int64_t SMALL_JOB_BYTES = 1 << 20;
constexpr int64_t TINY_JOB_BYTES = 128 << 10;     // host jobs this small are staged so that offsets and text go down in one copy

struct jtk_batch {
    const jtk_encoding* enc = nullptr;
    Stream stream;                       // the batch's own main stream
    hipStream_t last_stream = nullptr;   // main stream of the last job (the caller's, or `stream`)
    Stream copy_stream;                  // tokens of finished chunks to pinned host memory (JTK_ENCODE_TO_HOST)
    Event ev_fork, ev_copy;
    Pinned<int64_t> h_info;              // device-visible: per chunk, its first token and the end of its last
    ChunkSet set[MAX_SETS];
    int n_sets = 2;                      // chunks in flight (JTK_OPT_CHUNKS_IN_FLIGHT)
    bool n_sets_chosen = false;          // by the caller or the environment (else a job that streams ids to the host takes 3)
    int64_t chunk_bytes = (int64_t)1 << 30;    // JTK_OPT_CHUNK_BYTES: device-resident input (large chunks: fewer launches and kernel tails)
    int64_t host_chunk_bytes = (int64_t)32 << 20;   // JTK_OPT_HOST_CHUNK_BYTES: host input (small chunks: copies overlap kernels)
    // the whole batch
    DevBuf in_text, in_off;          // device copy of host input (host-buffer entry point)
    DevBuf in_pieces;                // caller-supplied pieces (jtk_batch_encode_pieces): begin[n] | end[n]
    // One allocation holds everything a job hands back: JtkResult + running token totals per chunk | status per document |
    // token offsets | token ids.  A small job's whole answer is then ONE copy to the host, and its header one memset.
    DevBuf out;
    struct View { void* p = nullptr; };
    View job, status, tok_off, tokens;   // where those parts are in `out` for the last job
    DevBuf plan;                     // chunk plan of a device-resident batch
    Pinned<int64_t> host_plan;
    std::vector<int64_t> chunk_doc, chunk_off;
    // JTK_OPT_REUSE_CHUNK_PLAN: the plan of the last device-resident batch is kept while the same offsets array (same pointer, counts)
    // is encoded again -- a step loop --, which saves the plan kernel and the call's only synchronisation.  The caller promises
    // not to change the offsets in place; if it does, the chunks' first and last documents no longer sit where the plan says and
    // k_mark_docs reports JTK_ERR_INVALID_ARGUMENT -- never a wrong answer.
    const int64_t* plan_doc_off = nullptr;
    int64_t plan_docs = -1, plan_bytes = -1, plan_chunk_bytes = -1;
    bool reuse_plan = false;             // JTK_OPT_REUSE_CHUNK_PLAN
    // results streamed to pinned host memory (JTK_ENCODE_TO_HOST)
    Pinned<int32_t> h_tokens;
    Pinned<int64_t> h_tok_off;
    Pinned<int32_t> h_status;
    Pinned<uint8_t> h_small;         // a small job's whole `out` block
    Pinned<uint8_t> h_in;            // a tiny host job's offsets and text, side by side
    Pinned<uint8_t> h_gather;        // jtk_batch_encode_max_tokens: the documents' leading bytes, gathered
    // where the host copy of the last job's result is: the buffers above, or inside h_small
    const int32_t* r_tokens = nullptr; const int64_t* r_tok_off = nullptr; int32_t* r_status = nullptr;
    bool have_host_result = false;
    // JTK_ENCODE_COMPACT_IDS: the host copy is two planes -- lo in h_tokens (or inside h_small), hi in h_hi (or h_small) -- and
    // there are no int32 ids in host memory; cp_stage: one chunk's planes on the device (lo | hi), compacted and copied on
    // copy_stream (in order: the next chunk's pass follows this chunk's copies)
    bool host_compact = false;
    Pinned<uint32_t> h_hi;
    const uint16_t* r_lo = nullptr; const uint32_t* r_hi = nullptr;
    DevBuf cp_stage;
    // batch decode (jtk_batch_decode*)
    DevBuf dec_in_ids, dec_in_off, dec_zero, dec_tile, dec_pre, dec_out, dec_byte_off;
    DevBuf dec_first, dec_in_win, dec_cell;   // jtk_batch_decode_rows*: first stop column per row | host begin, end | cell_byte for the host
    DevBuf trunc_kept, trunc_flag;   // jtk_batch_truncate
    DevBuf mt_scratch, mt_gather;    // jtk_batch_encode_device_max_tokens: per-document state of the rounds | the gathered prefixes
    Pinned<int64_t> h_mt;            // the round's (open documents, gathered bytes)
    bool have_trunc = false;
    // jtk_batch_chunk: hdr | per-document scan, long list, bases | tiles of the byte scan | records
    DevBuf ck_scratch, ck_tiles, ck_rec;
    DevBuf ck_plane;                     // jtk_batch_chunk_prefer: the level of the cut before every token
    const uint8_t* ck_end_level = nullptr;   // end_level[n_chunks] in ck_rec when the chunk result is jtk_batch_chunk_prefer's
    Pinned<int64_t> h_ck;                // (chunks, tokens) read once per call
    JtkChunkWork ck{};
    bool have_chunk = false, have_tiles = false;
    hipStream_t ck_stream = nullptr;     // stream of the last chunk plan
    Event ev_ck;                         // orders a chunk call's stream after the encode / the plan
    // jtk_batch_pack: hdr | P | SEG | RS | flag | lifting table (its own scratch: pack and chunk results outlive each other)
    DevBuf pk_scratch;
    Pinned<int64_t> h_pk;            // the plan's hdr, read once per call
    JtkPackWork pk{};
    bool have_pack = false;
    hipStream_t pk_stream = nullptr;     // stream of the last pack plan
    // jtk_batch_char_*: the rank / select index over the last encode's text for cp_unit (-1: none; a new encode drops it, a call
    // with another unit rebuilds it): sup [n_sup + 1] | dunit [n_docs + 1] (i64) | superblock totals [n_sup] (u32) | sub (u16)
    DevBuf cp_buf;
    JtkCharIndex cp{};
    int64_t* cp_dunit = nullptr;
    int cp_unit = -1;
    hipStream_t cp_stream = nullptr;     // stream of the last call that built or read the index
    // UTF-16 in and out (jtk_utf16.hip).  E: scratch (hdr | tile_off | tile counts | sub), the host form's input (units |
    // offsets), and two results, each UTF-8 text + doc_off: u16_tx_* of the last jtk_batch_transcode_utf16_device (valid until the
    // next one), u16_enc_* of the last jtk_batch_encode_utf16* (the encode's text: alive until the next such encode, whatever is
    // transcoded in between).  D: scratch and the units + unit_off of the last jtk_batch_decode_utf16.
    DevBuf u16_scratch, u16_in, u16_tx_text, u16_tx_off, u16_enc_text, u16_enc_off, u16_dscratch, u16_units, u16_unit_off;
    const uint8_t* u16_last_text = nullptr;   // jtk_batch_utf8_device_result: the last transcode of either kind
    const int64_t* u16_last_off = nullptr;
    int64_t u16_last_bytes = 0, u16_dec_units = 0, u16_dec_seqs = 0;
    bool have_u16 = false, have_u16_dec = false;
    hipStream_t u16_stream = nullptr;    // stream of the last transcode: the next one, on another stream, reuses its scratch behind it
    // JTK_ENCODE_ALLOW_SPECIAL (jtk_special.hip): the allowed set per literal of the encoding (a new batch allows all) and its
    // device copy; find scratch (hdr | the stitched status | per-block counts), candidates and sub-documents, the stitched result
    std::vector<uint8_t> sp_allowed;
    bool sp_dirty = true;
    DevBuf sp_lits;                  // ids [n] (int32) | allowed [n]
    DevBuf sp_find, sp_cand, sp_out;
    Pinned<int64_t> h_sp;            // (candidates, bad offsets, refusals) read once per call
    // JTK_ENCODE_FIM (jtk_fim.hip): the parameters (jtk_batch_set_fim) and, alive with the encode's result, hdr | the stitched
    // status | sub_off | cut | part_tok | kind; the stitched tokens and offsets share sp_out with allow-special
    jtk_fim_params fim{};
    bool fim_set = false, have_fim = false;
    DevBuf fim_buf;
    const uint8_t* fim_kind = nullptr;
    const int64_t* fim_cut = nullptr;
    const int64_t* fim_part_tok = nullptr;
    JtkDecodeWork dwork{};
    bool have_decode = false;
    int64_t dec_total = 0;
    int64_t dec_rows_width = -1;         // width of the last decode when it was a rows decode, -1 after a flat one
    // jtk_batch_decode_find_stops: keys [2 n] | stop_pos [n] | stop_col [n] (i64) | stop_which [n] | hold [n] (i32)
    DevBuf stop_buf;
    JtkStopWork stop{};
    bool have_stops = false;
    hipStream_t stop_stream = nullptr;   // stream of the last find_stops: the fetch waits for it
    // jtk_batch_ngram_repeats (jtk_repeat.hip): the table of one group of documents (key | count | first, jtk_rp_table_at), reused
    // from group to group and from call to call; the packed top word per document; the host copy of tok_off | status that the
    // groups are planned from.  ev_rp is recorded behind every pass: the next one, maybe on another stream, reuses the table
    // behind it, and the batch is not freed before it.
    DevBuf rp_table, rp_top;
    Pinned<uint8_t> h_rp;
    Event ev_rp;
    bool rp_queued = false;
    int64_t rp_table_bytes = (int64_t)256 << 20;   // JTK_OPT_REPEAT_TABLE_BYTES
    // jtk_batch_line_units / jtk_batch_line_repeats (jtk_lines.hip): ln_scratch = the two bit planes | the tiles' summaries and
    // carries | the per-document entries and offsets | hdr; ln_units = six 8-byte arrays per unit (begin, end, k, chars, and the two
    // prefixes at the end byte), allocated at the counted size.  The list is the last encode's for ln_p (unit, JTK_LINES_TRIM,
    // seed, doc_index_base): a new encode drops it, a call with other parameters replaces it.  The repeats share rp_table, rp_top
    // and ev_rp with jtk_batch_ngram_repeats: whichever pass comes next waits for the one before it.
    DevBuf ln_scratch, ln_units;
    Pinned<int64_t> h_ln;
    JtkLnWork ln{};
    jtk_lines_params ln_p{};
    bool have_lines = false;
    hipStream_t ln_stream = nullptr;     // stream of the last call that built or read the list
    JtkResult* host_result = nullptr;   // host_result_own, or the head of h_small after a small job
    Pinned<JtkResult> host_result_own;
    // the last job
    const uint8_t* job_text = nullptr;
    const int64_t* job_doc_off = nullptr;
    int64_t job_docs = 0, job_bytes = 0;
    uint32_t job_flags = 0;
    bool have_result = false, synced = false;
    bool job_pieces = false;             // the last encode took caller-supplied pieces (jtk_batch_encode_pieces)
    bool profiling = false;
    std::vector<Event> prof_ev;          // [chunk][stage][start, end]
    int prof_chunks = 0;                 // chunks of the last job that recorded events
};

// What a batch holds exists relative to its last encode, or to its last decode.  These two are the only places that give it up
// on behalf of another call (a pass that replaces its own result -- chunk, pack, the char index, UTF-16 out, stops -- clears
// its own flag and no other).  Every encode / decode entry calls its one at the point of no return: behind the checks that
// read only the arguments, before the first allocation, copy or launch that can touch memory the old result lives in.  A call
// that fails past that point leaves no result.
static void drop_encode_result(jtk_batch* b) {
    b->have_result = b->have_host_result = b->have_trunc = b->have_chunk = b->have_tiles = b->have_pack = b->have_fim = false;
    b->cp_unit = -1;
    b->have_lines = false;
    b->ck_end_level = nullptr;
    b->synced = false;
}
static void drop_decode_result(jtk_batch* b) {
    b->have_decode = b->have_u16_dec = b->have_stops = false;
    b->dec_rows_width = -1;
}

static hipStream_t pick_stream(const jtk_batch* b, void* stream_or_null) { return stream_or_null ? (hipStream_t)stream_or_null : b->stream.h; }

// what a pass over the last encode needs of it, besides that there is one
enum : unsigned { NEED_IDS = 1,         // token ids (the encode was not count-only)
                  NEED_TEXT_POS = 2,    // positions that are positions in the text (it did not take caller-supplied pieces)
                  NEED_TEXT_ORDER = 4 };// tokens in the order of the text's bytes (it did not rearrange the documents: JTK_ENCODE_FIM)
static int need_encode(const jtk_batch* b, unsigned what) {
    if (!b || !b->have_result) return fail(JTK_ERR_INVALID_ARGUMENT, "no batch encode result on this batch (jtk_batch_encode_device_max_tokens leaves none)");
    if ((what & NEED_IDS) && (b->job_flags & JTK_ENCODE_COUNT_ONLY)) return fail(JTK_ERR_INVALID_ARGUMENT, "the last encode was count-only: there are no token ids");
    if ((what & NEED_TEXT_POS) && b->job_pieces)
        return fail(JTK_ERR_INVALID_ARGUMENT, "the last encode took caller-supplied pieces: its positions are positions in the decoded stream, not in the text");
    if ((what & (NEED_TEXT_POS | NEED_TEXT_ORDER)) && (b->job_flags & JTK_ENCODE_FIM))
        return fail(JTK_ERR_INVALID_ARGUMENT, "the last encode was a JTK_ENCODE_FIM encode: its tokens are rearranged around sentinel ids and have no positions in the text");
    return JTK_OK;
}

static int sync_last(jtk_batch* b) {     // the host waits for the last encode, once (to read its header, or to rewrite its inputs)
    if (!b->synced) { HIP_TRY(hipStreamSynchronize(b->last_stream)); b->synced = true; }
    return JTK_OK;
}

#include "jtk_unicode_tables.h"
#include "jtk_block_classify.h"

// Host loops over many documents (the gather of the prefixes and the decisions of the maxTokens early exit): slices of
// [0, n) on up to 8 threads when there is enough to share out.
template <class F> static void host_slices(size_t n, F&& fn) {
    unsigned nt = std::thread::hardware_concurrency();
    nt = nt > 8 ? 8 : (nt < 1 ? 1 : nt);
    if (n < 16384 || nt == 1) { fn(0, (size_t)0, n); return; }
    std::vector<std::thread> th;
    for (unsigned k = 0; k < nt; k++) th.emplace_back([&, k] { fn((int)k, n * k / nt, n * (k + 1) / nt); });
    for (auto& t : th) t.join();
}

// encode()'s special-token check on the host (GptBytePairEncoding.java:52-56: text.contains(literal), per document) for the entry
// points whose text does not pass through k_pretok_split whole: one memchr pass per distinct FIRST byte of the literals (one
// pass for the shipped encodings: every literal starts with '<'), byte ranges shared out over the host threads.
static void find_special_docs(const jtk_encoding* enc, const uint8_t* utf8, int64_t n_bytes, const int64_t* doc_off, int64_t n_docs,
                              std::vector<uint8_t>& flag) {
    flag.assign((size_t)(n_docs > 0 ? n_docs : 1), 0);
    const auto& sp = enc->host.specials;
    if (sp.empty() || n_bytes <= 0) return;
    bool first[256] = {false};
    for (auto& x : sp) if (!x.first.empty()) first[(uint8_t)x.first[0]] = true;
    const size_t slice = (size_t)1 << 22;
    const size_t n_slices = ((size_t)n_bytes + slice - 1) / slice;
    host_slices(n_slices, [&](int, size_t lo, size_t hi) {
        const int64_t b0 = (int64_t)(lo * slice), b1 = std::min<int64_t>(n_bytes, (int64_t)(hi * slice));   // hits that START in [b0, b1)
        for (int fb = 0; fb < 256; fb++) {
            if (!first[fb]) continue;
            const uint8_t* p = utf8 + b0;
            const uint8_t* const endp = utf8 + b1;
            while (p < endp) {
                p = (const uint8_t*)memchr(p, fb, (size_t)(endp - p));
                if (!p) break;
                const int64_t pos = p - utf8;
                for (auto& x : sp) {
                    const std::string& lit = x.first;
                    if (lit.empty() || (uint8_t)lit[0] != (uint8_t)fb || pos + (int64_t)lit.size() > n_bytes) continue;
                    if (memcmp(p, lit.data(), lit.size()) != 0) continue;
                    const int64_t d = (std::upper_bound(doc_off, doc_off + n_docs + 1, pos) - doc_off) - 1;
                    if (d >= 0 && d < n_docs && pos + (int64_t)lit.size() <= doc_off[d + 1]) flag[(size_t)d] = 1;   // (one value: a benign race)
                }
                p++;
            }
        }
    });
}



extern "C" {

const char* jtk_version(void) { return "jtokkit_amd 0.1 (gfx950; Unicode " JTK_UNICODE_VERSION " class tables)"; }
const char* jtk_last_error(void) { return g_err.c_str(); }

int jtk_device_count(void) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) return fail(JTK_ERR_NO_DEVICE, std::string("hipGetDeviceCount: ") + hipGetErrorString(e));
    return n;
}

int jtk_encoding_create(const char* name, int pattern_kind, const uint8_t* tiktoken, size_t tiktoken_len,
                        const char* const* special_literals, const int32_t* special_ids, int n_specials,
                        int device, jtk_encoding** out) {
    if (!out) return fail(JTK_ERR_INVALID_ARGUMENT, "out is NULL");
    *out = nullptr;
    if (!tiktoken || n_specials < 0 || (n_specials > 0 && (!special_literals || !special_ids)))
        return fail(JTK_ERR_INVALID_ARGUMENT, "bad arguments");
    if (n_specials > JTK_MAX_SPECIALS) return fail(JTK_ERR_INVALID_ARGUMENT, "too many special tokens");
    for (int i = 0; i < n_specials; i++) {
        const size_t l = strlen(special_literals[i]);
        if (l < 1 || l > JTK_SPECIAL_MAXLEN)
            return fail(JTK_ERR_INVALID_ARGUMENT, "special-token literals must be 1..65535 bytes long");
        if (special_ids[i] < 0 || special_ids[i] > JTK_MAX_SPECIAL_ID)
            return fail(JTK_ERR_INVALID_ARGUMENT, "special-token id out of range");
    }
    std::unique_ptr<jtk_encoding> enc(new (std::nothrow) jtk_encoding());      // (its members free themselves on every return)
    if (!enc) return fail(JTK_ERR_OUT_OF_MEMORY, "out of host memory");
    std::string err;
    int rc = jtk_build_tables(name, pattern_kind, tiktoken, tiktoken_len, special_literals, special_ids, n_specials,
                              enc->host, err);
    if (rc != JTK_OK) return fail(rc, err);
    enc->tok_len.assign((size_t)enc->host.max_id + 1 + (size_t)enc->host.n_missing, 1);     // (pseudo ids: one byte each)
    {   // the largest id a result can hold: table ids, the pseudo ids above them, every special id
        int64_t top = (int64_t)enc->host.max_id + (int64_t)enc->host.n_missing;
        for (auto& sp : enc->host.specials) top = std::max<int64_t>(top, sp.second);
        enc->hb = jtk_compact_hb(top);
    }
    for (size_t i = 0; i <= (size_t)enc->host.max_id; i++) enc->tok_len[i] = (uint32_t)enc->host.id_to_bytes[i].size();

    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(JTK_ERR_NO_DEVICE, "no HIP device: jtokkit_amd has no CPU path");
    if (device < 0 || device >= ndev) return fail(JTK_ERR_INVALID_ARGUMENT, "device index out of range");
    enc->device = device;
    HIP_TRY(hipSetDevice(device));
    const size_t tok8_bytes = (enc->host.tok8.size() * sizeof(JtkTok8Slot) + 31) & ~(size_t)31;
    // the Unicode class table as pretok_split stages it in LDS (JtkDeviceTables::uc_lds_image)
    std::vector<uint8_t> uc_image;
    if (sizeof(jtk_uc_stage1_init) <= JTK_UC_LDS_STAGE1 && JTK_UC_LDS_STAGE1 + sizeof(jtk_uc_stage2_init) <= (size_t)JTK_UC_LDS_UNITS * 16) {
        uc_image.assign((size_t)JTK_UC_LDS_UNITS * 16, 0);
        memcpy(uc_image.data(), jtk_uc_stage1_init, sizeof(jtk_uc_stage1_init));
        memcpy(uc_image.data() + JTK_UC_LDS_STAGE1, jtk_uc_stage2_init, sizeof(jtk_uc_stage2_init));
    }
    if (enc->uc1.ensure(sizeof(jtk_uc_stage1_init)) || enc->uc2.ensure(sizeof(jtk_uc_stage2_init)) ||
        enc->uclds.ensure(uc_image.size() + 16) || enc->splittab.ensure(256 * sizeof(JtkCode4)) ||
        enc->brank.ensure(256 * 4) || enc->pairs.ensure(enc->host.pair_buckets.size() * sizeof(JtkPairBucket)) ||
        // the two whole-piece tables live in one allocation (tok8 slots, then tok16 slots): piece_resolve addresses both with
        // one base and a 32-bit offset; + 32: a 9..16-byte probe of the last slot may read 16 bytes past a 16-byte slot
        enc->tok8.ensure(tok8_bytes + enc->host.tok16.size() * sizeof(JtkTok16Slot) + 32) ||
        enc->bprank.ensure(65536 * 4) ||
        enc->bpbits.ensure(1024 * 8) || enc->bpcum.ensure(1024 * 2) || enc->bpranks.ensure(JTK_BP_MAX * 4) || enc->pairin.ensure(2048 * 4)) return JTK_ERR_OUT_OF_MEMORY;
    HIP_TRY(hipMemcpy(enc->uc1.p, jtk_uc_stage1_init, sizeof(jtk_uc_stage1_init), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(enc->uc2.p, jtk_uc_stage2_init, sizeof(jtk_uc_stage2_init), hipMemcpyHostToDevice));
    if (!uc_image.empty()) HIP_TRY(hipMemcpy(enc->uclds.p, uc_image.data(), uc_image.size(), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(enc->brank.p, enc->host.byte_rank, 256 * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(enc->pairs.p, enc->host.pair_buckets.data(), enc->host.pair_buckets.size() * sizeof(JtkPairBucket), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(enc->tok8.p, enc->host.tok8.data(), enc->host.tok8.size() * sizeof(JtkTok8Slot), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy((uint8_t*)enc->tok8.p + tok8_bytes, enc->host.tok16.data(), enc->host.tok16.size() * sizeof(JtkTok16Slot), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(enc->bprank.p, enc->host.bp_rank.data(), 65536 * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(enc->bpbits.p, enc->host.bp_bits.data(), 1024 * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(enc->bpcum.p, enc->host.bp_cum.data(), 1024 * 2, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(enc->bpranks.p, enc->host.bp_ranks.data(), JTK_BP_MAX * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(enc->pairin.p, enc->host.pair_in_token.data(), 2048 * 4, hipMemcpyHostToDevice));
    {   // decode table: byte strings of all ids (rank table + special tokens, GptBytePairEncoding.java:302-314) back to back
        uint32_t n_ids = enc->host.max_id + 1;
        for (auto& sp : enc->host.specials) if (sp.second >= 0 && (uint32_t)sp.second + 1 > n_ids) n_ids = (uint32_t)sp.second + 1;
        std::vector<const std::string*> str(n_ids, nullptr);
        for (uint32_t i = 0; i <= enc->host.max_id; i++) if (enc->host.id_present[i]) str[i] = &enc->host.id_to_bytes[i];
        for (auto& sp : enc->host.specials) if (sp.second >= 0 && !str[(size_t)sp.second]) str[(size_t)sp.second] = &sp.first;
        std::vector<uint32_t> off(n_ids + 1, 0);
        std::string blob;
        for (uint32_t i = 0; i < n_ids; i++) { off[i] = (uint32_t)blob.size(); if (str[i]) blob += *str[i]; }
        off[n_ids] = (uint32_t)blob.size();
        blob.append(16, '\0');
        if (enc->dec_off.ensure(off.size() * 4) || enc->dec_blob.ensure(blob.size())) return JTK_ERR_OUT_OF_MEMORY;
        HIP_TRY(hipMemcpy(enc->dec_off.p, off.data(), off.size() * 4, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(enc->dec_blob.p, blob.data(), blob.size(), hipMemcpyHostToDevice));
        enc->n_ids_table = n_ids;
        std::vector<uint32_t> bits((n_ids + 31) / 32 + 1, 0);
        for (uint32_t i = 0; i < n_ids; i++)
            if (!str[i] || str[i]->empty() || ((uint8_t)(*str[i])[0] & 0xC0) != 0x80) bits[i >> 5] |= 1u << (i & 31);
        if (enc->bnd.ensure(bits.size() * 4)) return JTK_ERR_OUT_OF_MEMORY;
        HIP_TRY(hipMemcpy(enc->bnd.p, bits.data(), bits.size() * 4, hipMemcpyHostToDevice));
    }
    if (!enc->host.long_tok.empty()) {
        if (enc->longtok.ensure(enc->host.long_tok.size() * sizeof(JtkLongTokSlot)) || enc->longblob.ensure(enc->host.long_blob.size())) return JTK_ERR_OUT_OF_MEMORY;
        HIP_TRY(hipMemcpy(enc->longtok.p, enc->host.long_tok.data(), enc->host.long_tok.size() * sizeof(JtkLongTokSlot), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(enc->longblob.p, enc->host.long_blob.data(), enc->host.long_blob.size(), hipMemcpyHostToDevice));
    }
    JtkDeviceTables& dt = enc->dt;
    memset(&dt, 0, sizeof(dt));
    dt.longtok.slots = (const JtkLongTokSlot*)enc->longtok.p;
    dt.longtok.blob = (const uint8_t*)enc->longblob.p;
    dt.longtok.n = (uint32_t)enc->host.long_tok.size();
    dt.longtok.max_len = enc->host.long_max_len;
    dt.uc.stage1 = (const uint8_t*)enc->uc1.p;
    dt.uc.stage2 = (const uint32_t*)enc->uc2.p;
    dt.uc_lds_image = uc_image.empty() ? nullptr : (const uint32_t*)enc->uclds.p;
    dt.split_tab = (const uint32_t*)enc->splittab.p;
    dt.byte_rank = (const uint32_t*)enc->brank.p;
    dt.pairs.buckets = (const JtkPairBucket*)enc->pairs.p;
    dt.pairs.bits = enc->host.pair_bits;
    dt.tok8.slots = (const JtkTok8Slot*)enc->tok8.p;
    dt.tok8.bits = enc->host.tok8_bits;
    dt.tok16.slots = (const JtkTok16Slot*)((const uint8_t*)enc->tok8.p + tok8_bytes);
    dt.tok16.n = enc->host.tok16_n;
    dt.bp_rank = (const uint32_t*)enc->bprank.p;
    dt.bp.bits = (const uint64_t*)enc->bpbits.p;
    dt.bp.cum = (const uint16_t*)enc->bpcum.p;
    dt.bp.ranks = (const uint32_t*)enc->bpranks.p;
    dt.pair_in_token = (const uint32_t*)enc->pairin.p;
    dt.kind = pattern_kind;
    dt.pseudo_base = enc->host.n_missing ? enc->host.pseudo_base : 0u;
    dt.n_specials = n_specials;
    {   // the literals for the device's text.contains check: offsets [n + 1] (u32), then the bytes
        std::vector<uint32_t> off((size_t)n_specials + 1, 0);
        std::vector<uint8_t> blob;
        for (int i = 0; i < n_specials; i++) {
            const size_t l = strlen(special_literals[i]);
            blob.insert(blob.end(), (const uint8_t*)special_literals[i], (const uint8_t*)special_literals[i] + l);
            off[(size_t)i + 1] = (uint32_t)blob.size();
            const uint8_t f = (uint8_t)special_literals[i][0];
            dt.special_first[f >> 5] |= 1u << (f & 31);
        }
        const size_t off_bytes = align_up(off.size() * 4, 16);
        if (enc->specials.ensure(off_bytes + blob.size() + 16)) return JTK_ERR_OUT_OF_MEMORY;
        HIP_TRY(hipMemcpy(enc->specials.p, off.data(), off.size() * 4, hipMemcpyHostToDevice));
        if (!blob.empty()) HIP_TRY(hipMemcpy((uint8_t*)enc->specials.p + off_bytes, blob.data(), blob.size(), hipMemcpyHostToDevice));
        dt.special_off = (const uint32_t*)enc->specials.p;
        dt.special_blob = (const uint8_t*)enc->specials.p + off_bytes;
    }
    {   // pretok_split's per-byte flag table, with the literals' first bytes and the all-letter lead bytes in it
        const JtkUcTables host_uc{jtk_uc_stage1_init, jtk_uc_stage2_init};
        uint32_t lead_letters[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (uint32_t b = 0; b < 256; b++) if (jtk_lead_all_letters(host_uc, b)) lead_letters[b >> 5] |= 1u << (b & 31);
        JtkCode4 tab[256];
        jtk_build_code4_table(pattern_kind == JTK_PAT_CL100K, dt.special_first, lead_letters, tab);
        HIP_TRY(hipMemcpy(enc->splittab.p, tab, sizeof(tab), hipMemcpyHostToDevice));
    }
    *out = enc.release();
    return JTK_OK;
}

void jtk_encoding_destroy(jtk_encoding* enc) {
    if (!enc) return;
    (void)hipSetDevice(enc->device);
    delete enc;
}
const char* jtk_encoding_name(const jtk_encoding* enc) { return enc ? enc->host.name.c_str() : ""; }
int jtk_encoding_device(const jtk_encoding* enc) { return enc ? enc->device : -1; }
int64_t jtk_encoding_vocab_size(const jtk_encoding* enc) { return enc ? enc->host.n_tokens : 0; }
int64_t jtk_encoding_pair_count(const jtk_encoding* enc) { return enc ? enc->host.n_pairs : 0; }
int jtk_encoding_id_bits(const jtk_encoding* enc) { return enc ? 16 + enc->hb : 0; }

int jtk_batch_create(const jtk_encoding* enc, jtk_batch** out) {
    if (!enc || !out) return fail(JTK_ERR_INVALID_ARGUMENT, "bad arguments");
    *out = nullptr;
    HIP_TRY(hipSetDevice(enc->device));
    jtk_batch* b = new (std::nothrow) jtk_batch();
    if (!b) return fail(JTK_ERR_OUT_OF_MEMORY, "out of host memory");
    b->enc = enc;
    b->sp_allowed.assign(enc->host.specials.size(), 1);
    if (const char* e = getenv("JTK_CHUNK_BYTES")) { const long long v = atoll(e); if (v >= (1 << 20)) b->chunk_bytes = v; }
    if (const char* e = getenv("JTK_HOST_CHUNK_BYTES")) { const long long v = atoll(e); if (v >= (1 << 16)) b->host_chunk_bytes = v; }
    if (const char* e = getenv("JTK_CHUNKS_IN_FLIGHT")) { const int v = atoi(e); if (v >= 1 && v <= MAX_SETS) { b->n_sets = v; b->n_sets_chosen = true; } }
    hipError_t e = b->stream.create();
    if (e == hipSuccess) e = b->host_result_own.alloc(sizeof(JtkResult));
    b->host_result = b->host_result_own.p;
    // (the streams and events of the chunk pipeline are created by the first job that forks: a batch that only ever sees
    // small single-chunk jobs -- one per caller thread in the per-call shape -- owns one stream, not six)
    if (e != hipSuccess) {
        jtk_batch_destroy(b);
        return fail(JTK_ERR_HIP, std::string("batch create: ") + hipGetErrorString(e));
    }
    *out = b;
    return JTK_OK;
}

void jtk_batch_destroy(jtk_batch* b) {
    if (!b) return;
    (void)hipSetDevice(b->enc->device);
    if (b->stream) (void)hipStreamSynchronize(b->stream);
    for (ChunkSet& cs : b->set)
        if (cs.stream) (void)hipStreamSynchronize(cs.stream);
    if (b->copy_stream) (void)hipStreamSynchronize(b->copy_stream);
    if (b->rp_queued) (void)hipEventSynchronize(b->ev_rp);      // (the last repeats pass may be on a caller's stream)
    delete b;                        // (every wait above comes before the first free: the members free themselves here)
}

int jtk_batch_set_option(jtk_batch* b, int option, int64_t value) {
    if (!b) return fail(JTK_ERR_INVALID_ARGUMENT, "batch is NULL");
    switch (option) {
        case JTK_OPT_CHUNK_BYTES:
            if (value < (1 << 16)) return fail(JTK_ERR_INVALID_ARGUMENT, "chunk size must be at least 64 KiB");
            b->chunk_bytes = value;
            return JTK_OK;
        case JTK_OPT_HOST_CHUNK_BYTES:
            if (value < (1 << 16)) return fail(JTK_ERR_INVALID_ARGUMENT, "chunk size must be at least 64 KiB");
            b->host_chunk_bytes = value;
            return JTK_OK;
        case JTK_OPT_CHUNKS_IN_FLIGHT:
            if (value < 1 || value > MAX_SETS) return fail(JTK_ERR_INVALID_ARGUMENT, "chunks in flight: 1..4");
            b->n_sets = (int)value;
            b->n_sets_chosen = true;
            return JTK_OK;
        case JTK_OPT_REUSE_CHUNK_PLAN:
            b->reuse_plan = value != 0;
            b->plan_doc_off = nullptr;
            return JTK_OK;
        case JTK_OPT_REPEAT_TABLE_BYTES:
            if (value < JTK_RP_MIN_TABLE_BYTES) return fail(JTK_ERR_INVALID_ARGUMENT, "repeat table budget must be at least 1280 bytes (64 slots)");
            b->rp_table_bytes = value;
            return JTK_OK;
        default: return fail(JTK_ERR_INVALID_ARGUMENT, "unknown option");
    }
}

int jtk_batch_set_profiling(jtk_batch* b, int enabled) {
    if (!b) return fail(JTK_ERR_INVALID_ARGUMENT, "batch is NULL");
    b->profiling = enabled != 0;
    b->prof_chunks = 0;
    return JTK_OK;
}

int jtk_batch_set_allowed_special(jtk_batch* b, const int32_t* special_ids, int n) {
    if (!b || (n > 0 && !special_ids)) return fail(JTK_ERR_INVALID_ARGUMENT, "bad arguments");
    const auto& sp = b->enc->host.specials;
    std::vector<uint8_t> allowed(sp.size(), n < 0 ? 1 : 0);
    for (int k = 0; k < n; k++) {
        bool known = false;
        for (size_t i = 0; i < sp.size(); i++)
            if (sp[i].second == special_ids[k]) { allowed[i] = 1; known = true; }   // (every literal of the id)
        if (!known) return fail(JTK_ERR_INVALID_ARGUMENT, "id " + std::to_string(special_ids[k]) + " is not a special token of this encoding");
    }
    // (the device copy is rewritten by the next allow-special encode: the last one's kernels must be done reading it)
    HIP_TRY(hipSetDevice(b->enc->device));
    int rc;
    if (b->have_result && (rc = sync_last(b))) return rc;
    b->sp_allowed.swap(allowed);
    b->sp_dirty = true;
    return JTK_OK;
}

int jtk_batch_set_fim(jtk_batch* b, const jtk_fim_params* params) {
    if (!b) return fail(JTK_ERR_INVALID_ARGUMENT, "batch is NULL");
    if (!params) { b->fim_set = false; return JTK_OK; }
    const int32_t ids[3] = {params->prefix_id, params->middle_id, params->suffix_id};
    const char* const names[3] = {"prefix_id", "middle_id", "suffix_id"};
    for (int k = 0; k < 3; k++) {
        bool known = false;
        for (auto& sp : b->enc->host.specials) known = known || sp.second == ids[k];
        if (!known) return fail(JTK_ERR_INVALID_ARGUMENT, std::string(names[k]) + " " + std::to_string(ids[k]) + " is not a special token of this encoding");
    }
    b->fim = *params;                // (read by the host when an encode is queued: the kernels take copies)
    b->fim_set = true;
    return JTK_OK;
}

int jtk_batch_fim_result(jtk_batch* b, const uint8_t** d_kind, const int64_t** d_cut, const int64_t** d_part_tok) {
    if (!b || !b->have_result || !b->have_fim) return fail(JTK_ERR_INVALID_ARGUMENT, "the last encode on this batch did not run with JTK_ENCODE_FIM");
    if (d_kind) *d_kind = b->fim_kind;
    if (d_cut) *d_cut = b->fim_cut;
    if (d_part_tok) *d_part_tok = b->fim_part_tok;
    return JTK_OK;
}

int jtk_batch_fim_result_fetch(jtk_batch* b, uint8_t* kind, int64_t* cut, int64_t* part_tok) {
    if (!b || !b->have_result || !b->have_fim) return fail(JTK_ERR_INVALID_ARGUMENT, "the last encode on this batch did not run with JTK_ENCODE_FIM");
    HIP_TRY(hipSetDevice(b->enc->device));
    if (int rc = sync_last(b)) return rc;
    const size_t n = (size_t)b->job_docs;
    if (n == 0) return JTK_OK;
    if (kind) HIP_TRY(hipMemcpy(kind, b->fim_kind, n, hipMemcpyDeviceToHost));
    if (cut) HIP_TRY(hipMemcpy(cut, b->fim_cut, n * 16, hipMemcpyDeviceToHost));
    if (part_tok) HIP_TRY(hipMemcpy(part_tok, b->fim_part_tok, n * 24, hipMemcpyDeviceToHost));
    return JTK_OK;
}

int jtk_host_alloc(size_t bytes, void** out) {
    if (!out) return fail(JTK_ERR_INVALID_ARGUMENT, "out is NULL");
    *out = nullptr;
    hipError_t e = hipHostMalloc(out, bytes ? bytes : 1, hipHostMallocDefault);
    if (e != hipSuccess) return fail(JTK_ERR_OUT_OF_MEMORY, std::string("hipHostMalloc: ") + hipGetErrorString(e));
    return JTK_OK;
}
void jtk_host_free(void* p) { if (p) (void)hipHostFree(p); }

}  // extern "C"

namespace {

// scratch of one chunk of `n_bytes` (from its tile-aligned origin) and `n_docs` documents; fills cs.work
int prepare_set(ChunkSet& cs, int64_t n_bytes, int64_t n_docs, size_t* bytes_to_clear) {
    JtkWork& w = cs.work;
    w.n_bytes = n_bytes;
    w.n_docs = n_docs;
    w.n_words = (n_bytes + 1 + 63) / 64 + 2;
    w.n_tiles = (n_bytes + 1 + JTK_TILE - 1) / JTK_TILE;
    const size_t mask_bytes = (size_t)w.n_words * 8;
    const size_t nt = (size_t)w.n_tiles;
    const size_t qcnt_bytes = (size_t)(JTK_NBINS + 1) * JTK_Q_SHARDS * JTK_QC_STRIDE * 4;
    const size_t zero_bytes = mask_bytes + 32 + qcnt_bytes;
    const size_t n_long_max = (size_t)n_bytes / (JTK_BIN_MAXLEN + 1) + 2;
    const size_t n_giant_max = (size_t)n_bytes / JTK_LONG_CAP + 2;
    const size_t tps = (nt + JTK_Q_SHARDS - 1) / JTK_Q_SHARDS;      // tiles per queue shard
    int rc;
    if ((rc = cs.zeroed.ensure(zero_bytes)) || (rc = cs.piecemask.ensure(mask_bytes)) ||
        (rc = cs.plist.ensure(nt * JTK_TILE * 4)) || (rc = cs.htok.ensure(nt * JTK_TILE * 4 + 64)) ||
        (rc = cs.docpre.ensure(nt * JTK_TILE * 4)) ||
        (rc = cs.tile_np.ensure(align_up(nt * 4, 16) * 2)) || (rc = cs.tile_off.ensure((nt + 1) * 8)) ||
        (rc = cs.q_meta.ensure(nt * 4 * 16)) ||
        (rc = cs.queues.ensure(tps * JTK_Q_SHARDS * ((size_t)(JTK_BIN_CAP0 + JTK_BIN_CAP1 + JTK_BIN_CAP2 + JTK_BIN_CAP3 + JTK_BIN_CAP4 + JTK_BIN_CAP5 + JTK_BIN_CAP6) * 24 + (size_t)JTK_TINY_CAP * 8))) ||
        (rc = cs.mid_list.ensure(n_long_max * sizeof(JtkLongPiece))) ||
        (rc = cs.long_list.ensure(n_long_max * sizeof(JtkLongPiece))) ||
        (rc = cs.giant_list.ensure(n_giant_max * sizeof(JtkLongPiece))))
        return rc;
    uint8_t* z = (uint8_t*)cs.zeroed.p;
    w.docmask = (uint64_t*)z;
    w.mid_count = (uint32_t*)(z + mask_bytes);
    w.long_count = (uint32_t*)(z + mask_bytes + 4);
    w.n_giant = (uint32_t*)(z + mask_bytes + 8);
    w.q_count = (uint32_t*)(z + mask_bytes + 32);
    w.piecemask = (uint64_t*)cs.piecemask.p;
    w.plist = (uint32_t*)cs.plist.p;
    w.htok = (uint32_t*)cs.htok.p;
    w.docpre = (uint32_t*)cs.docpre.p;
    w.tile_np = (uint32_t*)cs.tile_np.p;
    w.tile_tot = (uint32_t*)((uint8_t*)cs.tile_np.p + align_up(nt * 4, 16));
    w.tile_off = (int64_t*)cs.tile_off.p;
    {
        const size_t caps[JTK_NBINS] = {JTK_BIN_CAP0, JTK_BIN_CAP1, JTK_BIN_CAP2, JTK_BIN_CAP3, JTK_BIN_CAP4, JTK_BIN_CAP5, JTK_BIN_CAP6};
        uint8_t* qp = (uint8_t*)cs.queues.p;                      // all the 16-byte arrays first, then the 8-byte ones
        w.q_meta = (uint32_t*)cs.q_meta.p;
        for (int k = 0; k < JTK_NBINS; k++) {
            w.qd[k] = (uint4*)qp;
            w.q_cap[k] = (int64_t)(tps * caps[k]);
            qp += tps * caps[k] * JTK_Q_SHARDS * 16;
        }
        for (int k = 0; k < JTK_NBINS; k++) {
            w.qm[k] = (uint64_t*)qp;
            qp += tps * caps[k] * JTK_Q_SHARDS * 8;
        }
        w.qt = (uint64_t*)qp;
        w.qt_cap = (int64_t)(tps * JTK_TINY_CAP);
    }
    w.mid_list = (JtkLongPiece*)cs.mid_list.p;
    w.long_list = (JtkLongPiece*)cs.long_list.p;
    w.giant_list = (JtkLongPiece*)cs.giant_list.p;
    *bytes_to_clear = zero_bytes;
    return JTK_OK;
}

// The whole job: `chunk_doc` / `chunk_off` (n_chunks + 1 entries, filled by the caller) cut the batch into runs of whole
// documents.  Chunk c runs on scratch set c % n_sets and that set's stream; the sets' streams are forked from the main
// stream `s` and joined into it at the end, so the job as a whole is ordered like one operation on `s`.  The only link
// between chunks is the running token total (chunk c's scan follows chunk c - 1's).
// h_text != NULL: the text comes from host memory, copied chunk by chunk into in_text on the chunk's stream (so the copy of
// chunk c + 1 overlaps the kernels of chunk c).  to_host: every chunk's tokens are copied to the pinned host buffer as
// soon as they are packed.
struct PieceArgs {               // caller-supplied pieces instead of pretok_split
    const int64_t* d_begin; const int64_t* d_end;     // device copies
    const int64_t* h_begin;                           // host: to find each chunk's pieces
    int64_t n;
};

// mt != NULL: the maxTokens decision (jtk_batch_encode_device_max_tokens) runs as every chunk's epilogue, on the chunk's stream
// behind doc_offsets, while the chunk's piece mask is still in its scratch set.
int run_job(jtk_batch* b, const uint8_t* d_text, const uint8_t* h_text, const int64_t* d_doc_off, int64_t n_docs, int64_t n_bytes,
            uint32_t flags, hipStream_t s, bool to_host, const PieceArgs* pieces = nullptr, const JtkMaxTokWork* mt = nullptr) {
    const jtk_encoding* enc = b->enc;
    const int n_chunks = (int)b->chunk_doc.size() - 1;
    // JTK_ENCODE_COMPACT_IDS: what goes to pinned memory is the two planes of jtk_compact_rules.h instead of the int32 ids
    // (a count-only job has no ids either way); the device-side result stays int32
    const bool compact_req = to_host && (flags & JTK_ENCODE_COMPACT_IDS) != 0;
    const bool compact = compact_req && !(flags & JTK_ENCODE_COUNT_ONLY);
    const int hb = enc->hb;
    flags &= ~(uint32_t)JTK_ENCODE_COMPACT_IDS;
    // (ids streamed to the host chunk by chunk: the host waits for a chunk's scan before it can issue that chunk's copy, one
    // chunk behind the enqueueing -- with two sets that wait stalls the pipeline: 404 ms per step on the headline corpus against
    // 163 with three, profiles/r03_experiments/r03bc_e2e_memcpy.txt -- so such a job takes three unless the caller chose)
    const int want_sets = (!b->n_sets_chosen && to_host && h_text && b->n_sets < 3) ? 3 : b->n_sets;   // (host input: small chunks, small sets)
    const int n_sets = n_chunks < want_sets ? (n_chunks < 1 ? 1 : n_chunks) : want_sets;
    int rc;
    // batch-wide buffers
    const size_t status_bytes = align_up((size_t)(n_docs > 0 ? n_docs : 1) * 4, 16);
    const size_t job_bytes = align_up(64 + ((size_t)n_chunks + 2) * 8, 16);
    const size_t off_status = job_bytes, off_tok_off = off_status + status_bytes;
    size_t off_tokens = align_up(off_tok_off + ((size_t)n_docs + 1) * 8, 256);
    // a small single-chunk job (the per-call service's batches) copies its whole output block -- header, status, offsets and
    // the worst-case token range (one token per byte) -- right behind the kernels in ONE copy, instead of waiting for the
    // token count first: one host synchronisation and three copies less per batch
    const bool small_to_host = to_host && n_chunks == 1 && n_bytes <= SMALL_JOB_BYTES;
    // r03: for the smallest of them (a per-call device batch) the output block IS pinned host memory -- pack, doc_offsets and the
    // status atomics write over the link, and the copy up (a DMA of 14 us for 27 documents) is gone.  JTK_TINY_COPY_OUT=1: the copy.
    static const bool copy_out_env = getenv("JTK_TINY_COPY_OUT") != nullptr;
    const bool zero_copy_out = !copy_out_env && small_to_host && n_bytes <= TINY_JOB_BYTES && !h_text && !compact;
    // a small compact job: the planes lie between the offsets and the int32 ids, so that one copy of [0, off_tokens) takes
    // header, status, offsets and both worst-case planes (and not the ids); the tiny job takes this copying path too
    size_t off_lo = 0, off_hi = 0;
    if (compact && small_to_host) {
        off_lo = off_tokens;
        off_hi = off_lo + align_up((size_t)jtk_compact_lo_bytes(n_bytes + 64), 256);
        off_tokens = off_hi + align_up((size_t)jtk_compact_hi_words(n_bytes + 64, hb) * 4, 256);
    }
    uint8_t* out_base;
    if (zero_copy_out) {
        if ((rc = b->h_small.ensure(off_tokens + ((size_t)n_bytes + 64) * 4 + 4096))) return rc;
        out_base = b->h_small.p;
    } else {
        if ((rc = b->out.ensure(off_tokens + ((size_t)n_bytes + 64) * 4))) return rc;
        out_base = (uint8_t*)b->out.p;
    }
    b->job.p = out_base;
    b->status.p = out_base + off_status;
    b->tok_off.p = out_base + off_tok_off;
    b->tokens.p = out_base + off_tokens;
    JtkResult* d_result = (JtkResult*)b->job.p;
    int64_t* d_totals = (int64_t*)((uint8_t*)b->job.p + 64);       // [c]: tokens of the chunks before c
    HIP_TRY(hipMemsetAsync(out_base, 0, off_tok_off, s));          // JtkResult, totals and status
    if (to_host && !small_to_host) {
        if ((rc = b->h_tok_off.ensure(((size_t)n_docs + 1) * 8)) ||
            (rc = b->h_status.ensure((size_t)(n_docs > 0 ? n_docs : 1) * 4)) ||
            (rc = b->h_tokens.ensure((size_t)n_bytes * (n_bytes <= SMALL_JOB_BYTES ? 4 : 2) / (compact ? 2 : 1) + 4096)))     // grown as the chunks report
            return rc;
    }
    uint16_t* stage_lo = nullptr; uint32_t* stage_hi = nullptr;
    if (compact && !small_to_host) {
        // the same guess (a token per two bytes; per byte for a small job) for the hi plane; the staging planes hold the
        // largest chunk at a token per byte, plus the tokens back to the range's start
        int64_t max_chunk = 0;
        for (int c = 0; c < n_chunks; c++) max_chunk = std::max(max_chunk, b->chunk_off[c + 1] - b->chunk_off[c]);
        const int64_t cap_tok = max_chunk + 64 + JTK_CP_RANGE_ALIGN;
        const size_t stage_lo_bytes = align_up((size_t)jtk_compact_lo_bytes(cap_tok), 256);
        if ((hb && (rc = b->h_hi.ensure((size_t)jtk_compact_hi_words(n_bytes <= SMALL_JOB_BYTES ? n_bytes : n_bytes / 2, hb) * 4 + 4096))) ||
            (rc = b->cp_stage.ensure(stage_lo_bytes + (size_t)jtk_compact_hi_words(cap_tok, hb) * 4 + 16)))
            return rc;
        stage_lo = (uint16_t*)b->cp_stage.p;
        stage_hi = (uint32_t*)((uint8_t*)b->cp_stage.p + stage_lo_bytes);
    }
    const bool prof = b->profiling;
    if (prof) {
        const size_t need = (size_t)n_chunks * N_STAGES * 2;
        while (b->prof_ev.size() < need) { Event ev; HIP_TRY(ev.create_timed()); b->prof_ev.push_back(std::move(ev)); }
    }
    const bool fork = n_chunks > 1 || (h_text != nullptr && !(n_chunks == 1 && n_bytes <= SMALL_JOB_BYTES));
    if (fork) {
        HIP_TRY(b->ev_fork.create());                              // (each made by the first job that needs it)
        HIP_TRY(b->ev_copy.create());
        HIP_TRY(b->copy_stream.create());
        for (int k = 0; k < n_sets; k++) {
            ChunkSet& cs = b->set[k];
            HIP_TRY(cs.stream.create());
            HIP_TRY(cs.ev_scan.create());
            HIP_TRY(cs.ev_done.create());
        }
        HIP_TRY(hipEventRecord(b->ev_fork, s));
    }
    for (ChunkSet& cs : b->set) cs.used = false;

    if ((rc = b->h_info.ensure(((size_t)n_chunks + 1) * 16))) return rc;
    // tokens of chunk c to the host: on the copy stream, after the chunk's last kernel; the host needs the chunk's token
    // range for that (written to pinned memory by its scan), so this is called one chunk behind the enqueueing
    auto send_chunk_to_host = [&](int c) -> int {
        ChunkSet& cs = b->set[c % n_sets];
        HIP_TRY(hipEventSynchronize(cs.ev_scan));
        const int64_t t0 = b->h_info.p[2 * c], t1 = b->h_info.p[2 * c + 1];
        if (t1 > t0 && compact) {
            // the range's planes: compacted into the staging planes from its start tb (a multiple of 32 tokens at or below t0:
            // the words shared with the chunk before are rewritten whole, here and in pinned memory), then the two copies
            const int64_t tb = jtk_compact_range_start(t0);
            const int64_t w0 = jtk_compact_hi_word(tb, hb), w1 = jtk_compact_hi_words(t1, hb);
            if ((size_t)t1 * 2 > b->h_tokens.cap || (size_t)w1 * 4 > b->h_hi.cap) {
                // grow: earlier chunks' copies may still be in flight into the old buffers
                HIP_TRY(hipStreamSynchronize(b->copy_stream));
                const size_t rest = ((size_t)n_bytes - (size_t)b->chunk_off[c + 1]) / 2;        // tokens still expected
                int rc2 = b->h_tokens.ensure(((size_t)t1 + rest) * 2, (size_t)t0 * 2);
                if (!rc2 && hb) rc2 = b->h_hi.ensure((size_t)jtk_compact_hi_words(t1 + (int64_t)rest, hb) * 4, (size_t)jtk_compact_hi_words(t0, hb) * 4);
                if (rc2) return rc2;
            }
            HIP_TRY(hipStreamWaitEvent(b->copy_stream, cs.ev_done, 0));
            jtk_launch_compact((const int32_t*)b->tokens.p, t0, t1, nullptr, stage_lo, stage_hi, tb, hb, b->copy_stream);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync((uint16_t*)b->h_tokens.p + t0, stage_lo + (t0 - tb), (size_t)(t1 - t0) * 2, hipMemcpyDeviceToHost, b->copy_stream));
            if (hb) HIP_TRY(hipMemcpyAsync(b->h_hi.p + w0, stage_hi, (size_t)(w1 - w0) * 4, hipMemcpyDeviceToHost, b->copy_stream));
        } else if (t1 > t0 && !(flags & JTK_ENCODE_COUNT_ONLY)) {
            if ((size_t)t1 * 4 > b->h_tokens.cap) {
                // grow: earlier chunks' copies may still be in flight into the old buffer
                HIP_TRY(hipStreamSynchronize(b->copy_stream));
                int rc2 = b->h_tokens.ensure((size_t)t1 * 4 + ((size_t)n_bytes - (size_t)b->chunk_off[c + 1]) * 2, (size_t)t0 * 4);
                if (rc2) return rc2;
            }
            HIP_TRY(hipStreamWaitEvent(b->copy_stream, cs.ev_done, 0));
            HIP_TRY(hipMemcpyAsync(b->h_tokens.p + t0, (const int32_t*)b->tokens.p + t0, (size_t)(t1 - t0) * 4, hipMemcpyDeviceToHost, b->copy_stream));
        }
        return JTK_OK;
    };

    for (int c = 0; c < n_chunks; c++) {
        ChunkSet& cs = b->set[c % n_sets];
        hipStream_t cst = fork ? cs.stream.h : s;
        const int64_t d0 = b->chunk_doc[c], d1 = b->chunk_doc[c + 1];
        const int64_t b0 = b->chunk_off[c], b1 = b->chunk_off[c + 1];
        const int64_t origin = b0 & ~(int64_t)(JTK_TILE - 1);
        // (a set is reused by chunk c + n_sets on the same stream: its scratch is free by then)
        size_t zero_bytes = 0;
        if ((rc = prepare_set(cs, b1 - origin, d1 - d0, &zero_bytes)) != JTK_OK) return rc;
        JtkWork& w = cs.work;
        w.set_info = b->h_info.p + 2 * c;
        w.text = d_text + origin;
        w.text_base = origin;
        w.lead = b0 - origin;
        w.doc_off = d_doc_off + d0;
        w.status = (int32_t*)b->status.p + d0;
        w.tokens = (int32_t*)b->tokens.p;
        w.tok_off = (int64_t*)b->tok_off.p + d0;
        w.result = d_result;
        w.job_tokens = d_totals + c;
        w.job_tokens_next = d_totals + c + 1;
        w.check_special = (!(flags & JTK_ENCODE_ORDINARY) && enc->dt.n_specials > 0) ? 1u : 0u;
        // (a table that lacks single bytes: the ids are needed to tell which documents cannot be encoded, also for a count)
        w.count_only = ((flags & JTK_ENCODE_COUNT_ONLY) && !enc->dt.pseudo_base) ? 1u : 0u;
        w.inline_scan = (!fork && n_chunks == 1 && w.n_tiles >= 1 && w.n_tiles <= 1024) ? 1u : 0u;

        if (fork && !cs.used) { HIP_TRY(hipStreamWaitEvent(cst, b->ev_fork, 0)); cs.used = true; }
        if (h_text && b1 > b0) {
            // this chunk's bytes; the bytes before b0 in the first tile were copied with the previous chunk
            HIP_TRY(hipMemcpyAsync((uint8_t*)b->in_text.p + b0, h_text + b0, (size_t)(b1 - b0), hipMemcpyHostToDevice, cst));
        }
        int stage = 0;
        const Event* pe = prof ? &b->prof_ev[(size_t)c * N_STAGES * 2] : nullptr;
        auto begin = [&]() { if (prof) (void)hipEventRecord(pe[2 * stage], cst); };
        auto end = [&]() { if (prof) (void)hipEventRecord(pe[2 * stage + 1], cst); stage++; };

        begin();                                                    // mark_docs
        HIP_TRY(hipMemsetAsync(cs.zeroed.p, 0, zero_bytes, cst));
        jtk_launch_mark_docs(w, cst);
        end();
        begin();                                                    // optional UTF-8 validation (the special-token check rides in pretok_split)
        if (flags & JTK_ENCODE_VALIDATE_UTF8) jtk_launch_validate_utf8(w, cst);
        end();
        begin();
        if (pieces) {
            const size_t mask_bytes = (size_t)w.n_words * 8;
            if ((rc = cs.gapmask.ensure(mask_bytes))) return rc;
            w.gapmask = (uint64_t*)cs.gapmask.p;
            HIP_TRY(hipMemsetAsync(cs.piecemask.p, 0, mask_bytes, cst));
            HIP_TRY(hipMemsetAsync(cs.gapmask.p, 0, mask_bytes, cst));
            const int64_t* pb = pieces->h_begin;
            const int64_t p0 = std::lower_bound(pb, pb + pieces->n, b0) - pb, p1 = std::lower_bound(pb, pb + pieces->n, b1) - pb;
            jtk_launch_mark_pieces(w, pieces->d_begin + p0, pieces->d_end + p0, p1 - p0, cst);
        } else {
            w.gapmask = nullptr;
            jtk_launch_pretok_split(w, enc->dt, cst);
        }
        end();
        begin();
        jtk_launch_piece_resolve(w, enc->dt, cst);
        end();
        begin();
        jtk_launch_long_shortcut(w, enc->dt, cst);                  // (only for rank tables with entries merging cannot reproduce)
        jtk_launch_bpe_merge(w, enc->dt, cst);
        end();
        begin();
        if (fork && c > 0) HIP_TRY(hipStreamWaitEvent(cst, b->set[(c - 1) % n_sets].ev_scan, 0));
        if (!w.inline_scan) jtk_launch_tile_scan(w, cst);
        if (fork) HIP_TRY(hipEventRecord(cs.ev_scan, cst));
        end();
        begin();
        jtk_launch_pack(w, cst);
        end();
        begin();
        jtk_launch_doc_offsets(w, cst);
        if (enc->dt.pseudo_base) jtk_launch_flag_unencodable(w, enc->dt.pseudo_base, cst);
        end();
        if (mt) jtk_launch_maxtok_decide(w, *mt, d0, cst);
        HIP_TRY(hipGetLastError());
        if (small_to_host && !zero_copy_out) {
            // the whole answer in one copy: header, status, offsets and the worst-case token range (one token per byte)
            if (compact) {
                // (the host does not know the token count yet: the pass reads it from the job's header)
                jtk_launch_compact((const int32_t*)b->tokens.p, 0, n_bytes, &d_result->n_tokens, (uint16_t*)(out_base + off_lo),
                                   (uint32_t*)(out_base + off_hi), 0, hb, cst);
                HIP_TRY(hipGetLastError());
            }
            const size_t total = ((flags & JTK_ENCODE_COUNT_ONLY) || compact) ? off_tokens : off_tokens + (size_t)n_bytes * 4;
            if ((rc = b->h_small.ensure(total + 4096))) return rc;
            HIP_TRY(hipMemcpyAsync(b->h_small.p, b->out.p, total, hipMemcpyDeviceToHost, cst));
        }
        if (fork) HIP_TRY(hipEventRecord(cs.ev_done, cst));
        if (to_host && !small_to_host && c > 0) { if ((rc = send_chunk_to_host(c - 1)) != JTK_OK) return rc; }
    }
    if (to_host && !small_to_host && n_chunks > 0) { if ((rc = send_chunk_to_host(n_chunks - 1)) != JTK_OK) return rc; }
    if (fork) {
        for (int k = 0; k < n_sets; k++)
            if (b->set[k].used) HIP_TRY(hipStreamWaitEvent(s, b->set[k].ev_done, 0));
        if (to_host && !small_to_host) {
            HIP_TRY(hipEventRecord(b->ev_copy, b->copy_stream));
            HIP_TRY(hipStreamWaitEvent(s, b->ev_copy, 0));
        }
    }
    if (small_to_host) {
        b->host_result = (JtkResult*)b->h_small.p;
        b->r_status = (int32_t*)(b->h_small.p + off_status);
        b->r_tok_off = (const int64_t*)(b->h_small.p + off_tok_off);
        b->r_tokens = compact ? nullptr : (const int32_t*)(b->h_small.p + off_tokens);
        b->r_lo = (const uint16_t*)(b->h_small.p + off_lo); b->r_hi = (const uint32_t*)(b->h_small.p + off_hi);
    } else {
        if (to_host) {
            HIP_TRY(hipMemcpyAsync(b->h_tok_off.p, b->tok_off.p, ((size_t)n_docs + 1) * 8, hipMemcpyDeviceToHost, s));
            if (n_docs > 0) HIP_TRY(hipMemcpyAsync(b->h_status.p, b->status.p, (size_t)n_docs * 4, hipMemcpyDeviceToHost, s));
        }
        b->host_result = b->host_result_own.p;
        HIP_TRY(hipMemcpyAsync(b->host_result, d_result, sizeof(JtkResult), hipMemcpyDeviceToHost, s));
        b->r_status = b->h_status.p; b->r_tok_off = b->h_tok_off.p; b->r_tokens = compact ? nullptr : b->h_tokens.p;
        b->r_lo = (const uint16_t*)b->h_tokens.p; b->r_hi = b->h_hi.p;
    }
    b->host_compact = compact_req;
    b->job_text = d_text;
    b->job_doc_off = d_doc_off;
    b->job_docs = n_docs;
    b->job_bytes = n_bytes;
    b->job_flags = flags;
    b->job_pieces = pieces != nullptr;
    b->last_stream = s;
    b->prof_chunks = prof ? n_chunks : 0;
    // (what the last encode left was dropped by the entry point, before any of the above)
    b->have_result = true; b->have_host_result = to_host;
    return JTK_OK;
}

// Chunk plan of a batch whose offsets are in device memory: a batch of up to one chunk needs none; a larger one reads the chunk
// boundaries from the offsets (the one place where this waits for the work queued on `s` before it).
int plan_device_chunks(jtk_batch* b, const int64_t* d_doc_off, int64_t n_docs, int64_t n_bytes, hipStream_t s) {
    b->chunk_doc.assign(1, 0);
    b->chunk_off.assign(1, 0);
    if (n_bytes > b->chunk_bytes + b->chunk_bytes / 4 && n_docs > 1) {
        const int nc = (int)((n_bytes + b->chunk_bytes - 1) / b->chunk_bytes);
        int rc;
        if ((rc = b->plan.ensure(((size_t)nc + 1) * 16))) return rc;
        if ((rc = b->host_plan.ensure(((size_t)nc + 1) * 16))) return rc;
        int64_t* d_doc = (int64_t*)b->plan.p;
        int64_t* d_off = d_doc + nc + 1;
        jtk_launch_plan_chunks(d_doc_off, n_docs, b->chunk_bytes, nc, d_doc, d_off, s);
        HIP_TRY(hipMemcpyAsync(b->host_plan.p, b->plan.p, ((size_t)nc + 1) * 16, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        const int64_t* h_doc = b->host_plan.p;
        const int64_t* h_off = b->host_plan.p + nc + 1;
        for (int c = 1; c < nc; c++) {
            const int64_t d = h_doc[c], o = h_off[c];
            if (d <= b->chunk_doc.back() || d >= n_docs) continue;                 // no new document since the last boundary
            if (o < b->chunk_off.back() || o > n_bytes) return fail(JTK_ERR_INVALID_ARGUMENT, "document offsets are not non-decreasing within [0, n_bytes]");
            b->chunk_doc.push_back(d);
            b->chunk_off.push_back(o);
        }
    }
    b->chunk_doc.push_back(n_docs);
    b->chunk_off.push_back(n_bytes);
    return JTK_OK;
}

// Chunk plan of a batch whose offsets are in host memory, and the check of the offsets, in one pass; cb: the chunk size.
// (A refusal leaves the plan vectors half written and the kept device plan forgotten: no result reads them, every encode
// plans anew, and a second pass over the offsets only to spare them is not worth its time on the per-call path.)
int plan_host_chunks(jtk_batch* b, const int64_t* doc_off, int64_t n_docs, int64_t n_bytes, int64_t cb) {
    b->plan_doc_off = nullptr;
    b->chunk_doc.assign(1, 0);
    b->chunk_off.assign(1, 0);
    int64_t next = cb;
    for (int64_t d = 0; d < n_docs; d++) {
        if (doc_off[d + 1] < doc_off[d]) return fail(JTK_ERR_INVALID_ARGUMENT, "doc_off must be non-decreasing");
        if (doc_off[d] >= next && d > b->chunk_doc.back() && n_bytes - doc_off[d] > cb / 4) {
            b->chunk_doc.push_back(d);
            b->chunk_off.push_back(doc_off[d]);
            next = doc_off[d] + cb;
        }
    }
    b->chunk_doc.push_back(n_docs);
    b->chunk_off.push_back(n_bytes);
    return JTK_OK;
}

bool sp_any_allowed(const jtk_batch* b) {
    for (uint8_t a : b->sp_allowed) if (a) return true;
    return false;
}

// A stitched result (allow-special's, fill-in-the-middle's: written by a stitch behind the pipeline's run on sub-documents)
// becomes the batch's: result / status / tok_off / tokens are device memory that lives with it, flags the call's.  With
// JTK_ENCODE_TO_HOST the stitch comes after the last chunk, so the ids go to the host in one copy behind it, not chunk by chunk
// (one wait, for the token count); with JTK_ENCODE_COMPACT_IDS as the planes of the whole result.
int install_stitched(jtk_batch* b, const JtkResult* result, int32_t* status, int64_t* tok_off, int32_t* tokens, const int64_t* d_doc_off,
                     int64_t n_docs, uint32_t flags, hipStream_t s) {
    const bool to_host = (flags & JTK_ENCODE_TO_HOST) != 0, count_only = (flags & JTK_ENCODE_COUNT_ONLY) != 0;
    const bool compact_req = to_host && (flags & JTK_ENCODE_COMPACT_IDS) != 0, compact = compact_req && !count_only;
    const int hb = b->enc->hb;
    int rc;
    b->job.p = (void*)result; b->status.p = status; b->tok_off.p = tok_off; b->tokens.p = tokens;
    b->host_result = b->host_result_own.p;
    HIP_TRY(hipMemcpyAsync(b->host_result, result, sizeof(JtkResult), hipMemcpyDeviceToHost, s));
    b->job_doc_off = d_doc_off;
    b->job_docs = n_docs;
    b->job_flags = flags & ~(uint32_t)(JTK_ENCODE_TO_HOST | JTK_ENCODE_COMPACT_IDS);
    if (to_host) {
        HIP_TRY(hipStreamSynchronize(s));
        const int64_t nt = b->host_result->n_tokens;
        const size_t lo_bytes = align_up((size_t)jtk_compact_lo_bytes(nt), 256), hi_bytes = (size_t)jtk_compact_hi_words(nt, hb) * 4;
        if ((rc = b->h_tok_off.ensure(((size_t)n_docs + 1) * 8)) ||
            (rc = b->h_status.ensure((size_t)(n_docs > 0 ? n_docs : 1) * 4)) ||
            (rc = b->h_tokens.ensure((size_t)nt * (compact ? 2 : 4) + 4096)))
            return rc;
        HIP_TRY(hipMemcpyAsync(b->h_tok_off.p, tok_off, ((size_t)n_docs + 1) * 8, hipMemcpyDeviceToHost, s));
        if (n_docs > 0) HIP_TRY(hipMemcpyAsync(b->h_status.p, status, (size_t)n_docs * 4, hipMemcpyDeviceToHost, s));
        if (compact) {
            // the planes of the whole stitched result, compacted behind the stitch, in one copy each
            if ((hb && (rc = b->h_hi.ensure(hi_bytes + 4096))) || (rc = b->cp_stage.ensure(lo_bytes + hi_bytes + 16))) return rc;
            uint16_t* d_lo = (uint16_t*)b->cp_stage.p;
            uint32_t* d_hi = (uint32_t*)((uint8_t*)b->cp_stage.p + lo_bytes);
            if (nt > 0) {
                jtk_launch_compact(tokens, 0, nt, nullptr, d_lo, d_hi, 0, hb, s);
                HIP_TRY(hipGetLastError());
                HIP_TRY(hipMemcpyAsync(b->h_tokens.p, d_lo, (size_t)nt * 2, hipMemcpyDeviceToHost, s));
                if (hb) HIP_TRY(hipMemcpyAsync(b->h_hi.p, d_hi, hi_bytes, hipMemcpyDeviceToHost, s));
            }
        } else if (nt > 0 && !count_only) HIP_TRY(hipMemcpyAsync(b->h_tokens.p, tokens, (size_t)nt * 4, hipMemcpyDeviceToHost, s));
        b->r_tokens = compact ? nullptr : b->h_tokens.p; b->r_tok_off = b->h_tok_off.p; b->r_status = b->h_status.p;
        b->r_lo = (const uint16_t*)b->h_tokens.p; b->r_hi = b->h_hi.p;
    }
    b->host_compact = compact_req;
    b->have_result = true; b->have_host_result = to_host;
    return JTK_OK;
}

// JTK_ENCODE_ALLOW_SPECIAL on a device-resident batch (host input is copied down whole first), jtk_special.hip: find the
// candidates; with none in any document the pipeline runs on the documents as they are (today's call: its own special-token
// check then sees only literals outside the allowed set), else on the sub-documents, and the stitch writes the result.  cb: the
// chunk size of the pipeline run.  Waits once, for the candidate count, plus the chunk plan's wait of a run longer than one
// chunk (plan_device_chunks), plus, with JTK_ENCODE_TO_HOST after a stitch, once for the token count of the copy.
int run_allow_special(jtk_batch* b, const uint8_t* d_text, const int64_t* d_doc_off, int64_t n_docs, int64_t n_bytes, uint32_t flags,
                      hipStream_t s, int64_t cb) {
    const jtk_encoding* enc = b->enc;
    const bool to_host = (flags & JTK_ENCODE_TO_HOST) != 0, count_only = (flags & JTK_ENCODE_COUNT_ONLY) != 0;
    const uint32_t base_flags = flags & ~(uint32_t)(JTK_ENCODE_ALLOW_SPECIAL | JTK_ENCODE_TO_HOST);       // (keeps JTK_ENCODE_COMPACT_IDS)
    const int n_lits = (int)enc->host.specials.size();
    int rc;
    if (b->sp_dirty) {
        const size_t n = (size_t)n_lits;
        std::vector<uint8_t> h(n * 5 + 16, 0);
        for (size_t i = 0; i < n; i++) {
            const int32_t id = enc->host.specials[i].second;
            memcpy(&h[i * 4], &id, 4);
            h[n * 4 + i] = b->sp_allowed[i];
        }
        if ((rc = b->sp_lits.ensure(h.size()))) return rc;
        HIP_TRY(hipMemcpy(b->sp_lits.p, h.data(), h.size(), hipMemcpyHostToDevice));
        b->sp_dirty = false;
    }
    JtkSpecialWork w{};
    w.text = d_text; w.doc_off = d_doc_off; w.n_docs = n_docs; w.n_bytes = n_bytes;
    w.n_lits = n_lits; w.lit_off = enc->dt.special_off; w.lit_blob = enc->dt.special_blob;
    w.lit_id = (const int32_t*)b->sp_lits.p;
    w.allowed = (const uint8_t*)b->sp_lits.p + (size_t)n_lits * 4;
    w.check_dis = (flags & JTK_ENCODE_ORDINARY) ? 0u : 1u;
    for (int i = 0; i < n_lits; i++) {
        const std::string& lit = enc->host.specials[(size_t)i].first;
        if (b->sp_allowed[(size_t)i]) w.maxlen = std::max<int64_t>(w.maxlen, (int64_t)lit.size());
        else if (!w.check_dis) continue;
        const uint8_t f = (uint8_t)lit[0];
        w.first[f >> 5] |= 1u << (f & 31);
    }
    // find scratch: hdr [4] | status [n_docs] (the result's) | per-block counts [n_blk + 1]
    w.n_blk = (n_bytes + JTK_SPECIAL_BLOCK - 1) / JTK_SPECIAL_BLOCK;
    const size_t status_bytes = align_up((size_t)(n_docs > 0 ? n_docs : 1) * 4, 16);
    if ((rc = b->sp_find.ensure(32 + status_bytes + ((size_t)w.n_blk + 1) * 8)) ||
        (rc = b->h_sp.ensure(32)))
        return rc;
    uint8_t* z = (uint8_t*)b->sp_find.p;
    w.hdr = (int64_t*)z;
    w.status = (int32_t*)(z + 32);
    w.blk = (int64_t*)(z + 32 + status_bytes);
    HIP_TRY(hipMemsetAsync(z, 0, 32 + status_bytes, s));
    jtk_launch_special_find(w, s);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(b->h_sp.p, w.hdr, 24, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    w.n_cand = b->h_sp.p[0];
    const int64_t save_cb = b->chunk_bytes;
    auto plan = [&](const int64_t* off, int64_t nd) {
        b->chunk_bytes = cb;
        const int r = plan_device_chunks(b, off, nd, n_bytes, s);
        b->chunk_bytes = save_cb;
        return r;
    };
    // a document that ends with a negative status has no tokens, which only the stitch sees to: without a candidate it still
    // runs where the find pass has refused a document, and under validation, whose offenders are known only behind the pipeline
    const bool may_refuse = (b->h_sp.p[2] != 0 || (flags & JTK_ENCODE_VALIDATE_UTF8)) && n_docs > 0 && n_bytes > 0;
    if (b->h_sp.p[1] != 0 || (w.n_cand == 0 && !may_refuse)) {
        // no allowed literal in any document (or bad offsets, which today's call reports as it always does)
        if ((rc = plan(d_doc_off, n_docs)) || (rc = run_job(b, d_text, nullptr, d_doc_off, n_docs, n_bytes, base_flags, s, to_host))) return rc;
        b->job_flags |= JTK_ENCODE_ALLOW_SPECIAL;
        return JTK_OK;
    }
    // candidates: pos, doc (i64) | len, id (i32) | keep (u8);  sub-documents: off [ns + 1], doc [ns], cnt [ns + 1] (i64),
    // doc_first [n_docs] (i64) | lit [ns] (i32)
    w.n_sub = n_docs + 2 * w.n_cand;
    const size_t nc = (size_t)w.n_cand, ns = (size_t)w.n_sub;
    const size_t o_cdoc = nc * 8, o_len = o_cdoc + nc * 8, o_id = o_len + nc * 4, o_keep = o_id + nc * 4;
    const size_t o_soff = align_up(o_keep + nc, 16), o_sdoc = o_soff + (ns + 1) * 8, o_cnt = o_sdoc + ns * 8,
                 o_first = o_cnt + (ns + 1) * 8, o_lit = o_first + (size_t)n_docs * 8, c_total = o_lit + ns * 4;
    if ((rc = b->sp_cand.ensure(c_total + 16))) return rc;
    uint8_t* c = (uint8_t*)b->sp_cand.p;
    w.cand_pos = (int64_t*)c; w.cand_doc = (int64_t*)(c + o_cdoc); w.cand_len = (int32_t*)(c + o_len);
    w.cand_id = (int32_t*)(c + o_id); w.cand_keep = c + o_keep;
    w.sub_off = (int64_t*)(c + o_soff); w.sub_doc = (int64_t*)(c + o_sdoc); w.cnt = (int64_t*)(c + o_cnt);
    w.doc_first = (int64_t*)(c + o_first); w.sub_lit = (int32_t*)(c + o_lit);
    jtk_launch_special_write(w, s);
    HIP_TRY(hipGetLastError());
    // encodeOrdinary of every sub-document (the literals' tokens are not used: their ids are written instead)
    const uint32_t sub_flags = JTK_ENCODE_ORDINARY | (flags & (JTK_ENCODE_VALIDATE_UTF8 | JTK_ENCODE_COUNT_ONLY));
    if ((rc = plan(w.sub_off, w.n_sub)) || (rc = run_job(b, d_text, nullptr, w.sub_off, w.n_sub, n_bytes, sub_flags, s, false))) return rc;
    drop_encode_result(b);           // (the sub-documents' result is not the batch's: the stitched one is, once it is whole)
    // the stitched result: JtkResult | tok_off [n_docs + 1] | tokens (status: in the find scratch)
    const size_t o_tok_off = 64, o_tokens = align_up(o_tok_off + ((size_t)n_docs + 1) * 8, 256);
    if ((rc = b->sp_out.ensure(o_tokens + (count_only ? 0 : ((size_t)n_bytes + 64) * 4)))) return rc;
    uint8_t* out = (uint8_t*)b->sp_out.p;
    w.sub_tok_off = (const int64_t*)b->tok_off.p; w.sub_status = (const int32_t*)b->status.p; w.sub_tokens = (const int32_t*)b->tokens.p;
    w.result = (JtkResult*)out; w.tok_off = (int64_t*)(out + o_tok_off); w.tokens = (int32_t*)(out + o_tokens);
    w.count_only = count_only ? 1u : 0u;
    HIP_TRY(hipMemsetAsync(out, 0, sizeof(JtkResult), s));
    jtk_launch_special_stitch(w, s);
    HIP_TRY(hipGetLastError());
    return install_stitched(b, w.result, w.status, w.tok_off, w.tokens, d_doc_off, n_docs, flags, s);
}

// JTK_ENCODE_FIM on a device-resident batch (host input is copied down whole first), jtk_fim.hip: kind, cuts and the three
// sub-documents of every document, the pipeline on the sub-documents, the stitch.  cb: the chunk size of the pipeline run.  No
// wait of its own: the chunk plan's of a run longer than one chunk, and install_stitched's for a host copy.
int run_fim(jtk_batch* b, const uint8_t* d_text, const int64_t* d_doc_off, int64_t n_docs, int64_t n_bytes, uint32_t flags, hipStream_t s,
            int64_t cb) {
    const bool count_only = (flags & JTK_ENCODE_COUNT_ONLY) != 0;
    int rc;
    // hdr [4] | status [n] | sub_off [3n + 1] | cut [2n] | part_tok [3n] | kind [n];  the stitched result: JtkResult | tok_off
    // [n + 1] | tokens (at most a token per byte and three sentinels per document)
    const size_t n = (size_t)n_docs, status_bytes = align_up((n > 0 ? n : 1) * 4, 16);
    const size_t o_sub = 32 + status_bytes, o_cut = o_sub + (3 * n + 1) * 8, o_part = o_cut + 2 * n * 8, o_kind = o_part + 3 * n * 8;
    const size_t o_tok_off = 64, o_tokens = align_up(o_tok_off + (n + 1) * 8, 256);
    if ((rc = b->fim_buf.ensure(o_kind + n + 16)) ||
        (rc = b->sp_out.ensure(o_tokens + (count_only ? 0 : ((size_t)n_bytes + 3 * n + 64) * 4))))
        return rc;
    uint8_t* z = (uint8_t*)b->fim_buf.p;
    uint8_t* out = (uint8_t*)b->sp_out.p;
    JtkFimWork w{};
    w.text = d_text; w.doc_off = d_doc_off; w.n_docs = n_docs; w.n_bytes = n_bytes;
    w.seed = b->fim.seed; w.doc_index_base = b->fim.doc_index_base; w.fim_rate = b->fim.fim_rate; w.spm_rate = b->fim.spm_rate;
    w.hdr = (int64_t*)z; w.status = (int32_t*)(z + 32); w.sub_off = (int64_t*)(z + o_sub); w.cut = (int64_t*)(z + o_cut);
    w.part_tok = (int64_t*)(z + o_part); w.kind = z + o_kind;
    w.result = (JtkResult*)out; w.tok_off = (int64_t*)(out + o_tok_off); w.tokens = (int32_t*)(out + o_tokens);
    w.count_only = count_only ? 1u : 0u;
    HIP_TRY(hipMemsetAsync(z, 0, 32, s));
    HIP_TRY(hipMemsetAsync(out, 0, sizeof(JtkResult), s));
    jtk_launch_fim_cuts(w, s);
    HIP_TRY(hipGetLastError());
    // encodeOrdinary of every sub-document
    const uint32_t sub_flags = JTK_ENCODE_ORDINARY | (flags & (JTK_ENCODE_VALIDATE_UTF8 | JTK_ENCODE_COUNT_ONLY));
    const int64_t save_cb = b->chunk_bytes;
    b->chunk_bytes = cb;
    rc = plan_device_chunks(b, w.sub_off, 3 * n_docs, n_bytes, s);
    b->chunk_bytes = save_cb;
    if (rc || (rc = run_job(b, d_text, nullptr, w.sub_off, 3 * n_docs, n_bytes, sub_flags, s, false))) return rc;
    drop_encode_result(b);           // (the sub-documents' result is not the batch's: the stitched one is, once it is whole)
    w.sub_tok_off = (const int64_t*)b->tok_off.p; w.sub_status = (const int32_t*)b->status.p;
    w.v.n_docs = n_docs; w.v.kind = w.kind; w.v.part_tok = w.part_tok; w.v.tok_off = w.tok_off;
    w.v.sub_tok_off = w.sub_tok_off; w.v.sub_tokens = (const int32_t*)b->tokens.p;
    w.v.prefix_id = b->fim.prefix_id; w.v.middle_id = b->fim.middle_id; w.v.suffix_id = b->fim.suffix_id;
    jtk_launch_fim_stitch(w, s);
    HIP_TRY(hipGetLastError());
    if ((rc = install_stitched(b, w.result, w.status, w.tok_off, w.tokens, d_doc_off, n_docs, flags, s))) return rc;
    b->fim_kind = w.kind; b->fim_cut = w.cut; b->fim_part_tok = w.part_tok;
    b->have_fim = true;
    return JTK_OK;
}

// what JTK_ENCODE_FIM needs at the two entry points that take it
int fim_flags(const jtk_batch* b, uint32_t flags) {
    if (!(flags & JTK_ENCODE_FIM)) return JTK_OK;
    if (!b->fim_set) return fail(JTK_ERR_INVALID_ARGUMENT, "JTK_ENCODE_FIM without parameters: jtk_batch_set_fim has not set any on this batch");
    if (!(flags & JTK_ENCODE_ORDINARY))
        return fail(JTK_ERR_INVALID_ARGUMENT, "JTK_ENCODE_FIM needs JTK_ENCODE_ORDINARY: encode()'s special-token check would have to look across the cuts");
    if (flags & JTK_ENCODE_ALLOW_SPECIAL) return fail(JTK_ERR_INVALID_ARGUMENT, "JTK_ENCODE_FIM does not combine with JTK_ENCODE_ALLOW_SPECIAL");
    return JTK_OK;
}
const char* const FIM_ELSEWHERE = "JTK_ENCODE_FIM is for jtk_batch_encode / jtk_batch_encode_device";

}  // namespace

extern "C" {

int jtk_batch_encode_device(jtk_batch* b, const uint8_t* d_utf8, const int64_t* d_doc_off, int64_t n_docs,
                            int64_t n_bytes, uint32_t flags, void* stream_or_null, int64_t* n_tokens) {
    if (!b || n_docs < 0 || n_bytes < 0 || (n_bytes > 0 && !d_utf8) || !d_doc_off)
        return fail(JTK_ERR_INVALID_ARGUMENT, "bad arguments");
    if (((uintptr_t)d_utf8 & 15u) != 0) return fail(JTK_ERR_INVALID_ARGUMENT, "device text must be 16-byte aligned");
    if (n_bytes >= (int64_t)1 << 37) return fail(JTK_ERR_INVALID_ARGUMENT, "batch too large (128 GiB of text per call at most)");
    if (flags & JTK_ENCODE_TO_HOST) return fail(JTK_ERR_INVALID_ARGUMENT, "JTK_ENCODE_TO_HOST is for jtk_batch_encode (host buffers)");
    if (flags & JTK_ENCODE_COMPACT_IDS) return fail(JTK_ERR_INVALID_ARGUMENT, "JTK_ENCODE_COMPACT_IDS is for jtk_batch_encode with JTK_ENCODE_TO_HOST (on the device: jtk_batch_compact)");
    int rc;
    if ((rc = fim_flags(b, flags))) return rc;
    HIP_TRY(hipSetDevice(b->enc->device));
    drop_encode_result(b);
    hipStream_t s = pick_stream(b, stream_or_null);
    if ((flags & JTK_ENCODE_ALLOW_SPECIAL) && !sp_any_allowed(b)) flags &= ~(uint32_t)JTK_ENCODE_ALLOW_SPECIAL;   // empty set: today's call
    if (flags & JTK_ENCODE_FIM) {
        b->plan_doc_off = nullptr;                                  // (no JTK_OPT_REUSE_CHUNK_PLAN here)
        rc = run_fim(b, d_utf8, d_doc_off, n_docs, n_bytes, flags, s, b->chunk_bytes);
    } else if (flags & JTK_ENCODE_ALLOW_SPECIAL) {
        b->plan_doc_off = nullptr;                                  // (no JTK_OPT_REUSE_CHUNK_PLAN here)
        rc = run_allow_special(b, d_utf8, d_doc_off, n_docs, n_bytes, flags, s, b->chunk_bytes);
    } else {
        // chunk plan: a batch of up to one chunk needs none; a larger one reads the chunk boundaries from the offsets (the one
        // place where this call waits for the work queued on `s` before it)
        const bool same_plan = b->reuse_plan && b->plan_doc_off == d_doc_off && b->plan_docs == n_docs && b->plan_bytes == n_bytes && b->plan_chunk_bytes == b->chunk_bytes &&
                               b->chunk_doc.size() >= 2 && b->chunk_doc.back() == n_docs && b->chunk_off.back() == n_bytes;
        if (!same_plan) {
            if ((rc = plan_device_chunks(b, d_doc_off, n_docs, n_bytes, s))) return rc;
            b->plan_doc_off = d_doc_off; b->plan_docs = n_docs; b->plan_bytes = n_bytes; b->plan_chunk_bytes = b->chunk_bytes;
        }
        if ((rc = run_job(b, d_utf8, nullptr, d_doc_off, n_docs, n_bytes, flags, s, false))) b->plan_doc_off = nullptr;
    }
    if (rc != JTK_OK) return rc;
    if (n_tokens) {
        HIP_TRY(hipStreamSynchronize(s));
        b->synced = true;
        *n_tokens = b->host_result->n_tokens;
    }
    return JTK_OK;
}

int jtk_batch_encode(jtk_batch* b, const uint8_t* utf8, const int64_t* doc_off, int64_t n_docs,
                     uint32_t flags, int64_t* n_tokens) {
    if (!b || n_docs < 0 || !doc_off) return fail(JTK_ERR_INVALID_ARGUMENT, "bad arguments");
    if ((flags & JTK_ENCODE_COMPACT_IDS) && !(flags & JTK_ENCODE_TO_HOST))
        return fail(JTK_ERR_INVALID_ARGUMENT, "JTK_ENCODE_COMPACT_IDS needs JTK_ENCODE_TO_HOST (on the device: jtk_batch_compact)");
    if (doc_off[0] != 0) return fail(JTK_ERR_INVALID_ARGUMENT, "doc_off[0] must be 0");
    const int64_t n_bytes = doc_off[n_docs];
    if (n_bytes > 0 && !utf8) return fail(JTK_ERR_INVALID_ARGUMENT, "utf8 is NULL");
    if (n_bytes >= (int64_t)1 << 37) return fail(JTK_ERR_INVALID_ARGUMENT, "batch too large (128 GiB of text per call at most)");
    const int64_t cb = b->host_chunk_bytes < b->chunk_bytes ? b->host_chunk_bytes : b->chunk_bytes;
    int rc;
    if ((rc = fim_flags(b, flags)) || (rc = plan_host_chunks(b, doc_off, n_docs, n_bytes, cb))) return rc;
    HIP_TRY(hipSetDevice(b->enc->device));
    drop_encode_result(b);
    if ((flags & JTK_ENCODE_ALLOW_SPECIAL) && !sp_any_allowed(b)) flags &= ~(uint32_t)JTK_ENCODE_ALLOW_SPECIAL;   // empty set: today's call
    if (flags & (JTK_ENCODE_ALLOW_SPECIAL | JTK_ENCODE_FIM)) {
        // the text goes down whole (the candidates are found, the cuts are made, before any chunk is encoded); then as device input
        if ((rc = b->in_text.ensure((size_t)n_bytes + 64)) || (rc = b->in_off.ensure(((size_t)n_docs + 1) * 8))) return rc;
        HIP_TRY(hipMemcpyAsync(b->in_off.p, doc_off, ((size_t)n_docs + 1) * 8, hipMemcpyHostToDevice, b->stream));
        if (n_bytes > 0) HIP_TRY(hipMemcpyAsync(b->in_text.p, utf8, (size_t)n_bytes, hipMemcpyHostToDevice, b->stream));
        rc = (flags & JTK_ENCODE_FIM) ? run_fim(b, (const uint8_t*)b->in_text.p, (const int64_t*)b->in_off.p, n_docs, n_bytes, flags, b->stream, cb)
                                      : run_allow_special(b, (const uint8_t*)b->in_text.p, (const int64_t*)b->in_off.p, n_docs, n_bytes, flags, b->stream, cb);
    } else if (b->chunk_doc.size() == 2 && n_bytes <= TINY_JOB_BYTES) {
        // a per-call device batch: offsets and text go down in ONE copy (staged side by side in pinned memory; copying a few KB on
        // the host costs less than a second DMA)
        const size_t off_text = align_up(((size_t)n_docs + 1) * 8, 256), total = off_text + (size_t)n_bytes;
        if ((rc = b->h_in.ensure(total + 64)) || (rc = b->in_text.ensure(total + 64))) return rc;
        memcpy(b->h_in.p, doc_off, ((size_t)n_docs + 1) * 8);
        if (n_bytes > 0) memcpy(b->h_in.p + off_text, utf8, (size_t)n_bytes);
        // (the other way round -- the kernels reading text and offsets from the pinned block over the link -- was 5 us slower:
        // four kernels read the text)
        HIP_TRY(hipMemcpyAsync(b->in_text.p, b->h_in.p, total, hipMemcpyHostToDevice, b->stream));
        rc = run_job(b, (const uint8_t*)b->in_text.p + off_text, nullptr, (const int64_t*)b->in_text.p, n_docs, n_bytes,
                     flags & ~(uint32_t)JTK_ENCODE_TO_HOST, b->stream, (flags & JTK_ENCODE_TO_HOST) != 0);
    } else {
        if ((rc = b->in_text.ensure((size_t)n_bytes + 64)) || (rc = b->in_off.ensure(((size_t)n_docs + 1) * 8))) return rc;
        HIP_TRY(hipMemcpyAsync(b->in_off.p, doc_off, ((size_t)n_docs + 1) * 8, hipMemcpyHostToDevice, b->stream));
        rc = run_job(b, (const uint8_t*)b->in_text.p, utf8, (const int64_t*)b->in_off.p, n_docs, n_bytes, flags & ~(uint32_t)JTK_ENCODE_TO_HOST,
                     b->stream, (flags & JTK_ENCODE_TO_HOST) != 0);
    }
    if (rc != JTK_OK) return rc;
    HIP_TRY(hipStreamSynchronize(b->stream));
    b->synced = true;
    if (n_tokens) *n_tokens = b->host_result->n_tokens;
    return JTK_OK;
}

int jtk_batch_encode_pieces(jtk_batch* b, const uint8_t* utf8, const int64_t* doc_off, int64_t n_docs,
                            const int64_t* piece_begin, const int64_t* piece_end, int64_t n_pieces, uint32_t flags, int64_t* n_tokens) {
    if (!b || n_docs < 0 || !doc_off || n_pieces < 0 || (n_pieces > 0 && (!piece_begin || !piece_end)))
        return fail(JTK_ERR_INVALID_ARGUMENT, "bad arguments");
    if (flags & JTK_ENCODE_ALLOW_SPECIAL) return fail(JTK_ERR_INVALID_ARGUMENT, "JTK_ENCODE_ALLOW_SPECIAL is for jtk_batch_encode / jtk_batch_encode_device");
    if (flags & JTK_ENCODE_FIM) return fail(JTK_ERR_INVALID_ARGUMENT, FIM_ELSEWHERE);
    if ((flags & JTK_ENCODE_COMPACT_IDS) && !(flags & JTK_ENCODE_TO_HOST))
        return fail(JTK_ERR_INVALID_ARGUMENT, "JTK_ENCODE_COMPACT_IDS needs JTK_ENCODE_TO_HOST (on the device: jtk_batch_compact)");
    if (doc_off[0] != 0) return fail(JTK_ERR_INVALID_ARGUMENT, "doc_off[0] must be 0");
    const int64_t n_bytes = doc_off[n_docs];
    if (n_bytes > 0 && !utf8) return fail(JTK_ERR_INVALID_ARGUMENT, "utf8 is NULL");
    if (n_bytes >= (int64_t)1 << 37) return fail(JTK_ERR_INVALID_ARGUMENT, "batch too large (128 GiB of text per call at most)");
    // pieces: ascending, non-empty, non-overlapping, each inside one document
    {
        int64_t d = 0, prev_end = 0;
        for (int64_t i = 0; i < n_pieces; i++) {
            const int64_t p = piece_begin[i], e = piece_end[i];
            if (p < prev_end || e <= p || e > n_bytes) return fail(JTK_ERR_INVALID_ARGUMENT, "pieces must be ascending, non-empty and non-overlapping");
            while (d < n_docs && doc_off[d + 1] <= p) d++;
            if (d >= n_docs || e > doc_off[d + 1]) return fail(JTK_ERR_INVALID_ARGUMENT, "a piece crosses a document boundary");
            prev_end = e;
        }
    }
    int rc;
    if ((rc = plan_host_chunks(b, doc_off, n_docs, n_bytes, b->host_chunk_bytes < b->chunk_bytes ? b->host_chunk_bytes : b->chunk_bytes))) return rc;
    HIP_TRY(hipSetDevice(b->enc->device));
    drop_encode_result(b);
    if ((rc = b->in_text.ensure((size_t)n_bytes + 64)) || (rc = b->in_off.ensure(((size_t)n_docs + 1) * 8)) ||
        (rc = b->in_pieces.ensure((size_t)(n_pieces > 0 ? n_pieces : 1) * 16)))
        return rc;
    HIP_TRY(hipMemcpyAsync(b->in_off.p, doc_off, ((size_t)n_docs + 1) * 8, hipMemcpyHostToDevice, b->stream));
    int64_t* d_begin = (int64_t*)b->in_pieces.p;
    int64_t* d_end = d_begin + (n_pieces > 0 ? n_pieces : 1);
    if (n_pieces > 0) {
        HIP_TRY(hipMemcpyAsync(d_begin, piece_begin, (size_t)n_pieces * 8, hipMemcpyHostToDevice, b->stream));
        HIP_TRY(hipMemcpyAsync(d_end, piece_end, (size_t)n_pieces * 8, hipMemcpyHostToDevice, b->stream));
    }
    const PieceArgs pa{d_begin, d_end, piece_begin, n_pieces};
    // the special-token check of encode() (GptBytePairEncoding.java:52-56, text.contains) rides in pretok_split on the device;
    // with caller-supplied pieces that kernel does not run, so it is done here on the host
    std::vector<int64_t> special_docs;
    if (!(flags & JTK_ENCODE_ORDINARY)) {
        std::vector<uint8_t> flag;
        find_special_docs(b->enc, utf8, n_bytes, doc_off, n_docs, flag);
        for (int64_t d = 0; d < n_docs; d++) if (flag[(size_t)d]) special_docs.push_back(d);
    }
    rc = run_job(b, (const uint8_t*)b->in_text.p, utf8, (const int64_t*)b->in_off.p, n_docs, n_bytes,
                 (flags | JTK_ENCODE_ORDINARY) & ~(uint32_t)JTK_ENCODE_TO_HOST, b->stream, (flags & JTK_ENCODE_TO_HOST) != 0, &pa);
    if (rc != JTK_OK) return rc;
    HIP_TRY(hipStreamSynchronize(b->stream));
    if (!special_docs.empty()) {
        const int32_t st = JTK_ERR_UNSUPPORTED_SPECIAL;
        for (int64_t d : special_docs) {
            HIP_TRY(hipMemcpy((int32_t*)b->status.p + d, &st, 4, hipMemcpyDefault));
            if (b->have_host_result) b->r_status[d] = st;
        }
        if (b->host_result->worst_status > st) b->host_result->worst_status = st;
    }
    b->synced = true;
    if (n_tokens) *n_tokens = b->host_result->n_tokens;
    return JTK_OK;
}

void* jtk_batch_stream(jtk_batch* b) { return b ? (void*)b->stream.h : nullptr; }

int jtk_batch_result(jtk_batch* b, int64_t* n_tokens, int64_t* n_docs, int32_t* worst_status) {
    if (!b || !b->have_result) return fail(JTK_ERR_INVALID_ARGUMENT, "no encode has run on this batch");
    HIP_TRY(hipSetDevice(b->enc->device));
    if (int rc = sync_last(b)) return rc;
    if (n_tokens) *n_tokens = b->host_result->n_tokens;
    if (n_docs) *n_docs = b->job_docs;
    if (worst_status) *worst_status = b->host_result->worst_status;
    return JTK_OK;
}

int jtk_batch_fetch(jtk_batch* b, int32_t* tokens, int64_t tokens_cap, int64_t* tok_off, int32_t* status) {
    int64_t nt = 0;
    int rc = jtk_batch_result(b, &nt, nullptr, nullptr);
    if (rc != JTK_OK) return rc;
    const bool count_only = (b->job_flags & JTK_ENCODE_COUNT_ONLY) != 0;
    if (tokens) {
        if (count_only) return fail(JTK_ERR_INVALID_ARGUMENT, "the last encode was count-only: there are no token ids");
        if (tokens_cap < nt) return fail(JTK_ERR_CAPACITY, "tokens buffer too small");
        if (nt > 0) {
            if (b->have_host_result && !b->host_compact) memcpy(tokens, b->r_tokens, (size_t)nt * 4);
            else HIP_TRY(hipMemcpy(tokens, b->tokens.p, (size_t)nt * 4, hipMemcpyDefault));
        }
    }
    if (tok_off) HIP_TRY(hipMemcpy(tok_off, b->tok_off.p, ((size_t)b->job_docs + 1) * 8, hipMemcpyDefault));
    if (status && b->job_docs > 0)
        HIP_TRY(hipMemcpy(status, b->status.p, (size_t)b->job_docs * 4, hipMemcpyDefault));
    return JTK_OK;
}

int jtk_batch_host_result(jtk_batch* b, const int32_t** tokens, const int64_t** tok_off, const int32_t** status) {
    if (!b || !b->have_result || !b->have_host_result)
        return fail(JTK_ERR_INVALID_ARGUMENT, "the last encode on this batch did not run with JTK_ENCODE_TO_HOST");
    if (b->host_compact)
        return fail(JTK_ERR_INVALID_ARGUMENT, "the last encode ran with JTK_ENCODE_COMPACT_IDS: host memory holds no int32 ids, read the planes with jtk_batch_host_result_compact()");
    HIP_TRY(hipSetDevice(b->enc->device));
    if (int rc = sync_last(b)) return rc;
    if (tokens) *tokens = (b->job_flags & JTK_ENCODE_COUNT_ONLY) ? nullptr : b->r_tokens;
    if (tok_off) *tok_off = b->r_tok_off;
    if (status) *status = b->r_status;
    return JTK_OK;
}

int jtk_batch_host_result_compact(jtk_batch* b, const uint16_t** lo, const uint32_t** hi, int* id_bits, const int64_t** tok_off,
                                  const int32_t** status) {
    if (!b || !b->have_result || !b->have_host_result || !b->host_compact)
        return fail(JTK_ERR_INVALID_ARGUMENT, "the last encode on this batch did not run with JTK_ENCODE_TO_HOST | JTK_ENCODE_COMPACT_IDS");
    HIP_TRY(hipSetDevice(b->enc->device));
    if (int rc = sync_last(b)) return rc;
    const bool count_only = (b->job_flags & JTK_ENCODE_COUNT_ONLY) != 0;
    if (lo) *lo = count_only ? nullptr : b->r_lo;
    if (hi) *hi = (count_only || !b->enc->hb) ? nullptr : b->r_hi;
    if (id_bits) *id_bits = 16 + b->enc->hb;
    if (tok_off) *tok_off = b->r_tok_off;
    if (status) *status = b->r_status;
    return JTK_OK;
}

int jtk_widen_ids(const uint16_t* lo, const uint32_t* hi, int id_bits, int64_t first, int64_t n, int32_t* out) {
    if (!jtk_compact_valid_bits(id_bits)) return fail(JTK_ERR_INVALID_ARGUMENT, "id_bits must be 16, 17, 18, 20, 24 or 32");
    const int hb = id_bits - 16;
    if (first < 0 || n < 0 || (n > 0 && (!lo || !out || (hb && !hi)))) return fail(JTK_ERR_INVALID_ARGUMENT, "bad arguments");
    if (!hb) for (int64_t k = 0; k < n; k++) out[k] = lo[first + k];
    else for (int64_t k = 0; k < n; k++) out[k] = jtk_compact_widen(lo, hi, hb, first + k);
    return JTK_OK;
}

int jtk_batch_device_result(jtk_batch* b, const int32_t** d_tokens, const int64_t** d_tok_off,
                            const int32_t** d_status) {
    if (!b || !b->have_result) return fail(JTK_ERR_INVALID_ARGUMENT, "no encode has run on this batch");
    if (d_tokens) *d_tokens = (b->job_flags & JTK_ENCODE_COUNT_ONLY) ? nullptr : (const int32_t*)b->tokens.p;
    if (d_tok_off) *d_tok_off = (const int64_t*)b->tok_off.p;
    if (d_status) *d_status = (const int32_t*)b->status.p;
    return JTK_OK;
}

int jtk_batch_kernel_times(jtk_batch* b, const char** names, float* ms, int cap, int* n) {
    if (!b || !n) return fail(JTK_ERR_INVALID_ARGUMENT, "bad arguments");
    *n = 0;
    if (b->prof_chunks <= 0) return fail(JTK_ERR_INVALID_ARGUMENT, "profiling was not enabled for the last encode");
    HIP_TRY(hipSetDevice(b->enc->device));
    HIP_TRY(hipStreamSynchronize(b->last_stream));
    for (int i = 0; i < N_STAGES && i < cap; i++) {
        float sum = 0.f;
        for (int c = 0; c < b->prof_chunks; c++) {
            float t = 0.f;
            HIP_TRY(hipEventElapsedTime(&t, b->prof_ev[((size_t)c * N_STAGES + i) * 2], b->prof_ev[((size_t)c * N_STAGES + i) * 2 + 1]));
            sum += t;
        }
        if (names) names[i] = STAGE_NAMES[i];
        if (ms) ms[i] = sum;
        *n = i + 1;
    }
    return JTK_OK;
}

// ---- maxTokens on the device ---------------------------------------------------------------------------
int jtk_batch_truncate(jtk_batch* b, int64_t max_tokens) {
    if (!b || !b->have_result || max_tokens < 0) return fail(JTK_ERR_INVALID_ARGUMENT, "bad arguments (an encode must have run on this batch)");
    if (b->job_flags & JTK_ENCODE_ALLOW_SPECIAL) return fail(JTK_ERR_INVALID_ARGUMENT, "maxTokens is not defined after a JTK_ENCODE_ALLOW_SPECIAL encode");
    if (b->job_flags & JTK_ENCODE_FIM) return fail(JTK_ERR_INVALID_ARGUMENT, "maxTokens is not defined after a JTK_ENCODE_FIM encode");
    HIP_TRY(hipSetDevice(b->enc->device));
    if (int rc = sync_last(b)) return rc;
    const int64_t nd = b->job_docs;
    int rc;
    if ((rc = b->trunc_kept.ensure((size_t)(nd > 0 ? nd : 1) * 8)) || (rc = b->trunc_flag.ensure((size_t)(nd > 0 ? nd : 1)))) return rc;
    JtkTruncWork t{};
    t.tokens = (const int32_t*)b->tokens.p; t.tok_off = (const int64_t*)b->tok_off.p; t.text = b->job_text; t.doc_off = b->job_doc_off;
    t.n_docs = nd; t.tab_off = (const uint32_t*)b->enc->dec_off.p; t.max_tokens = max_tokens;
    t.kept = (int64_t*)b->trunc_kept.p; t.truncated = (uint8_t*)b->trunc_flag.p;
    jtk_launch_truncate(t, b->last_stream);
    HIP_TRY(hipGetLastError());
    b->have_trunc = true;
    return JTK_OK;
}

int jtk_batch_fetch_truncated(jtk_batch* b, int64_t* kept, uint8_t* truncated) {
    if (!b || !b->have_trunc) return fail(JTK_ERR_INVALID_ARGUMENT, "jtk_batch_truncate has not run on this batch");
    HIP_TRY(hipSetDevice(b->enc->device));
    HIP_TRY(hipStreamSynchronize(b->last_stream));
    const size_t nd = (size_t)b->job_docs;
    if (kept && nd) HIP_TRY(hipMemcpy(kept, b->trunc_kept.p, nd * 8, hipMemcpyDeviceToHost));
    if (truncated && nd) HIP_TRY(hipMemcpy(truncated, b->trunc_flag.p, nd, hipMemcpyDeviceToHost));
    return JTK_OK;
}

int jtk_batch_device_truncated(jtk_batch* b, const int64_t** d_kept, const uint8_t** d_truncated) {
    if (!b || !b->have_trunc) return fail(JTK_ERR_INVALID_ARGUMENT, "jtk_batch_truncate has not run on this batch");
    if (d_kept) *d_kept = (const int64_t*)b->trunc_kept.p;
    if (d_truncated) *d_truncated = (const uint8_t*)b->trunc_flag.p;
    return JTK_OK;
}

// ---- batch decode ------------------------------------------------------------------------------------
int jtk_batch_decode_device(jtk_batch* b, const int32_t* d_ids, const int64_t* d_seq_off, int64_t n_seqs, int64_t n_ids,
                            void* stream_or_null, int64_t* n_bytes) {
    if (!b || n_seqs < 0 || n_ids < 0 || (n_ids > 0 && !d_ids) || !d_seq_off) return fail(JTK_ERR_INVALID_ARGUMENT, "bad arguments");
    const jtk_encoding* enc = b->enc;
    HIP_TRY(hipSetDevice(enc->device));
    drop_decode_result(b);
    hipStream_t s = pick_stream(b, stream_or_null);
    JtkDecodeWork& w = b->dwork;
    w.ids = d_ids; w.seq_off = d_seq_off; w.n_tok = n_ids; w.n_seqs = n_seqs;
    w.n_tiles = (n_ids + JTK_DEC_TILE - 1) / JTK_DEC_TILE;
    if (w.n_tiles < 1) w.n_tiles = 1;
    w.tab_off = (const uint32_t*)enc->dec_off.p; w.tab_blob = (const uint8_t*)enc->dec_blob.p; w.n_ids_table = enc->n_ids_table;
    const size_t nt = (size_t)w.n_tiles;
    const size_t mask_bytes = (nt * (JTK_DEC_TILE / 64) + 2) * 8;
    const size_t status_bytes = align_up((size_t)(n_seqs > 0 ? n_seqs : 1) * 4, 16);
    const size_t zero_bytes = mask_bytes + status_bytes + 16;
    int rc;
    if ((rc = b->dec_zero.ensure(zero_bytes)) || (rc = b->dec_tile.ensure(nt * 4 + (nt + 1) * 8 + 16)) ||
        (rc = b->dec_pre.ensure(nt * JTK_DEC_TILE * 4)) || (rc = b->dec_byte_off.ensure(((size_t)n_seqs + 1) * 8)))
        return rc;
    uint8_t* z = (uint8_t*)b->dec_zero.p;
    w.seqmask = (uint64_t*)z;
    w.status = (int32_t*)(z + mask_bytes);
    w.total = (int64_t*)(z + mask_bytes + status_bytes);
    w.worst_status = (int32_t*)(z + mask_bytes + status_bytes + 8);
    w.tile_off = (int64_t*)b->dec_tile.p;
    w.tile_bytes = (uint32_t*)((uint8_t*)b->dec_tile.p + (nt + 1) * 8);
    w.seqpre = (uint32_t*)b->dec_pre.p;
    w.byte_off = (int64_t*)b->dec_byte_off.p;
    w.out = nullptr;
    // phase 1: sizes (the output is allocated once they are known)
    HIP_TRY(hipMemsetAsync(z, 0, zero_bytes, s));
    jtk_launch_decode_count(w, s);
    int64_t total = 0;
    HIP_TRY(hipMemcpyAsync(&total, w.total, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if ((rc = b->dec_out.ensure((size_t)total + 64))) return rc;
    w.out = (uint8_t*)b->dec_out.p;
    // phase 2: bytes and per-sequence offsets
    jtk_launch_decode_scatter(w, s);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s));
    b->dec_total = total;
    b->have_decode = true;
    if (n_bytes) *n_bytes = total;
    return JTK_OK;
}

int jtk_batch_decode(jtk_batch* b, const int32_t* ids, const int64_t* seq_off, int64_t n_seqs, int64_t* n_bytes) {
    if (!b || n_seqs < 0 || !seq_off) return fail(JTK_ERR_INVALID_ARGUMENT, "bad arguments");
    if (seq_off[0] != 0) return fail(JTK_ERR_INVALID_ARGUMENT, "seq_off[0] must be 0");
    for (int64_t q = 0; q < n_seqs; q++)
        if (seq_off[q + 1] < seq_off[q]) return fail(JTK_ERR_INVALID_ARGUMENT, "seq_off must be non-decreasing");
    const int64_t n_ids = seq_off[n_seqs];
    if (n_ids > 0 && !ids) return fail(JTK_ERR_INVALID_ARGUMENT, "ids is NULL");
    HIP_TRY(hipSetDevice(b->enc->device));
    drop_decode_result(b);
    int rc;
    if ((rc = b->dec_in_ids.ensure((size_t)n_ids * 4 + 64)) || (rc = b->dec_in_off.ensure(((size_t)n_seqs + 1) * 8))) return rc;
    if (n_ids > 0) HIP_TRY(hipMemcpyAsync(b->dec_in_ids.p, ids, (size_t)n_ids * 4, hipMemcpyHostToDevice, b->stream));
    HIP_TRY(hipMemcpyAsync(b->dec_in_off.p, seq_off, ((size_t)n_seqs + 1) * 8, hipMemcpyHostToDevice, b->stream));
    return jtk_batch_decode_device(b, (const int32_t*)b->dec_in_ids.p, (const int64_t*)b->dec_in_off.p, n_seqs, n_ids, nullptr, n_bytes);
}

int jtk_batch_decode_fetch(jtk_batch* b, uint8_t* out, int64_t out_cap, int64_t* byte_off, int32_t* status) {
    if (!b || !b->have_decode) return fail(JTK_ERR_INVALID_ARGUMENT, "no decode has run on this batch");
    HIP_TRY(hipSetDevice(b->enc->device));
    if (out) {
        if (out_cap < b->dec_total) return fail(JTK_ERR_CAPACITY, "output buffer too small");
        if (b->dec_total > 0) HIP_TRY(hipMemcpy(out, b->dwork.out, (size_t)b->dec_total, hipMemcpyDeviceToHost));
    }
    if (byte_off) HIP_TRY(hipMemcpy(byte_off, b->dwork.byte_off, ((size_t)b->dwork.n_seqs + 1) * 8, hipMemcpyDeviceToHost));
    if (status && b->dwork.n_seqs > 0) HIP_TRY(hipMemcpy(status, b->dwork.status, (size_t)b->dwork.n_seqs * 4, hipMemcpyDeviceToHost));
    return JTK_OK;
}

int jtk_batch_decode_device_result(jtk_batch* b, const uint8_t** d_out, const int64_t** d_byte_off, const int32_t** d_status) {
    if (!b || !b->have_decode) return fail(JTK_ERR_INVALID_ARGUMENT, "no decode has run on this batch");
    if (d_out) *d_out = b->dwork.out;
    if (d_byte_off) *d_byte_off = b->dwork.byte_off;
    if (d_status) *d_status = b->dwork.status;
    return JTK_OK;
}

// ---- decode of an id matrix (jtk_decode_rows.hip) -----------------------------------------------------
static_assert(JTK_DECODE_MAX_STOP_IDS == JTK_DR_MAX_STOP, "the rule header holds as many stop ids as the ABI takes");

// the argument checks both entries share; *n_cells = n_rows * width
static int decode_rows_args(jtk_batch* b, const void* rows, int id_bytes, int64_t n_rows, int64_t width, int64_t row_stride,
                            const int64_t* stop_ids, int n_stop, uint32_t flags, int64_t* n_cells) {
    if (!b) return fail(JTK_ERR_INVALID_ARGUMENT, "batch is NULL");
    if (id_bytes != 4 && id_bytes != 8) return fail(JTK_ERR_INVALID_ARGUMENT, "id_bytes must be 4 or 8");
    if (n_rows < 0 || width < 0 || row_stride < 0) return fail(JTK_ERR_INVALID_ARGUMENT, "negative size");
    if (row_stride < width) return fail(JTK_ERR_INVALID_ARGUMENT, "row_stride is smaller than width");
    if (n_stop < 0 || n_stop > JTK_DECODE_MAX_STOP_IDS) return fail(JTK_ERR_INVALID_ARGUMENT, "n_stop must be 0..JTK_DECODE_MAX_STOP_IDS");
    if (n_stop > 0 && !stop_ids) return fail(JTK_ERR_INVALID_ARGUMENT, "stop_ids is NULL");
    if (flags & ~(uint32_t)(JTK_DECODE_SKIP_PAD | JTK_DECODE_KEEP_STOP)) return fail(JTK_ERR_INVALID_ARGUMENT, "unknown flag bits");
    const int64_t lim = (int64_t)1 << 58;                              // (element and byte counts stay far inside 64 bits)
    if (n_rows > 0 && row_stride > lim / n_rows) return fail(JTK_ERR_INVALID_ARGUMENT, "matrix too large");
    *n_cells = n_rows * width;
    if (*n_cells / JTK_DEC_TILE >= ((int64_t)1 << 31) - 1) return fail(JTK_ERR_INVALID_ARGUMENT, "matrix too large");
    if (*n_cells > 0 && !rows) return fail(JTK_ERR_INVALID_ARGUMENT, "rows is NULL");
    return JTK_OK;
}

int jtk_batch_decode_rows_device(jtk_batch* b, const void* d_rows, int id_bytes, int64_t n_rows, int64_t width, int64_t row_stride,
                                 const int64_t* d_begin_or_null, const int64_t* d_end_or_null, int64_t pad_id,
                                 const int64_t* stop_ids, int n_stop, uint32_t flags, int64_t* d_cell_byte_or_null,
                                 void* stream_or_null, int64_t* n_bytes) {
    int64_t n_cells = 0;
    int rc;
    if ((rc = decode_rows_args(b, d_rows, id_bytes, n_rows, width, row_stride, stop_ids, n_stop, flags, &n_cells))) return rc;
    const jtk_encoding* enc = b->enc;
    HIP_TRY(hipSetDevice(enc->device));
    drop_decode_result(b);           // (dec_zero, dec_tile and dec_byte_off below are the last decode's)
    hipStream_t s = pick_stream(b, stream_or_null);
    JtkDecodeRowsWork w{};
    w.rows = d_rows; w.id_bytes = id_bytes; w.n_rows = n_rows; w.width = width; w.row_stride = row_stride; w.n_cells = n_cells;
    w.n_tiles = (n_cells + JTK_DEC_TILE - 1) / JTK_DEC_TILE;
    w.begin = d_begin_or_null; w.end = d_end_or_null;
    w.rule.pad_id = pad_id; w.rule.n_stop = n_stop;
    for (int k = 0; k < n_stop; k++) w.rule.stop[k] = stop_ids[k];
    w.rule.skip_pad = (flags & JTK_DECODE_SKIP_PAD) != 0; w.rule.keep_stop = (flags & JTK_DECODE_KEEP_STOP) != 0;
    w.tab_off = (const uint32_t*)enc->dec_off.p; w.tab_blob = (const uint8_t*)enc->dec_blob.p; w.n_ids_table = enc->n_ids_table;
    const size_t nt = (size_t)(w.n_tiles > 0 ? w.n_tiles : 1);
    const size_t status_bytes = align_up((size_t)(n_rows > 0 ? n_rows : 1) * 4, 16);
    const size_t zero_bytes = status_bytes + 16;
    if ((rc = b->dec_zero.ensure(zero_bytes)) || (rc = b->dec_tile.ensure(nt * 4 + (nt + 1) * 8 + 16)) ||
        (rc = b->dec_byte_off.ensure(((size_t)n_rows + 1) * 8)) || (n_stop > 0 && (rc = b->dec_first.ensure((size_t)(n_rows > 0 ? n_rows : 1) * 8))))
        return rc;
    uint8_t* z = (uint8_t*)b->dec_zero.p;
    w.status = (int32_t*)z;
    w.total = (int64_t*)(z + status_bytes);
    w.tile_off = (int64_t*)b->dec_tile.p;
    w.tile_bytes = (uint32_t*)((uint8_t*)b->dec_tile.p + (nt + 1) * 8);
    w.byte_off = (int64_t*)b->dec_byte_off.p;
    w.cell_byte = d_cell_byte_or_null;
    w.first_stop = n_stop > 0 ? (unsigned long long*)b->dec_first.p : nullptr;
    // phase 1: sizes (the output is allocated once they are known)
    HIP_TRY(hipMemsetAsync(z, 0, zero_bytes, s));
    int64_t total = 0;
    if (n_cells > 0) {
        if (w.first_stop) HIP_TRY(hipMemsetAsync(w.first_stop, 0xFF, (size_t)n_rows * 8, s));      // JTK_DR_NO_STOP
        jtk_launch_decode_rows_count(w, s);
        HIP_TRY(hipMemcpyAsync(&total, w.total, 8, hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(hipStreamSynchronize(s));
    if ((rc = b->dec_out.ensure((size_t)total + 64))) return rc;
    w.out = (uint8_t*)b->dec_out.p;
    // phase 2: bytes, per-row offsets, per-cell offsets (a matrix without cells: every row is empty)
    if (n_cells > 0) jtk_launch_decode_rows_scatter(w, s);
    else HIP_TRY(hipMemsetAsync(w.byte_off, 0, ((size_t)n_rows + 1) * 8, s));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s));
    // the result is read as a flat decode's: jtk_batch_decode_fetch / jtk_batch_decode_device_result with n_seqs = n_rows
    b->dwork.n_seqs = n_rows; b->dwork.out = w.out; b->dwork.byte_off = w.byte_off; b->dwork.status = w.status;
    b->dec_total = total;
    b->dec_rows_width = width;
    b->have_decode = true;
    if (n_bytes) *n_bytes = total;
    return JTK_OK;
}

int jtk_batch_decode_rows(jtk_batch* b, const void* rows, int id_bytes, int64_t n_rows, int64_t width, int64_t row_stride,
                          const int64_t* begin_or_null, const int64_t* end_or_null, int64_t pad_id, const int64_t* stop_ids,
                          int n_stop, uint32_t flags, int64_t* cell_byte_or_null, int64_t* n_bytes) {
    int64_t n_cells = 0;
    int rc;
    if ((rc = decode_rows_args(b, rows, id_bytes, n_rows, width, row_stride, stop_ids, n_stop, flags, &n_cells))) return rc;
    HIP_TRY(hipSetDevice(b->enc->device));
    drop_decode_result(b);
    const size_t n_elem = n_cells > 0 ? (size_t)(n_rows - 1) * (size_t)row_stride + (size_t)width : 0;   // the last row's tail is not read
    const size_t row_bytes = (size_t)(n_rows > 0 ? n_rows : 1) * 8;
    if ((rc = b->dec_in_ids.ensure(n_elem * (size_t)id_bytes + 64)) || (rc = b->dec_in_win.ensure(2 * row_bytes)) ||
        (cell_byte_or_null && (rc = b->dec_cell.ensure((size_t)n_cells * 8 + 8))))
        return rc;
    int64_t* d_begin = begin_or_null ? (int64_t*)b->dec_in_win.p : nullptr;
    int64_t* d_end = end_or_null ? (int64_t*)((uint8_t*)b->dec_in_win.p + row_bytes) : nullptr;
    if (n_elem > 0) HIP_TRY(hipMemcpyAsync(b->dec_in_ids.p, rows, n_elem * (size_t)id_bytes, hipMemcpyHostToDevice, b->stream));
    if (d_begin && n_rows > 0) HIP_TRY(hipMemcpyAsync(d_begin, begin_or_null, (size_t)n_rows * 8, hipMemcpyHostToDevice, b->stream));
    if (d_end && n_rows > 0) HIP_TRY(hipMemcpyAsync(d_end, end_or_null, (size_t)n_rows * 8, hipMemcpyHostToDevice, b->stream));
    if ((rc = jtk_batch_decode_rows_device(b, b->dec_in_ids.p, id_bytes, n_rows, width, row_stride, d_begin, d_end, pad_id, stop_ids, n_stop,
                                           flags, cell_byte_or_null ? (int64_t*)b->dec_cell.p : nullptr, nullptr, n_bytes)))
        return rc;
    if (cell_byte_or_null && n_cells > 0) HIP_TRY(hipMemcpy(cell_byte_or_null, b->dec_cell.p, (size_t)n_cells * 8, hipMemcpyDeviceToHost));
    return JTK_OK;
}

int jtk_decode(const jtk_encoding* enc, const int32_t* ids, int64_t n, uint8_t* out, int64_t cap, int64_t* len) {
    if (!enc || n < 0 || (n > 0 && !ids)) return fail(JTK_ERR_INVALID_ARGUMENT, "bad arguments");
    const int64_t r = jtk_host_decode(enc->host, ids, n, out, cap);
    if (r == JTK_ERR_UNKNOWN_TOKEN) return fail(JTK_ERR_UNKNOWN_TOKEN, "Unknown token for decoding");
    if (r < 0) return fail((int)r, "decode buffer too small");
    if (len) *len = r;
    return JTK_OK;
}

}  // extern "C"

// Encoding.encode(text, maxTokens) from the full token list of `text` (GptBytePairEncoding.java:90-100): the first
// min(maxTokens, nt) tokens, backed off until decode(tokens) is a prefix of the text.  head: at least that many leading
// tokens.  Returns the count kept; *truncated = EncodingResult.isTruncated().
int64_t jtk_max_tokens_backoff(const jtk_encoding* enc, const uint8_t* utf8, int64_t len, const int32_t* head, int64_t nt,
                               int64_t max_tokens, int* truncated) {
    const int64_t keep = nt < max_tokens ? nt : max_tokens;
    int64_t nb = 0;
    for (int64_t k = 0; k < keep; k++) nb += enc->tok_len[(size_t)head[(size_t)k]];
    // truncated = text.length() > decoded.length(), both in UTF-16 units: the units before the cut are common to both, so only
    // the text from the cut on is counted
    const JtkBackoff r = jtk_maxtok_backoff(utf8, len, keep, nb, [&](int64_t k) { return (int64_t)enc->tok_len[(size_t)head[(size_t)k]]; });
    if (truncated) *truncated = r.ok && jtk_more_units_than(utf8, r.from, len, r.units);
    return r.keep;
}

extern "C" {

int jtk_encode(jtk_batch* b, const uint8_t* utf8, int64_t len, uint32_t flags, int64_t max_tokens,
               int32_t* tokens, int64_t tokens_cap, int64_t* n_tokens, int* truncated) {
    if (!b || len < 0) return fail(JTK_ERR_INVALID_ARGUMENT, "bad arguments");
    if (flags & JTK_ENCODE_ALLOW_SPECIAL) return fail(JTK_ERR_INVALID_ARGUMENT, "JTK_ENCODE_ALLOW_SPECIAL is for jtk_batch_encode / jtk_batch_encode_device");
    if (flags & JTK_ENCODE_FIM) return fail(JTK_ERR_INVALID_ARGUMENT, FIM_ELSEWHERE);
    if (flags & JTK_ENCODE_COMPACT_IDS) return fail(JTK_ERR_INVALID_ARGUMENT, "JTK_ENCODE_COMPACT_IDS is for jtk_batch_encode with JTK_ENCODE_TO_HOST");
    if (truncated) *truncated = 0;
    if (n_tokens) *n_tokens = 0;
    if (!utf8) return JTK_OK;                                    // text == null -> empty result
    if (max_tokens >= 0) {
        // encode(text, maxTokens): the leading bytes only (jtk_batch_encode_max_tokens below)
        const int64_t off2[2] = {0, len};
        std::vector<int32_t> head((size_t)((max_tokens < len ? max_tokens : len) + 1));
        int64_t keep = 0; uint8_t tr = 0; int32_t st = 0;
        int rc = jtk_batch_encode_max_tokens(b, utf8, off2, 1, flags & JTK_ENCODE_ORDINARY, max_tokens, head.data(), &keep, &tr, &st);
        if (rc != JTK_OK) return rc;
        if (st == JTK_ERR_UNSUPPORTED_SPECIAL) return fail(st, "Encoding special tokens is not supported yet.");
        if (st == JTK_ERR_UNENCODABLE) return fail(st, "Unknown token for encoding: the rank map lacks a single-byte token this text needs");
        if (st != JTK_OK) return fail(st, "document could not be encoded");
        if (truncated) *truncated = tr;
        if (n_tokens) *n_tokens = keep;
        if (tokens) {
            if (tokens_cap < keep) return fail(JTK_ERR_CAPACITY, "tokens buffer too small");
            if (keep > 0) memcpy(tokens, head.data(), (size_t)keep * 4);
        }
        return JTK_OK;
    }
    const int64_t off[2] = {0, len};
    int64_t nt = 0;
    // (the result comes back with the job -- status and ids in pinned host memory -- instead of two more copies behind it)
    int rc = jtk_batch_encode(b, utf8, off, 1, (flags & ~(uint32_t)JTK_ENCODE_COUNT_ONLY) | JTK_ENCODE_TO_HOST, &nt);
    if (rc != JTK_OK) return rc;
    const int32_t st = b->r_status[0];
    if (st == JTK_ERR_UNSUPPORTED_SPECIAL) return fail(st, "Encoding special tokens is not supported yet.");
    if (st == JTK_ERR_UNENCODABLE) return fail(st, "Unknown token for encoding: the rank map lacks a single-byte token this text needs");
    if (st != JTK_OK) return fail(st, "document could not be encoded");
    if (n_tokens) *n_tokens = nt;
    if (tokens) {
        if (tokens_cap < nt) return fail(JTK_ERR_CAPACITY, "tokens buffer too small");
        if (nt > 0) memcpy(tokens, b->r_tokens, (size_t)nt * 4);
    }
    return JTK_OK;
}

// Encoding.encode(text, maxTokens) for every document, without encoding the documents whole.  The reference stops matching
// once maxTokens tokens exist (GptBytePairEncoding.java:83-88); here each document's leading P bytes are encoded (P = 8 bytes
// per wanted token + 64 to begin with), and the result is taken when it is certain to be the head of the document's full token
// list: that is the tokens before a piece start q that (a) lies at least 16 bytes before the cut -- every look-ahead of the
// patterns (a contraction, the character after a white-space run) is shorter -- and (b) does not sit inside a white-space run
// that might reach the cut (`\s*[\r\n]+` and `\s+(?!\S)` look to the END of the run): text[q] is no white space, or it is one
// ASCII white-space character followed by something else.  Pieces before q are then matched exactly as in the whole text and
// pieces encode independently.  Documents whose prefix holds fewer than maxTokens such tokens go round again with 4x the bytes.
int jtk_batch_encode_max_tokens(jtk_batch* b, const uint8_t* utf8, const int64_t* doc_off, int64_t n_docs, uint32_t flags,
                                int64_t max_tokens, int32_t* tokens, int64_t* kept, uint8_t* truncated, int32_t* status) {
    if (!b || n_docs < 0 || !doc_off || max_tokens < 0 || !kept || (max_tokens > 0 && n_docs > 0 && !tokens))
        return fail(JTK_ERR_INVALID_ARGUMENT, "bad arguments");
    if (flags & JTK_ENCODE_ALLOW_SPECIAL) return fail(JTK_ERR_INVALID_ARGUMENT, "JTK_ENCODE_ALLOW_SPECIAL is for jtk_batch_encode / jtk_batch_encode_device");
    if (flags & JTK_ENCODE_FIM) return fail(JTK_ERR_INVALID_ARGUMENT, FIM_ELSEWHERE);
    if (doc_off[0] != 0) return fail(JTK_ERR_INVALID_ARGUMENT, "doc_off[0] must be 0");
    for (int64_t d = 0; d < n_docs; d++)
        if (doc_off[d + 1] < doc_off[d]) return fail(JTK_ERR_INVALID_ARGUMENT, "doc_off must be non-decreasing");
    const int64_t n_bytes = doc_off[n_docs];
    if (n_bytes > 0 && !utf8) return fail(JTK_ERR_INVALID_ARGUMENT, "utf8 is NULL");
    const jtk_encoding* enc = b->enc;
    std::vector<uint8_t> special((size_t)(n_docs > 0 ? n_docs : 1), 0);
    if (!(flags & JTK_ENCODE_ORDINARY)) find_special_docs(enc, utf8, n_bytes, doc_off, n_docs, special);   // text.contains(special) looks at the whole document (:52-56)
    std::vector<int64_t> active;
    active.reserve((size_t)n_docs);
    for (int64_t d = 0; d < n_docs; d++) {
        kept[d] = 0;
        if (truncated) truncated[d] = 0;
        if (status) status[d] = special[(size_t)d] ? JTK_ERR_UNSUPPORTED_SPECIAL : JTK_OK;
        if (special[(size_t)d]) continue;
        const int64_t len = doc_off[d + 1] - doc_off[d];
        if (len == 0 || max_tokens == 0) {
            int tr = 0;
            jtk_max_tokens_backoff(enc, utf8 + doc_off[d], len, nullptr, 0, 0, &tr);
            if (truncated) truncated[d] = (uint8_t)tr;
            continue;
        }
        active.push_back(d);
    }
    const int64_t cb = b->host_chunk_bytes < b->chunk_bytes ? b->host_chunk_bytes : b->chunk_bytes;   // a group stays one chunk
    int64_t P = jtk_maxtok_first_prefix(max_tokens);
    uint8_t* gtext = nullptr;                                        // (pinned: the prefixes go down by DMA while the kernels start)
    std::vector<int64_t> goff, next_active;
    std::vector<uint64_t> mask;
    const bool trace = getenv("JTK_MAXTOK_TRACE") != nullptr;
    auto now = [] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double t_begin = now();
    double t_gather = 0, t_enc = 0, t_dec = 0, t_mask = 0;
    while (!active.empty()) {
        next_active.clear();
        size_t a0 = 0;
        while (a0 < active.size()) {
            // one group: as many prefixes as fit one chunk
            size_t a1 = a0;
            int64_t gbytes = 0;
            goff.assign(1, 0);
            while (a1 < active.size()) {
                const int64_t d = active[a1], len = doc_off[d + 1] - doc_off[d];
                const int64_t p = jtk_maxtok_prefix_bytes(len, P, cb);     // past one host chunk the document goes whole, and alone
                if (a1 > a0 && gbytes + p > cb) break;
                gbytes += p;
                goff.push_back(gbytes);
                a1++;
            }
            double t0 = now();
            { const int prc = b->h_gather.ensure((size_t)gbytes + 64); if (prc) return prc; }
            gtext = b->h_gather.p;
            host_slices(a1 - a0, [&](int, size_t lo, size_t hi) {
                for (size_t i = lo; i < hi; i++)
                    memcpy(gtext + goff[i], utf8 + doc_off[active[a0 + i]], (size_t)(goff[i + 1] - goff[i]));
            });
            const int64_t ng = (int64_t)(a1 - a0);
            int64_t nt = 0;
            const int64_t save_host_chunk = b->host_chunk_bytes;
            if (gbytes > cb) b->host_chunk_bytes = gbytes;           // a single document above the host chunk size: still one chunk
            double t1 = now(); t_gather += t1 - t0;
            int rc = jtk_batch_encode(b, gtext, goff.data(), ng, JTK_ENCODE_ORDINARY | JTK_ENCODE_TO_HOST, &nt);
            b->host_chunk_bytes = save_host_chunk;
            double t2 = now(); t_enc += t2 - t1;
            if (rc != JTK_OK) return rc;
            if (b->chunk_doc.size() != 2) {
                // longer than a device chunk: no single piece mask; such a document is encoded whole
                const int32_t* toks = b->r_tokens; const int64_t* toff = b->r_tok_off;
                for (size_t a = a0; a < a1; a++) {
                    const int64_t d = active[a], len = doc_off[d + 1] - doc_off[d], i = (int64_t)(a - a0);
                    if (goff[i + 1] - goff[i] != len) return fail(JTK_ERR_INVALID_ARGUMENT, "max-tokens prefix spans device chunks");
                    int tr = 0;
                    const int64_t k = jtk_max_tokens_backoff(enc, utf8 + doc_off[d], len, toks + toff[i], toff[i + 1] - toff[i], max_tokens, &tr);
                    if (k > 0) memcpy(tokens + d * max_tokens, toks + toff[i], (size_t)k * 4);
                    kept[d] = k;
                    if (truncated) truncated[d] = (uint8_t)tr;
                }
                a0 = a1;
                continue;
            }
            const int32_t* toks = b->r_tokens; const int64_t* toff = b->r_tok_off; const int32_t* st = b->r_status;
            const size_t n_words = (size_t)((gbytes + 1 + 63) / 64);
            mask.resize(n_words);
            {
                double tm = now();
                HIP_TRY(hipMemcpy(mask.data(), b->set[0].piecemask.p, n_words * 8, hipMemcpyDeviceToHost));
                t_mask += now() - tm;
            }
            std::vector<int64_t> again[8];
            host_slices(a1 - a0, [&](int slice, size_t lo, size_t hi) {
                for (size_t ii = lo; ii < hi; ii++) {
                    const int64_t i = (int64_t)ii, d = active[a0 + ii], len = doc_off[d + 1] - doc_off[d];
                    const int64_t p = goff[i + 1] - goff[i], t0 = toff[i], n = toff[i + 1] - t0;
                    if (st[i] != JTK_OK) { if (status) status[d] = st[i]; continue; }
                    int64_t k = -1;
                    if (p == len) k = n;
                    else {
                        // the last safe piece start at or before p - JTK_MAXTOK_MARGIN
                        const int64_t q = jtk_maxtok_last_safe_start(mask.data(), goff[i], gtext + goff[i], p);
                        if (q > 0 && n >= max_tokens) {
                            int64_t cum = 0;
                            for (int64_t kk = 0; kk < max_tokens && cum <= q; kk++) cum += enc->tok_len[(size_t)toks[t0 + kk]];
                            if (jtk_maxtok_decided(n, max_tokens, cum, q)) k = max_tokens;          // maxTokens tokens, all before q
                        }
                    }
                    if (k < 0) { again[slice].push_back(d); continue; }
                    int tr = 0;
                    // (the back-off looks at the text around the cut only: that is inside the prefix, which is in the cache -- the
                    // document itself is a cold line per look)
                    const int64_t keep = jtk_max_tokens_backoff(enc, gtext + goff[i], len, toks + t0, k, max_tokens, &tr);
                    if (keep > 0) memcpy(tokens + d * max_tokens, toks + t0, (size_t)keep * 4);
                    kept[d] = keep;
                    if (truncated) truncated[d] = (uint8_t)tr;
                }
            });
            for (auto& v : again) next_active.insert(next_active.end(), v.begin(), v.end());
            t_dec += now() - t2;
            a0 = a1;
        }
        if (trace) fprintf(stderr, "[max_tokens] P=%lld docs=%zu -> %zu again; gather %.2f encode %.2f mask %.2f decide(incl. mask) %.2f ms; %.2f ms since the rounds began\n",
                           (long long)P, active.size(), next_active.size(), t_gather, t_enc, t_mask, t_dec, now() - t_begin);
        active.swap(next_active);
        P = jtk_maxtok_next_prefix(P);
    }
    return JTK_OK;
}

// jtk_batch_encode_max_tokens with device input and device rows: the same rounds, as kernels (jtk_maxtok.hip).  Per round the
// host reads one 16-byte word (open documents, gathered bytes) to size the gather and the encode; everything else stays on the
// device.  The decisions run as run_job's per-chunk epilogue.
int jtk_batch_encode_device_max_tokens(jtk_batch* b, const uint8_t* d_utf8, const int64_t* d_doc_off, int64_t n_docs,
                                       int64_t n_bytes, uint32_t flags, int64_t max_tokens, int32_t pad_id,
                                       int32_t* d_tokens, int64_t* d_kept, uint8_t* d_truncated, int32_t* d_status,
                                       void* stream_or_null) {
    if (!b || n_docs < 0 || n_bytes < 0 || (n_bytes > 0 && !d_utf8) || !d_doc_off || max_tokens < 0 ||
        (max_tokens > 0 && n_docs > 0 && !d_tokens) || (n_docs > 0 && (!d_kept || !d_truncated || !d_status)))
        return fail(JTK_ERR_INVALID_ARGUMENT, "bad arguments");
    if (flags & ~(uint32_t)JTK_ENCODE_ORDINARY) return fail(JTK_ERR_INVALID_ARGUMENT, "flags: JTK_ENCODE_ORDINARY or 0");
    if (n_bytes >= (int64_t)1 << 37) return fail(JTK_ERR_INVALID_ARGUMENT, "batch too large (128 GiB of text per call at most)");
    const jtk_encoding* enc = b->enc;
    HIP_TRY(hipSetDevice(enc->device));
    // the batch's last encode result is given up (its chunk plan and scratch are reused below), and the rounds' prefix jobs
    // are not results of the batch: none is left on any return path
    struct NoResult {
        jtk_batch* b;
        ~NoResult() { drop_encode_result(b); b->plan_doc_off = nullptr; }
    } no_result{b};
    drop_encode_result(b);
    if (n_docs == 0) return JTK_OK;
    hipStream_t s = pick_stream(b, stream_or_null);
    const size_t nd = (size_t)n_docs;
    const int64_t n_blk = (n_docs + 1023) / 1024;
    // scratch: hdr (4 x i64: open documents, gathered bytes, bad flag) | act[2][nd] | goff[nd + 1] | blk_base[2 * n_blk] |
    //          blk_bytes[n_blk] | blk_cnt[n_blk] | special[nd] | again[2][nd]
    const size_t o_act = 32, o_goff = o_act + 2 * nd * 8, o_base = o_goff + (nd + 1) * 8, o_bb = o_base + (size_t)n_blk * 16,
                 o_bc = o_bb + (size_t)n_blk * 8, o_sp = align_up(o_bc + (size_t)n_blk * 4, 16), o_ag = o_sp + align_up(nd, 16),
                 total = o_ag + 2 * align_up(nd, 16);
    int rc;
    if ((rc = b->mt_scratch.ensure(total)) || (rc = b->h_mt.ensure(16))) return rc;
    uint8_t* z = (uint8_t*)b->mt_scratch.p;
    JtkMaxTokWork m{};
    m.text = d_utf8; m.doc_off = d_doc_off; m.n_docs = n_docs; m.n_bytes = n_bytes;
    m.max_tokens = max_tokens; m.pad_id = pad_id;
    m.out_tokens = d_tokens; m.out_kept = d_kept; m.out_truncated = d_truncated; m.out_status = d_status;
    m.hdr = (int64_t*)z; m.bad = (uint32_t*)(z + 16);
    m.goff = (int64_t*)(z + o_goff);
    m.blk_base = (int64_t*)(z + o_base); m.blk_bytes = (int64_t*)(z + o_bb); m.blk_cnt = (uint32_t*)(z + o_bc);
    m.special = z + o_sp;
    m.tab_off = (const uint32_t*)enc->dec_off.p; m.n_ids_table = enc->n_ids_table;
    int64_t* act[2] = {(int64_t*)(z + o_act), (int64_t*)(z + o_act) + nd};
    uint8_t* again[2] = {z + o_ag, z + o_ag + align_up(nd, 16)};
    // round 1: offsets, encode()'s special-token check over the whole text, the rows that need no encode
    HIP_TRY(hipMemsetAsync(z, 0, 32, s));
    HIP_TRY(hipMemsetAsync(m.special, 0, nd, s));
    jtk_launch_maxtok_check(m, s);
    if (!(flags & JTK_ENCODE_ORDINARY)) jtk_launch_maxtok_special(m, enc->dt, s);
    jtk_launch_maxtok_finish_closed(m, s);
    HIP_TRY(hipGetLastError());
    // as on the host (jtk_batch_encode_max_tokens): the same prefix sizes, so that the same bytes are encoded
    const int64_t cb = b->host_chunk_bytes < b->chunk_bytes ? b->host_chunk_bytes : b->chunk_bytes;
    const bool trace = getenv("JTK_MAXTOK_TRACE") != nullptr;
    int64_t n_in = n_docs;
    for (int round = 1;; round++) {
        const int cur = (round - 1) & 1;
        m.round = round;
        m.P = round == 1 ? jtk_maxtok_first_prefix(max_tokens) : jtk_maxtok_next_prefix(m.P);
        m.cb = cb;
        m.n_in = n_in;
        m.n_blk = (n_in + 1023) / 1024;
        m.act_in = act[cur ^ 1]; m.again_in = again[cur ^ 1];
        m.act = act[cur]; m.again = again[cur];
        Event ev[5];
        if (trace) for (auto& e : ev) HIP_TRY(e.create_timed());
        if (trace) HIP_TRY(hipEventRecord(ev[0], s));
        jtk_launch_maxtok_plan(m, s);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(b->h_mt.p, m.hdr, 16, hipMemcpyDeviceToHost, s));
        if (trace) HIP_TRY(hipEventRecord(ev[1], s));
        HIP_TRY(hipStreamSynchronize(s));
        const int64_t n_act = b->h_mt.p[0], gbytes = b->h_mt.p[1];
        if (n_act < 0) return fail(JTK_ERR_INVALID_ARGUMENT, "document offsets are not non-decreasing within [0, n_bytes]");
        if (n_act == 0) break;
        if ((rc = b->mt_gather.ensure((size_t)gbytes + 64))) return rc;
        m.gather = (uint8_t*)b->mt_gather.p;
        m.gbytes = gbytes;
        jtk_launch_maxtok_gather(m, n_act, s);
        HIP_TRY(hipGetLastError());
        if (trace) HIP_TRY(hipEventRecord(ev[2], s));
        if ((rc = plan_device_chunks(b, m.goff, n_act, gbytes, s))) return rc;
        if (trace) HIP_TRY(hipEventRecord(ev[3], s));
        rc = run_job(b, m.gather, nullptr, m.goff, n_act, gbytes, JTK_ENCODE_ORDINARY, s, false, nullptr, &m);
        if (rc != JTK_OK) return rc;
        if (trace) {
            HIP_TRY(hipEventRecord(ev[4], s));
            HIP_TRY(hipStreamSynchronize(s));
            float t_plan = 0, t_gather = 0, t_encode = 0;
            (void)hipEventElapsedTime(&t_plan, ev[0], ev[1]);
            (void)hipEventElapsedTime(&t_gather, ev[1], ev[2]);
            (void)hipEventElapsedTime(&t_encode, ev[3], ev[4]);
            fprintf(stderr, "[device max_tokens] round %d P=%lld docs=%lld bytes=%lld chunks=%zu: plan %.3f gather %.3f encode+decide %.3f ms\n",
                    round, (long long)m.P, (long long)n_act, (long long)gbytes, b->chunk_doc.size() - 1, t_plan, t_gather, t_encode);
        }
        n_in = n_act;
    }
    return JTK_OK;
}


// ---- chunks of the last encode (jtk_chunk.hip) --------------------------------------------------------------------------
// `to` waits for the work queued on `from` so far (nothing when they are the same stream).
static int ck_order(jtk_batch* b, hipStream_t from, hipStream_t to) {
    if (from == to) return JTK_OK;
    HIP_TRY(b->ev_ck.create());
    HIP_TRY(hipEventRecord(b->ev_ck, from));
    HIP_TRY(hipStreamWaitEvent(to, b->ev_ck, 0));
    return JTK_OK;
}

// the inputs of the chunk kernels (the last encode) and the per-document scratch: hdr[4] | chunk_off[nd + 1] | long[nd] | dbase[nd]
static int ck_setup(jtk_batch* b) {
    const size_t nd = (size_t)b->job_docs;
    int rc;
    if ((rc = b->ck_scratch.ensure(32 + (3 * nd + 1) * 8))) return rc;
    JtkChunkWork& w = b->ck;
    w = JtkChunkWork{};
    b->ck_end_level = nullptr;
    w.tokens = (const int32_t*)b->tokens.p; w.tok_off = (const int64_t*)b->tok_off.p; w.status = (const int32_t*)b->status.p;
    w.doc_off = b->job_doc_off; w.n_docs = b->job_docs;
    w.bnd = (const uint32_t*)b->enc->bnd.p; w.tab_off = (const uint32_t*)b->enc->dec_off.p; w.n_ids_table = b->enc->n_ids_table;
    w.hdr = (int64_t*)b->ck_scratch.p;
    w.chunk_off = w.hdr + 4;
    w.long_docs = w.chunk_off + nd + 1;
    w.dbase = w.long_docs + nd;
    return JTK_OK;
}

// the byte scan over the tokens (tiles, sub16) and the document bases
static int ck_tiles(jtk_batch* b, int64_t n_tok, hipStream_t s) {
    JtkChunkWork& w = b->ck;
    w.n_tok = n_tok;
    w.n_tiles = (n_tok + JTK_DEC_TILE - 1) / JTK_DEC_TILE;
    const size_t o_off = align_up((size_t)w.n_tiles * 4 + 4, 16), o_sub = o_off + ((size_t)w.n_tiles + 1) * 8;
    int rc;
    if ((rc = b->ck_tiles.ensure(o_sub + ((size_t)n_tok / 16 + 1) * 4))) return rc;
    w.tile_bytes = (uint32_t*)b->ck_tiles.p;
    w.tile_off = (int64_t*)((uint8_t*)b->ck_tiles.p + o_off);
    w.sub16 = (uint32_t*)((uint8_t*)b->ck_tiles.p + o_sub);
    jtk_launch_chunk_tiles(w, s);
    HIP_TRY(hipGetLastError());
    b->have_tiles = true;
    return JTK_OK;
}

// the byte scan of the last encode's tokens, ready on s: the one a chunk plan or an earlier position call left, or a new one
// behind the encode
static int ck_byte_scan(jtk_batch* b, hipStream_t s) {
    if (b->have_tiles) return ck_order(b, b->ck_stream, s);
    int64_t nt = 0;
    int rc;
    if ((rc = jtk_batch_result(b, &nt, nullptr, nullptr)) || (rc = ck_order(b, b->last_stream, s)) || (rc = ck_setup(b)) ||
        (rc = ck_tiles(b, nt, s)))
        return rc;
    b->ck_stream = s;
    return JTK_OK;
}

// the records of nc chunks in ck_rec: chunk_doc | tok_begin | byte_begin | byte_end (i64) | n_tok (i32) | split (u8), and
// behind them, when end_level is asked for, end_level (u8)
static int ck_records(jtk_batch* b, int64_t nc, uint8_t** end_level) {
    const size_t n = (size_t)(nc > 0 ? nc : 1), o_i32 = 4 * n * 8, o_u8 = align_up(o_i32 + n * 4, 16);
    int rc;
    if ((rc = b->ck_rec.ensure(o_u8 + (end_level ? 2 : 1) * n))) return rc;
    JtkChunkWork& w = b->ck;
    int64_t* r64 = (int64_t*)b->ck_rec.p;
    w.chunk_doc = r64; w.tok_begin = r64 + n; w.byte_begin = r64 + 2 * n; w.byte_end = r64 + 3 * n;
    w.n_tok_out = (int32_t*)((uint8_t*)b->ck_rec.p + o_i32);
    w.split = (uint8_t*)b->ck_rec.p + o_u8;
    w.n_chunks = nc;
    if (end_level) *end_level = w.split + n;
    return JTK_OK;
}

int jtk_batch_chunk(jtk_batch* b, int64_t chunk_tokens, int64_t overlap, void* stream_or_null, int64_t* n_chunks) {
    if (!b || !n_chunks) return fail(JTK_ERR_INVALID_ARGUMENT, "bad arguments");
    *n_chunks = 0;
    int rc;
    if ((rc = need_encode(b, NEED_IDS | NEED_TEXT_ORDER))) return rc;
    if (chunk_tokens < 1 || chunk_tokens > INT32_MAX) return fail(JTK_ERR_INVALID_ARGUMENT, "chunk_tokens must be in [1, 2^31 - 1]");
    if (overlap < 0 || overlap >= chunk_tokens) return fail(JTK_ERR_INVALID_ARGUMENT, "overlap must be in [0, chunk_tokens)");
    HIP_TRY(hipSetDevice(b->enc->device));
    hipStream_t s = pick_stream(b, stream_or_null);
    b->have_chunk = false;
    b->have_tiles = false;
    if ((rc = ck_order(b, b->last_stream, s)) || (rc = ck_setup(b)) || (rc = b->h_ck.ensure(32))) return rc;
    JtkChunkWork& w = b->ck;
    w.N = chunk_tokens; w.overlap = overlap;
    // count per document, scan; the one wait: (chunks, tokens)
    HIP_TRY(hipMemsetAsync(w.hdr, 0, 32, s));
    jtk_launch_chunk_count(w, s);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(b->h_ck.p, w.hdr, 16, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    const int64_t nc = b->h_ck.p[0], nt = b->h_ck.p[1];
    if ((rc = ck_tiles(b, nt, s)) || (rc = ck_records(b, nc, nullptr))) return rc;
    jtk_launch_chunk_write(w, s);
    HIP_TRY(hipGetLastError());
    b->have_chunk = true;
    b->ck_stream = s;
    *n_chunks = nc;
    return JTK_OK;
}

int jtk_batch_chunk_fetch(jtk_batch* b, int64_t* chunk_off, int64_t* chunk_doc, int64_t* tok_begin, int32_t* n_tok,
                          int64_t* byte_begin, int64_t* byte_end, uint8_t* split) {
    if (!b || !b->have_chunk) return fail(JTK_ERR_INVALID_ARGUMENT, "jtk_batch_chunk has not run on the last encode of this batch");
    HIP_TRY(hipSetDevice(b->enc->device));
    HIP_TRY(hipStreamSynchronize(b->ck_stream));
    const JtkChunkWork& w = b->ck;
    const size_t nc = (size_t)w.n_chunks;
    if (chunk_off) HIP_TRY(hipMemcpy(chunk_off, w.chunk_off, ((size_t)w.n_docs + 1) * 8, hipMemcpyDeviceToHost));
    if (nc) {
        if (chunk_doc) HIP_TRY(hipMemcpy(chunk_doc, w.chunk_doc, nc * 8, hipMemcpyDeviceToHost));
        if (tok_begin) HIP_TRY(hipMemcpy(tok_begin, w.tok_begin, nc * 8, hipMemcpyDeviceToHost));
        if (n_tok) HIP_TRY(hipMemcpy(n_tok, w.n_tok_out, nc * 4, hipMemcpyDeviceToHost));
        if (byte_begin) HIP_TRY(hipMemcpy(byte_begin, w.byte_begin, nc * 8, hipMemcpyDeviceToHost));
        if (byte_end) HIP_TRY(hipMemcpy(byte_end, w.byte_end, nc * 8, hipMemcpyDeviceToHost));
        if (split) HIP_TRY(hipMemcpy(split, w.split, nc, hipMemcpyDeviceToHost));
    }
    return JTK_OK;
}

int jtk_batch_chunk_device_result(jtk_batch* b, const int64_t** d_chunk_off, const int64_t** d_chunk_doc,
                                  const int64_t** d_tok_begin, const int32_t** d_n_tok, const int64_t** d_byte_begin,
                                  const int64_t** d_byte_end, const uint8_t** d_split) {
    if (!b || !b->have_chunk) return fail(JTK_ERR_INVALID_ARGUMENT, "jtk_batch_chunk has not run on the last encode of this batch");
    const JtkChunkWork& w = b->ck;
    if (d_chunk_off) *d_chunk_off = w.chunk_off;
    if (d_chunk_doc) *d_chunk_doc = w.chunk_doc;
    if (d_tok_begin) *d_tok_begin = w.tok_begin;
    if (d_n_tok) *d_n_tok = w.n_tok_out;
    if (d_byte_begin) *d_byte_begin = w.byte_begin;
    if (d_byte_end) *d_byte_end = w.byte_end;
    if (d_split) *d_split = w.split;
    return JTK_OK;
}

int jtk_batch_chunk_rows(jtk_batch* b, int32_t pad_id, int32_t* d_rows, void* stream_or_null) {
    if (!b || !b->have_chunk) return fail(JTK_ERR_INVALID_ARGUMENT, "jtk_batch_chunk has not run on the last encode of this batch");
    if (b->ck.n_chunks > 0 && !d_rows) return fail(JTK_ERR_INVALID_ARGUMENT, "d_rows is NULL");
    if (((uintptr_t)d_rows & 3u) != 0) return fail(JTK_ERR_INVALID_ARGUMENT, "d_rows must be 4-byte aligned");
    HIP_TRY(hipSetDevice(b->enc->device));
    hipStream_t s = pick_stream(b, stream_or_null);
    int rc;
    if ((rc = ck_order(b, b->ck_stream, s))) return rc;
    jtk_launch_chunk_rows(b->ck, pad_id, d_rows, s);
    HIP_TRY(hipGetLastError());
    return JTK_OK;
}

int jtk_batch_compact(jtk_batch* b, uint16_t* d_lo, uint32_t* d_hi, void* stream_or_null) {
    int rc;
    if ((rc = need_encode(b, NEED_IDS))) return rc;
    if (((uintptr_t)d_lo & 1u) != 0 || ((uintptr_t)d_hi & 3u) != 0) return fail(JTK_ERR_INVALID_ARGUMENT, "d_lo must be 2-byte and d_hi 4-byte aligned");
    HIP_TRY(hipSetDevice(b->enc->device));
    int64_t nt = 0;
    if ((rc = jtk_batch_result(b, &nt, nullptr, nullptr))) return rc;
    const int hb = b->enc->hb;
    if (nt > 0 && (!d_lo || (hb && !d_hi))) return fail(JTK_ERR_INVALID_ARGUMENT, hb ? "d_lo or d_hi is NULL" : "d_lo is NULL");
    hipStream_t s = pick_stream(b, stream_or_null);
    if ((rc = ck_order(b, b->last_stream, s))) return rc;
    jtk_launch_compact((const int32_t*)b->tokens.p, 0, nt, nullptr, d_lo, d_hi, 0, hb, s);
    HIP_TRY(hipGetLastError());
    return JTK_OK;
}

// ---- MinHash signatures of the last encode (jtk_minhash.hip) -------------------------------------------------------------
int jtk_batch_minhash(jtk_batch* b, const jtk_minhash_params* p, uint32_t* d_sig, int32_t* d_n_shingles, uint64_t* d_band_keys,
                      void* stream_or_null) {
    int rc;
    if ((rc = need_encode(b, NEED_IDS))) return rc;
    if (!p) return fail(JTK_ERR_INVALID_ARGUMENT, "params is NULL");
    if (!jtk_mh_params_ok(p->ngram, p->num_hashes, p->bands, p->flags))
        return fail(JTK_ERR_INVALID_ARGUMENT, "minhash: ngram 1..32, num_hashes 1..256, bands 0 or a divisor of num_hashes, flags 0");
    if (((uintptr_t)d_sig & 3u) || ((uintptr_t)d_n_shingles & 3u) || ((uintptr_t)d_band_keys & 7u))
        return fail(JTK_ERR_INVALID_ARGUMENT, "unaligned array (4-byte sig and n_shingles, 8-byte band keys)");
    HIP_TRY(hipSetDevice(b->enc->device));
    int64_t nt = 0;
    if ((rc = jtk_batch_result(b, &nt, nullptr, nullptr))) return rc;
    if (b->job_docs > 0 && !d_sig) return fail(JTK_ERR_INVALID_ARGUMENT, "d_sig is NULL");
    hipStream_t s = pick_stream(b, stream_or_null);
    if ((rc = ck_order(b, b->last_stream, s))) return rc;
    JtkMhView v;
    v.tokens = (const int32_t*)b->tokens.p; v.tok_off = (const int64_t*)b->tok_off.p; v.status = (const int32_t*)b->status.p;
    v.n_docs = b->job_docs; v.total = nt; v.ngram = p->ngram;
    jtk_launch_minhash(v, p->seed, p->num_hashes, p->bands, d_sig, d_n_shingles, d_band_keys, s);
    HIP_TRY(hipGetLastError());
    return JTK_OK;
}

int jtk_batch_minhash_agree(jtk_batch* b, const uint32_t* d_sig, int64_t n_sig, int32_t num_hashes, const int64_t* d_pair_a,
                            const int64_t* d_pair_b, int64_t n_pairs, int32_t* d_agree, void* stream_or_null) {
    if (!b) return fail(JTK_ERR_INVALID_ARGUMENT, "batch is NULL");
    if (num_hashes < 1 || num_hashes > JTK_MH_MAX_HASHES) return fail(JTK_ERR_INVALID_ARGUMENT, "num_hashes must be in 1..256");
    if (n_sig < 0 || n_pairs < 0) return fail(JTK_ERR_INVALID_ARGUMENT, "n_sig and n_pairs must not be negative");
    if (n_pairs > 0 && (!d_pair_a || !d_pair_b || !d_agree || (n_sig > 0 && !d_sig)))
        return fail(JTK_ERR_INVALID_ARGUMENT, "d_sig, d_pair_a, d_pair_b or d_agree is NULL");
    if (((uintptr_t)d_sig & 3u) || ((uintptr_t)d_pair_a & 7u) || ((uintptr_t)d_pair_b & 7u) || ((uintptr_t)d_agree & 3u))
        return fail(JTK_ERR_INVALID_ARGUMENT, "unaligned array (4-byte sig and agree, 8-byte int64 pairs)");
    HIP_TRY(hipSetDevice(b->enc->device));
    jtk_launch_minhash_agree(d_sig, n_sig, num_hashes, d_pair_a, d_pair_b, n_pairs, d_agree, pick_stream(b, stream_or_null));
    HIP_TRY(hipGetLastError());
    return JTK_OK;
}

// ---- token n-gram sets and overlap (jtk_ngram.hip) ----------------------------------------------------------------------
// A set lives on its encoding's device and outlives batches.  Its calls may come on different streams: each call that queues work
// first makes its stream wait for `ev` (ng_wait) and records `ev` behind what it queued (ng_done), so the calls take effect in
// the order they were made, and no stream handle is kept.
struct jtk_ngram_set {
    const jtk_encoding* enc = nullptr;
    jtk_ngram_params p{};
    DevBuf table;                    // uint64 [capacity], 0 = empty
    int64_t capacity = 0;
    DevBuf d_hdr;                    // uint64: [0] the key count, [1] the n-grams of the batch that is being added
    Stream own;                      // add_keys and the reads
    Event ev;
    uint64_t* slots() const { return (uint64_t*)table.p; }
    uint64_t* hdr() const { return (uint64_t*)d_hdr.p; }
};

static int ng_wait(const jtk_ngram_set* s, hipStream_t st) { HIP_TRY(hipStreamWaitEvent(st, s->ev, 0)); return JTK_OK; }
static int ng_done(const jtk_ngram_set* s, hipStream_t st) { HIP_TRY(hipEventRecord(s->ev, st)); return JTK_OK; }

static void ng_free(jtk_ngram_set* s) {
    if (s->ev) (void)hipEventSynchronize(s->ev);                // (the last call that queued work on the table)
    delete s;
}

// room for m more keys beside c, by the capacity rule; a larger table is filled from the old one on `st`, which is waited for
static int ng_reserve(jtk_ngram_set* s, int64_t c, int64_t m, hipStream_t st) {
    const int64_t cap = jtk_ng_capacity(c, m);
    if (cap <= s->capacity) return JTK_OK;
    DevBuf grown;
    hipError_t e = grown.alloc((size_t)cap * 8);
    if (e != hipSuccess) return fail(JTK_ERR_OUT_OF_MEMORY, std::string("hipMalloc (n-gram table): ") + hipGetErrorString(e));
    e = hipMemsetAsync(grown.p, 0, (size_t)cap * 8, st);
    if (e == hipSuccess) {
        jtk_launch_ngram_insert_keys(s->slots(), s->capacity, (uint64_t*)grown.p, cap, nullptr, st);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return fail(JTK_ERR_HIP, std::string("n-gram table growth: ") + hipGetErrorString(e));
    s->table = std::move(grown);     // (frees the old table: the insert that read it is done)
    s->capacity = cap;
    return JTK_OK;
}

static JtkMhView ng_view(const jtk_batch* b, int64_t nt, int32_t ngram) {
    JtkMhView v;
    v.tokens = (const int32_t*)b->tokens.p; v.tok_off = (const int64_t*)b->tok_off.p; v.status = (const int32_t*)b->status.p;
    v.n_docs = b->job_docs; v.total = nt; v.ngram = ngram;
    return v;
}

int jtk_ngram_set_create(const jtk_encoding* enc, const jtk_ngram_params* p, jtk_ngram_set** out) {
    if (!enc || !p || !out) return fail(JTK_ERR_INVALID_ARGUMENT, "enc, params or out is NULL");
    if (!jtk_ng_params_ok(p->ngram, p->flags)) return fail(JTK_ERR_INVALID_ARGUMENT, "n-gram set: ngram 1..32, flags 0");
    HIP_TRY(hipSetDevice(enc->device));
    jtk_ngram_set* s = new (std::nothrow) jtk_ngram_set();
    if (!s) return fail(JTK_ERR_OUT_OF_MEMORY, "out of host memory");
    s->enc = enc;
    s->p = *p;
    s->capacity = jtk_ng_capacity(0, 0);
    hipError_t e = s->own.create();
    if (e == hipSuccess) e = s->ev.create();
    if (e == hipSuccess) e = s->table.alloc((size_t)s->capacity * 8);
    if (e == hipSuccess) e = s->d_hdr.alloc(16);
    if (e == hipSuccess) e = hipMemsetAsync(s->table.p, 0, (size_t)s->capacity * 8, s->own);
    if (e == hipSuccess) e = hipMemsetAsync(s->d_hdr.p, 0, 16, s->own);
    if (e == hipSuccess) e = hipEventRecord(s->ev, s->own);
    if (e != hipSuccess) {
        ng_free(s);
        return fail(e == hipErrorOutOfMemory ? JTK_ERR_OUT_OF_MEMORY : JTK_ERR_HIP, std::string("jtk_ngram_set_create: ") + hipGetErrorString(e));
    }
    *out = s;
    return JTK_OK;
}

void jtk_ngram_set_destroy(jtk_ngram_set* s) {
    if (!s) return;
    (void)hipSetDevice(s->enc->device);
    ng_free(s);
}

int jtk_ngram_set_add_batch(jtk_ngram_set* s, jtk_batch* b, void* stream_or_null) {
    if (!s) return fail(JTK_ERR_INVALID_ARGUMENT, "the n-gram set is NULL");
    int rc;
    if ((rc = need_encode(b, NEED_IDS))) return rc;
    if (b->enc != s->enc) return fail(JTK_ERR_INVALID_ARGUMENT, "the batch belongs to another encoding object than the n-gram set");
    HIP_TRY(hipSetDevice(b->enc->device));
    int64_t nt = 0;
    if ((rc = jtk_batch_result(b, &nt, nullptr, nullptr))) return rc;
    hipStream_t st = pick_stream(b, stream_or_null);
    if ((rc = ck_order(b, b->last_stream, st)) || (rc = ng_wait(s, st))) return rc;
    const JtkMhView v = ng_view(b, nt, s->p.ngram);
    HIP_TRY(hipMemsetAsync(s->hdr() + 1, 0, 8, st));
    jtk_launch_ngram_count(v, s->hdr() + 1, st);
    HIP_TRY(hipGetLastError());
    int64_t h[2] = {0, 0};                                   // keys in the set, n-grams in the batch
    HIP_TRY(hipMemcpyAsync(h, s->hdr(), 16, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if ((rc = ng_reserve(s, h[0], h[1], st))) return rc;
    jtk_launch_ngram_insert(v, s->p.seed, s->slots(), s->capacity, s->hdr(), st);
    HIP_TRY(hipGetLastError());
    return ng_done(s, st);
}

int jtk_ngram_set_add_keys(jtk_ngram_set* s, const uint64_t* keys, int64_t n) {
    if (!s) return fail(JTK_ERR_INVALID_ARGUMENT, "the n-gram set is NULL");
    if (n < 0) return fail(JTK_ERR_INVALID_ARGUMENT, "n must not be negative");
    if (n > 0 && !keys) return fail(JTK_ERR_INVALID_ARGUMENT, "keys is NULL");
    for (int64_t i = 0; i < n; i++)
        if (keys[i] == 0) return fail(JTK_ERR_INVALID_ARGUMENT, "a key of 0 cannot be in an n-gram set (0 is the empty slot)");
    if (n == 0) return JTK_OK;
    HIP_TRY(hipSetDevice(s->enc->device));
    int rc;
    if ((rc = ng_wait(s, s->own))) return rc;
    DevBuf tmp;                                                  // (staging that lives for this call)
    if ((rc = tmp.ensure((size_t)n * 8))) return rc;
    HIP_TRY(hipMemcpyAsync(tmp.p, keys, (size_t)n * 8, hipMemcpyHostToDevice, s->own));
    int64_t c = 0;
    HIP_TRY(hipMemcpyAsync(&c, s->hdr(), 8, hipMemcpyDeviceToHost, s->own));
    HIP_TRY(hipStreamSynchronize(s->own));
    if ((rc = ng_reserve(s, c, n, s->own))) return rc;
    jtk_launch_ngram_insert_keys((const uint64_t*)tmp.p, n, s->slots(), s->capacity, s->hdr(), s->own);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s->own));
    return ng_done(s, s->own);
}

int jtk_ngram_set_size(const jtk_ngram_set* s, int64_t* n_keys, int64_t* capacity) {
    if (!s) return fail(JTK_ERR_INVALID_ARGUMENT, "the n-gram set is NULL");
    HIP_TRY(hipSetDevice(s->enc->device));
    if (n_keys) {
        int rc;
        if ((rc = ng_wait(s, s->own))) return rc;
        HIP_TRY(hipMemcpyAsync(n_keys, s->hdr(), 8, hipMemcpyDeviceToHost, s->own));
        HIP_TRY(hipStreamSynchronize(s->own));
    }
    if (capacity) *capacity = s->capacity;
    return JTK_OK;
}

int jtk_ngram_set_keys(const jtk_ngram_set* s, uint64_t* keys, int64_t cap) {
    int64_t c = 0;
    int rc;
    if ((rc = jtk_ngram_set_size(s, &c, nullptr))) return rc;
    if (cap < c) return fail(JTK_ERR_INVALID_ARGUMENT, "keys has room for fewer than n_keys keys");
    if (c == 0) return JTK_OK;
    if (!keys) return fail(JTK_ERR_INVALID_ARGUMENT, "keys is NULL");
    std::vector<uint64_t> slots((size_t)s->capacity);
    HIP_TRY(hipMemcpyAsync(slots.data(), s->slots(), slots.size() * 8, hipMemcpyDeviceToHost, s->own));
    HIP_TRY(hipStreamSynchronize(s->own));
    int64_t n = 0;
    for (uint64_t k : slots)
        if (k && n < c) keys[n++] = k;
    if (n != c) return fail(JTK_ERR_HIP, "the n-gram table does not hold the number of keys it counts");
    return JTK_OK;
}

int jtk_batch_ngram_overlap(jtk_batch* b, const jtk_ngram_set* s, uint8_t* d_tok_flags, int32_t* d_n_hit, int32_t* d_n_covered,
                            int64_t* d_first_hit, void* stream_or_null) {
    if (!s) return fail(JTK_ERR_INVALID_ARGUMENT, "the n-gram set is NULL");
    int rc;
    if ((rc = need_encode(b, NEED_IDS))) return rc;
    if (b->enc != s->enc) return fail(JTK_ERR_INVALID_ARGUMENT, "the batch belongs to another encoding object than the n-gram set");
    if (((uintptr_t)d_n_hit & 3u) || ((uintptr_t)d_n_covered & 3u) || ((uintptr_t)d_first_hit & 7u))
        return fail(JTK_ERR_INVALID_ARGUMENT, "unaligned array (4-byte n_hit and n_covered, 8-byte first_hit)");
    HIP_TRY(hipSetDevice(b->enc->device));
    int64_t nt = 0;
    if ((rc = jtk_batch_result(b, &nt, nullptr, nullptr))) return rc;
    hipStream_t st = pick_stream(b, stream_or_null);
    if ((rc = ck_order(b, b->last_stream, st)) || (rc = ng_wait(s, st))) return rc;
    jtk_launch_ngram_overlap(ng_view(b, nt, s->p.ngram), s->p.seed, s->slots(), s->capacity, d_tok_flags, d_n_hit, d_n_covered, d_first_hit, st);
    HIP_TRY(hipGetLastError());
    return ng_done(s, st);
}

// ---- repeated n-grams inside a document (jtk_repeat.hip) ------------------------------------------------------------------
int jtk_batch_ngram_repeats(jtk_batch* b, const jtk_repeat_params* p, uint8_t* d_tok_flags, int32_t* d_n_repeat, int32_t* d_n_covered,
                            int32_t* d_top_count, int64_t* d_top_first, void* stream_or_null) {
    int rc;
    if ((rc = need_encode(b, NEED_IDS))) return rc;
    if (!p) return fail(JTK_ERR_INVALID_ARGUMENT, "params is NULL");
    if (!jtk_rp_params_ok(p->ngram, p->flags)) return fail(JTK_ERR_INVALID_ARGUMENT, "n-gram repeats: ngram 1..32, flags 0 or JTK_REPEAT_MARK_FIRST");
    if (((uintptr_t)d_n_repeat & 3u) || ((uintptr_t)d_n_covered & 3u) || ((uintptr_t)d_top_count & 3u) || ((uintptr_t)d_top_first & 7u))
        return fail(JTK_ERR_INVALID_ARGUMENT, "unaligned array (4-byte n_repeat, n_covered and top_count, 8-byte top_first)");
    HIP_TRY(hipSetDevice(b->enc->device));
    int64_t nt = 0;
    if ((rc = jtk_batch_result(b, &nt, nullptr, nullptr))) return rc;
    const int64_t nd = b->job_docs;
    const bool want_top = d_top_count || d_top_first;
    if (nd <= 0 || !(d_tok_flags || d_n_repeat || d_n_covered || want_top)) return JTK_OK;
    hipStream_t st = pick_stream(b, stream_or_null);
    if ((rc = ck_order(b, b->last_stream, st))) return rc;
    HIP_TRY(b->ev_rp.create());
    if (b->rp_queued) HIP_TRY(hipStreamWaitEvent(st, b->ev_rp, 0));
    // the plan: the groups come from the documents' token counts and statuses, read once
    if ((rc = b->h_rp.ensure((size_t)(nd + 1) * 8 + (size_t)nd * 4))) return rc;
    int64_t* const h_off = (int64_t*)b->h_rp.p;
    int32_t* const h_status = (int32_t*)(h_off + nd + 1);
    HIP_TRY(hipMemcpyAsync(h_off, b->tok_off.p, (size_t)(nd + 1) * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(h_status, b->status.p, (size_t)nd * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (h_off[0] != 0 || h_off[nd] > nt) return fail(JTK_ERR_HIP, "the token offsets of the last encode do not cover its tokens");
    for (int64_t d = 0; d < nd; d++)
        if (h_off[d + 1] - h_off[d] > JTK_RP_MAX_DOC_TOKENS) return fail(JTK_ERR_INVALID_ARGUMENT, "n-gram repeats: a document of 2^31 tokens or more");
    struct Group { int64_t lo, hi, m; };
    std::vector<Group> groups;
    int64_t m_max = 0;
    for (int64_t d0 = 0; d0 < nd;) {
        int64_t m = 0;
        const int64_t d1 = jtk_rp_group_end(h_off, h_status, nd, p->ngram, d0, b->rp_table_bytes, &m);
        if (h_off[d1] > h_off[d0]) groups.push_back({h_off[d0], h_off[d1], m});
        if (m > m_max) m_max = m;
        d0 = d1;
    }
    // everything that can fail for lack of memory comes before the first write; a table that grows is not in use any more
    const size_t table_bytes = m_max ? (size_t)jtk_rp_table_bytes(m_max) : 0, top_bytes = want_top ? (size_t)nd * 8 : 0;
    if ((table_bytes > b->rp_table.cap || top_bytes > b->rp_top.cap) && b->rp_queued) HIP_TRY(hipEventSynchronize(b->ev_rp));
    if ((rc = b->rp_table.ensure(table_bytes)) || (rc = b->rp_top.ensure(top_bytes))) return rc;
    uint64_t* const top = want_top ? (uint64_t*)b->rp_top.p : nullptr;
    const JtkMhView v = ng_view(b, nt, p->ngram);
    jtk_launch_repeat_preset(nd, d_n_repeat, d_n_covered, top, st);
    for (const Group& g : groups) {
        if (g.m == 0) {                                          // (tokens without an n-gram: documents shorter than n, refused ones)
            if (d_tok_flags) HIP_TRY(hipMemsetAsync(d_tok_flags + g.lo, 0, (size_t)(g.hi - g.lo), st));
            continue;
        }
        const int64_t cap = jtk_rp_capacity(g.m);
        const JtkRpTable t = jtk_rp_table_at(b->rp_table.p, cap);
        HIP_TRY(hipMemsetAsync(t.key, 0, (size_t)cap * 12, st));                // key | count
        HIP_TRY(hipMemsetAsync(t.first, 0xFF, (size_t)cap * 8, st));
        jtk_launch_repeat_group(v, p->seed, p->doc_index_base, p->flags, t, g.lo, g.hi, d_tok_flags, d_n_repeat, d_n_covered, top, st);
    }
    if (want_top) jtk_launch_repeat_top(nd, top, d_top_count, d_top_first, st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(b->ev_rp, st));
    b->rp_queued = true;
    return JTK_OK;
}

// ---- duplicate lines and paragraphs inside a document (jtk_lines.hip; the rule is jtk_lines_rules.h) -----------------------------
static_assert(sizeof(jtk_lines_params) == 24 && sizeof(jtk_lines_out) == sizeof(JtkLnOut), "the ABI's structs are the kernels'");
static int ln_check(const jtk_batch* b, const jtk_lines_params* p) {
    int rc;
    if ((rc = need_encode(b, NEED_TEXT_POS))) return rc;
    if (!p) return fail(JTK_ERR_INVALID_ARGUMENT, "params is NULL");
    if (!jtk_ln_params_ok(p->unit, p->flags))
        return fail(JTK_ERR_INVALID_ARGUMENT, "line units: unit JTK_LINES_LINE or JTK_LINES_PARAGRAPH, flags out of JTK_LINES_MARK_FIRST | JTK_LINES_TRIM");
    return JTK_OK;
}
static bool ln_same_list(const jtk_lines_params& a, const jtk_lines_params& b) {
    return a.unit == b.unit && ((a.flags ^ b.flags) & JTK_LINES_TRIM) == 0 && a.seed == b.seed && a.doc_index_base == b.doc_index_base;
}

// Where the parts of ln_scratch lie for a text of n_tiles tiles and nd documents, every part 8-byte aligned:
//   edge | ref        two bit planes, `plane` bytes each: one bit per byte of the tiles and the bit at n_bytes (k_ln_mark ORs whole
//                     32-bit words), read 16 bits per granule plus the first bit of the next granule: (granules + 2) * 2 bytes
//   8-byte per tile   sum_hash | tile_hash | tile_units | tile_chars
//   per document      doc_units | doc_chars | unit_off | char_off, nd + 1 entries each
//   hdr               2 entries (the unit count)
//   4-byte per tile   sum_word | sum_units | sum_chars | tile_cf | tile_cb
struct LnLayout {
    size_t tiles, plane, per_tile8, per_doc, hdr, per_tile4, total;
    int64_t nd;
    LnLayout(int64_t n_tiles, int64_t n_docs) : tiles((size_t)n_tiles), nd(n_docs) {
        plane = align_up((tiles * JTK_LN_TILE_GRANULES + 2) * 2, 16);
        per_tile8 = tiles * 8;
        per_doc = ((size_t)nd + 1) * 8;
        hdr = 16;
        per_tile4 = tiles * 4;
        total = 2 * plane + 4 * per_tile8 + 4 * per_doc + hdr + 5 * per_tile4 + 16;
    }
    void place(uint8_t* z, JtkLnWork* w) const {
        w->edge = (uint32_t*)z; w->ref = (uint32_t*)(z + plane);
        uint64_t* const t8 = (uint64_t*)(z + 2 * plane);
        w->sum_hash = t8; w->tile_hash = t8 + tiles; w->tile_units = (int64_t*)(t8 + 2 * tiles); w->tile_chars = (int64_t*)(t8 + 3 * tiles);
        int64_t* const d8 = (int64_t*)(t8 + 4 * tiles);
        w->doc_units = d8; w->doc_chars = d8 + (nd + 1); w->unit_off = d8 + 2 * (nd + 1); w->char_off = d8 + 3 * (nd + 1); w->hdr = d8 + 4 * (nd + 1);
        uint32_t* const t4 = (uint32_t*)(w->hdr + 2);
        w->sum_word = t4; w->sum_units = t4 + tiles; w->sum_chars = t4 + 2 * tiles; w->tile_cf = t4 + 3 * tiles; w->tile_cb = t4 + 4 * tiles;
    }
};

int jtk_batch_line_units(jtk_batch* b, const jtk_lines_params* p, void* stream_or_null, int64_t* n_units) {
    if (!n_units) return fail(JTK_ERR_INVALID_ARGUMENT, "n_units is NULL");
    *n_units = 0;
    int rc;
    if ((rc = ln_check(b, p))) return rc;
    HIP_TRY(hipSetDevice(b->enc->device));
    hipStream_t st = pick_stream(b, stream_or_null);
    const int64_t nd = b->job_docs, nb = b->job_bytes;
    if (nd <= 0) {                                               // (no document: no unit, and no array to hold)
        b->ln = JtkLnWork{};
        b->ln_p = *p; b->ln_stream = st; b->have_lines = true;
        return JTK_OK;
    }
    // behind the encode, behind the readers of the list that this one replaces, behind an earlier repeats pass
    if ((rc = ck_order(b, b->last_stream, st))) return rc;
    if (b->ln_stream && (rc = ck_order(b, b->ln_stream, st))) return rc;
    if (b->rp_queued) HIP_TRY(hipStreamWaitEvent(st, b->ev_rp, 0));
    b->have_lines = false;
    const LnLayout lay(jtk_lines_tiles(nb), nd);
    if (b->ln_scratch.cap < lay.total && b->rp_queued) HIP_TRY(hipEventSynchronize(b->ev_rp));      // (a buffer that grows is not in use any more)
    if ((rc = b->ln_scratch.ensure(lay.total)) || (rc = b->h_ln.ensure(lay.per_doc + 16))) return rc;
    uint8_t* const z = (uint8_t*)b->ln_scratch.p;
    JtkLnWork w{};
    w.text = b->job_text; w.doc_off = b->job_doc_off; w.status = (const int32_t*)b->status.p;
    w.n_bytes = nb; w.n_docs = nd; w.unit = p->unit; w.flags = p->flags;
    lay.place(z, &w);
    // count, the one wait, the list at its exact size, write
    HIP_TRY(hipMemsetAsync(z, 0, 2 * lay.plane, st));
    jtk_launch_lines_count(w, st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(b->h_ln.p, w.hdr, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const int64_t n = b->h_ln.p[0];
    if (n < 0 || n > nb) return fail(JTK_ERR_HIP, "the unit count of the text is outside [0, n_bytes]");
    if (b->ln_units.cap < (size_t)n * JTK_LN_UNIT_BYTES + 16 && b->rp_queued) HIP_TRY(hipEventSynchronize(b->ev_rp));
    if ((rc = b->ln_units.ensure((size_t)n * JTK_LN_UNIT_BYTES + 16))) return rc;
    int64_t* const u8 = (int64_t*)b->ln_units.p;
    w.n_units = n;
    w.u_begin = u8; w.u_end = u8 + n; w.u_k = (uint64_t*)(u8 + 2 * n); w.u_chars = u8 + 3 * n; w.u_pe = (uint64_t*)(u8 + 4 * n); w.u_ce = u8 + 5 * n;
    jtk_launch_lines_write(w, p->seed, p->doc_index_base, st);
    HIP_TRY(hipGetLastError());
    b->ln = w; b->ln_p = *p; b->ln_stream = st; b->have_lines = true;
    *n_units = n;
    return JTK_OK;
}

int jtk_batch_line_repeats(jtk_batch* b, const jtk_lines_params* p, const jtk_lines_out* out, void* stream_or_null) {
    int rc;
    if ((rc = ln_check(b, p))) return rc;
    if (!out) return fail(JTK_ERR_INVALID_ARGUMENT, "out is NULL");
    if (!b->have_lines || !ln_same_list(b->ln_p, *p))
        return fail(JTK_ERR_INVALID_ARGUMENT, "no unit list of the last encode for these parameters: call jtk_batch_line_units first");
    if (((uintptr_t)out->n_dup & 3u) || ((uintptr_t)out->top_count & 3u) || ((uintptr_t)out->unit_begin & 7u) || ((uintptr_t)out->unit_end & 7u) ||
        ((uintptr_t)out->unit_off & 7u) || ((uintptr_t)out->dup_bytes & 7u) || ((uintptr_t)out->dup_chars & 7u) || ((uintptr_t)out->unit_bytes & 7u) ||
        ((uintptr_t)out->unit_chars & 7u) || ((uintptr_t)out->doc_chars & 7u) || ((uintptr_t)out->top_first & 7u))
        return fail(JTK_ERR_INVALID_ARGUMENT, "unaligned array (4-byte n_dup and top_count, 8-byte int64 arrays)");
    const int64_t nd = b->job_docs;
    if (nd <= 0) return JTK_OK;
    HIP_TRY(hipSetDevice(b->enc->device));
    hipStream_t st = pick_stream(b, stream_or_null);
    if ((rc = ck_order(b, b->ln_stream, st))) return rc;
    HIP_TRY(b->ev_rp.create());
    if (b->rp_queued) HIP_TRY(hipStreamWaitEvent(st, b->ev_rp, 0));
    // the plan: the groups come from the documents' unit counts, read once
    const JtkLnWork& w = b->ln;
    int64_t* const h_off = b->h_ln.p;
    HIP_TRY(hipMemcpyAsync(h_off, w.unit_off, (size_t)(nd + 1) * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (h_off[0] != 0 || h_off[nd] != w.n_units) return fail(JTK_ERR_HIP, "the unit offsets of the list do not cover its units");
    for (int64_t d = 0; d < nd; d++)
        if (h_off[d + 1] - h_off[d] > JTK_LN_MAX_DOC_UNITS) return fail(JTK_ERR_INVALID_ARGUMENT, "line repeats: a document of 2^31 units or more");
    struct Group { int64_t lo, hi; };
    std::vector<Group> groups;
    int64_t m_max = 0;
    for (int64_t d0 = 0; d0 < nd;) {
        int64_t m = 0;
        const int64_t d1 = jtk_ln_group_end(h_off, nd, d0, b->rp_table_bytes, &m);
        if (m > 0) groups.push_back({h_off[d0], h_off[d1]});
        if (m > m_max) m_max = m;
        d0 = d1;
    }
    // everything that can fail for lack of memory comes before the first write; a table that grows is not in use any more
    const bool want_top = out->top_count || out->top_first;
    const size_t table_bytes = m_max ? (size_t)jtk_rp_table_bytes(m_max) : 0, top_bytes = want_top ? (size_t)nd * 8 : 0;
    if ((table_bytes > b->rp_table.cap || top_bytes > b->rp_top.cap) && b->rp_queued) HIP_TRY(hipEventSynchronize(b->ev_rp));
    if ((rc = b->rp_table.ensure(table_bytes)) || (rc = b->rp_top.ensure(top_bytes))) return rc;
    uint64_t* const top = want_top ? (uint64_t*)b->rp_top.p : nullptr;
    JtkLnOut o;
    memcpy(&o, out, sizeof o);
    jtk_launch_lines_preset(w, o, top, st);
    if (w.n_units > 0) {
        if (o.unit_begin) HIP_TRY(hipMemcpyAsync(o.unit_begin, w.u_begin, (size_t)w.n_units * 8, hipMemcpyDeviceToDevice, st));
        if (o.unit_end) HIP_TRY(hipMemcpyAsync(o.unit_end, w.u_end, (size_t)w.n_units * 8, hipMemcpyDeviceToDevice, st));
    }
    const bool passes = o.unit_flags || o.n_dup || o.dup_bytes || o.dup_chars || o.unit_bytes || o.unit_chars || want_top;
    for (const Group& g : groups) {
        if (!passes) break;
        const int64_t cap = jtk_rp_capacity(g.hi - g.lo);
        const JtkRpTable t = jtk_rp_table_at(b->rp_table.p, cap);
        HIP_TRY(hipMemsetAsync(t.key, 0, (size_t)cap * 12, st));                // key | count
        HIP_TRY(hipMemsetAsync(t.first, 0xFF, (size_t)cap * 8, st));
        jtk_launch_lines_group(w, p->flags, t, g.lo, g.hi, o, top, st);
    }
    if (want_top) jtk_launch_repeat_top(nd, top, o.top_count, o.top_first, st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(b->ev_rp, st));
    b->rp_queued = true;
    b->ln_stream = st;
    return JTK_OK;
}

int jtk_batch_token_offsets(jtk_batch* b, int64_t* d_byte_pos, void* stream_or_null) {
    int rc;
    if ((rc = need_encode(b, NEED_IDS | NEED_TEXT_ORDER))) return rc;
    HIP_TRY(hipSetDevice(b->enc->device));
    hipStream_t s = pick_stream(b, stream_or_null);
    if ((rc = ck_byte_scan(b, s))) return rc;
    if (b->ck.n_tok > 0 && !d_byte_pos) return fail(JTK_ERR_INVALID_ARGUMENT, "d_byte_pos is NULL");
    jtk_launch_token_offsets(b->ck, d_byte_pos, s);
    HIP_TRY(hipGetLastError());
    return JTK_OK;
}

int jtk_batch_token_cut_levels(jtk_batch* b, uint32_t prefer, uint8_t* d_level, void* stream_or_null) {
    int rc;
    if ((rc = need_encode(b, NEED_IDS))) return rc;
    if (prefer & ~15u) return fail(JTK_ERR_INVALID_ARGUMENT, "prefer holds bits outside JTK_CUT_WORD | _SENTENCE | _LINE | _PARAGRAPH");
    HIP_TRY(hipSetDevice(b->enc->device));
    int64_t nt = 0;
    if ((rc = jtk_batch_result(b, &nt, nullptr, nullptr))) return rc;
    if (nt > 0 && !d_level) return fail(JTK_ERR_INVALID_ARGUMENT, "d_level is NULL");
    hipStream_t s = pick_stream(b, stream_or_null);
    if ((rc = ck_order(b, b->last_stream, s))) return rc;
    // (a view of the last encode of its own: the batch's chunk result stays as it is)
    JtkChunkWork w{};
    w.tokens = (const int32_t*)b->tokens.p; w.tok_off = (const int64_t*)b->tok_off.p; w.n_docs = b->job_docs;
    w.tab_off = (const uint32_t*)b->enc->dec_off.p; w.n_ids_table = b->enc->n_ids_table;
    if (nt > 0) jtk_launch_cut_levels(w, (const uint8_t*)b->enc->dec_blob.p, prefer, d_level, s);
    HIP_TRY(hipGetLastError());
    return JTK_OK;
}

int jtk_batch_chunk_prefer(jtk_batch* b, int64_t chunk_tokens, int64_t overlap, int64_t min_tokens, uint32_t prefer,
                           void* stream_or_null, int64_t* n_chunks) {
    if (!b || !n_chunks) return fail(JTK_ERR_INVALID_ARGUMENT, "bad arguments");
    *n_chunks = 0;
    int rc;
    if ((rc = need_encode(b, NEED_IDS | NEED_TEXT_ORDER))) return rc;
    if (chunk_tokens < 1 || chunk_tokens > INT32_MAX) return fail(JTK_ERR_INVALID_ARGUMENT, "chunk_tokens must be in [1, 2^31 - 1]");
    if (overlap < 0 || overlap >= chunk_tokens) return fail(JTK_ERR_INVALID_ARGUMENT, "overlap must be in [0, chunk_tokens)");
    if (min_tokens < 1 || min_tokens > chunk_tokens) return fail(JTK_ERR_INVALID_ARGUMENT, "min_tokens must be in [1, chunk_tokens]");
    if (prefer & ~15u) return fail(JTK_ERR_INVALID_ARGUMENT, "prefer holds bits outside JTK_CUT_WORD | _SENTENCE | _LINE | _PARAGRAPH");
    HIP_TRY(hipSetDevice(b->enc->device));
    hipStream_t s = pick_stream(b, stream_or_null);
    int64_t nt = 0;
    if ((rc = jtk_batch_result(b, &nt, nullptr, nullptr))) return rc;      // (the plane is sized by the token count)
    b->have_chunk = false;
    b->have_tiles = false;
    if ((rc = ck_order(b, b->last_stream, s)) || (rc = ck_setup(b)) || (rc = b->h_ck.ensure(32)) ||
        (rc = b->ck_plane.ensure((size_t)nt + 16))) return rc;
    JtkChunkPreferWork p{};
    JtkChunkWork& w = b->ck;
    w.N = chunk_tokens; w.overlap = overlap;
    p.plane = (const uint8_t*)b->ck_plane.p; p.min_tokens = min_tokens; p.prefer = prefer;
    // plane, count per document, scan; the wait: (chunks, tokens)
    HIP_TRY(hipMemsetAsync(w.hdr, 0, 32, s));
    if (nt > 0) jtk_launch_cut_levels(w, (const uint8_t*)b->enc->dec_blob.p, prefer, (uint8_t*)b->ck_plane.p, s);
    p.w = w;
    jtk_launch_chunk_prefer_count(p, s);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(b->h_ck.p, w.hdr, 16, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    const int64_t nc = b->h_ck.p[0];
    if ((rc = ck_tiles(b, nt, s)) || (rc = ck_records(b, nc, &p.end_level))) return rc;
    p.w = w;
    jtk_launch_chunk_prefer_write(p, s);
    HIP_TRY(hipGetLastError());
    b->ck_end_level = p.end_level;
    b->have_chunk = true;
    b->ck_stream = s;
    *n_chunks = nc;
    return JTK_OK;
}

int jtk_batch_chunk_levels(jtk_batch* b, uint8_t* end_level_or_null, const uint8_t** d_end_level_or_null) {
    if (!b || !b->have_chunk) return fail(JTK_ERR_INVALID_ARGUMENT, "jtk_batch_chunk_prefer has not run on the last encode of this batch");
    if (!b->ck_end_level) return fail(JTK_ERR_INVALID_ARGUMENT, "the last chunk call was jtk_batch_chunk: it has no levels");
    if (d_end_level_or_null) *d_end_level_or_null = b->ck_end_level;
    if (end_level_or_null && b->ck.n_chunks > 0) {
        HIP_TRY(hipSetDevice(b->enc->device));
        HIP_TRY(hipStreamSynchronize(b->ck_stream));
        HIP_TRY(hipMemcpy(end_level_or_null, b->ck_end_level, (size_t)b->ck.n_chunks, hipMemcpyDeviceToHost));
    }
    return JTK_OK;
}


// ---- packed rows of the last encode (jtk_pack.hip) ---------------------------------------------------------------------
static bool pk_known_id(const jtk_encoding* enc, int32_t id) {
    const JtkHostTables& h = enc->host;
    if ((uint32_t)id <= h.max_id && (size_t)id < h.id_present.size() && h.id_present[(size_t)id]) return true;
    for (const auto& sp : h.specials) if (sp.second == id) return true;
    return false;
}

int jtk_batch_pack(jtk_batch* b, int64_t seq_len, int32_t sep_id, uint32_t flags, void* stream_or_null,
                   int64_t* n_rows, int64_t* n_segments, int32_t* max_seqlen) {
    if (!b || !n_rows || !n_segments || !max_seqlen) return fail(JTK_ERR_INVALID_ARGUMENT, "bad arguments");
    *n_rows = 0; *n_segments = 0; *max_seqlen = 0;
    int rc;
    if ((rc = need_encode(b, NEED_IDS))) return rc;
    if (seq_len < 1) return fail(JTK_ERR_INVALID_ARGUMENT, "seq_len must be at least 1");
    if (seq_len > INT32_MAX)
        return fail(JTK_ERR_INVALID_ARGUMENT, "seq_len must be below 2^31: cu_seqlens (int32) indexes the cells of the rows");
    if (sep_id < -1) return fail(JTK_ERR_INVALID_ARGUMENT, "sep_id must be -1 (no separator) or a token id");
    if (sep_id >= 0 && !pk_known_id(b->enc, sep_id))
        return fail(JTK_ERR_INVALID_ARGUMENT, "sep_id " + std::to_string(sep_id) + " is neither a rank id nor a special id of the encoding");
    if (flags & ~(uint32_t)(JTK_PACK_WHOLE_DOCS | JTK_PACK_SEP_FIRST | JTK_PACK_DROP_LAST))
        return fail(JTK_ERR_INVALID_ARGUMENT, "flags: JTK_PACK_WHOLE_DOCS, JTK_PACK_SEP_FIRST, JTK_PACK_DROP_LAST");
    const bool whole = (flags & JTK_PACK_WHOLE_DOCS) != 0, drop = (flags & JTK_PACK_DROP_LAST) != 0;
    if (whole && drop) return fail(JTK_ERR_INVALID_ARGUMENT, "JTK_PACK_DROP_LAST does not apply with JTK_PACK_WHOLE_DOCS (every row is padded)");
    const int64_t n = b->job_docs;
    if (n >= INT32_MAX) return fail(JTK_ERR_INVALID_ARGUMENT, "too many documents to pack in one call (2^31 - 1 at most)");
    HIP_TRY(hipSetDevice(b->enc->device));
    hipStream_t s = pick_stream(b, stream_or_null);
    b->have_pack = false;                                              // (this call replaces its own result)
    int K = 1;
    while (K < 62 && ((int64_t)1 << K) <= n) K++;                      // 2^K > n >= the number of groups
    // scratch: hdr[4] | P | SEG | RS [n + 1] | flag [n] | up [K][n + 1]
    const size_t m = (size_t)n + 1, o_flag = 32 + 3 * m * 8, o_up = align_up(o_flag + m, 16);
    const size_t bytes = whole ? o_up + (size_t)K * m * 4 : o_flag;
    if ((rc = b->pk_scratch.ensure(bytes)) || (rc = b->h_pk.ensure(32)) ||
        (rc = ck_order(b, b->last_stream, s)))
        return rc;
    JtkPackWork& w = b->pk;
    w = JtkPackWork{};
    uint8_t* base = (uint8_t*)b->pk_scratch.p;
    w.hdr = (int64_t*)base;
    w.P = (int64_t*)(base + 32);
    w.SEG = w.P + m;
    w.RS = w.SEG + m;
    w.flag = base + o_flag;
    w.up = whole ? (int32_t*)(base + o_up) : nullptr;
    w.K = K;
    w.drop_last = drop;
    w.status = (const int32_t*)b->status.p;
    JtkPackView& v = w.v;
    v.tokens = (const int32_t*)b->tokens.p; v.tok_off = (const int64_t*)b->tok_off.p;
    v.P = w.P; v.SEG = w.SEG; v.RS = w.RS; v.flag = w.flag; v.nxt = w.up;
    v.n = n; v.L = seq_len; v.sep_id = sep_id; v.sep_first = (flags & JTK_PACK_SEP_FIRST) != 0 && sep_id >= 0; v.whole = whole;
    // plan; the one wait: hdr
    HIP_TRY(hipMemsetAsync(w.hdr, 0, 32, s));
    jtk_launch_pack_plan(w, s);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(b->h_pk.p, w.hdr, 32, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    const int64_t S = b->h_pk.p[0];
    int64_t rows, segs, longest = b->h_pk.p[3];
    if (whole) {
        rows = b->h_pk.p[2];
        segs = b->h_pk.p[1];
    } else {
        rows = jtk_pack_concat_rows(S, seq_len, drop);
        const int64_t pad = rows > 0 ? rows * seq_len - S : 0;        // (the last row's pad; never with DROP_LAST)
        segs = b->h_pk.p[1] + (pad > 0 ? 1 : 0);
        if (pad > longest) longest = pad;
    }
    if (rows > INT32_MAX / seq_len)
        return fail(JTK_ERR_INVALID_ARGUMENT, "the rows would hold " + std::to_string(rows) + " x " + std::to_string(seq_len) +
                                                  " cells, more than cu_seqlens (int32) can index (2^31 - 1): split the batch");
    w.n_rows = rows;
    w.n_seg = segs;
    b->have_pack = true;
    b->pk_stream = s;
    *n_rows = rows; *n_segments = segs; *max_seqlen = (int32_t)longest;
    return JTK_OK;
}

int jtk_batch_pack_write(jtk_batch* b, int32_t pad_id, int32_t* d_rows, int32_t* d_positions, int32_t* d_cu_seqlens,
                         int64_t* d_seg_doc, void* stream_or_null) {
    if (!b || !b->have_pack) return fail(JTK_ERR_INVALID_ARGUMENT, "jtk_batch_pack has not run on the last encode of this batch");
    if (b->pk.n_rows > 0 && !d_rows) return fail(JTK_ERR_INVALID_ARGUMENT, "d_rows is NULL");
    if (((uintptr_t)d_rows & 3u) || ((uintptr_t)d_positions & 3u) || ((uintptr_t)d_cu_seqlens & 3u) || ((uintptr_t)d_seg_doc & 7u))
        return fail(JTK_ERR_INVALID_ARGUMENT, "unaligned output (4-byte int32, 8-byte int64 arrays)");
    HIP_TRY(hipSetDevice(b->enc->device));
    hipStream_t s = pick_stream(b, stream_or_null);
    int rc;
    if ((rc = ck_order(b, b->pk_stream, s))) return rc;
    jtk_launch_pack_write(b->pk, pad_id, d_rows, d_positions, d_cu_seqlens, d_seg_doc, s);
    HIP_TRY(hipGetLastError());
    return JTK_OK;
}

int jtk_batch_pack_fetch(jtk_batch* b, int32_t pad_id, int32_t* rows, int32_t* positions, int32_t* cu_seqlens, int64_t* seg_doc) {
    if (!b || !b->have_pack) return fail(JTK_ERR_INVALID_ARGUMENT, "jtk_batch_pack has not run on the last encode of this batch");
    const size_t cells = (size_t)(b->pk.n_rows * b->pk.v.L), ns = (size_t)b->pk.n_seg;
    // device staging: rows | positions | cu_seqlens | seg_doc
    const size_t o_pos = align_up(cells * 4, 16), o_cu = o_pos + align_up(cells * 4, 16), o_sd = align_up(o_cu + (ns + 1) * 4, 16);
    HIP_TRY(hipSetDevice(b->enc->device));
    DevBuf tmp;                                                  // (staging that lives for this call)
    int rc;
    if ((rc = tmp.ensure(o_sd + ns * 8 + 16))) return rc;
    uint8_t* p = (uint8_t*)tmp.p;
    if ((rc = jtk_batch_pack_write(b, pad_id, (int32_t*)p, positions ? (int32_t*)(p + o_pos) : nullptr, (int32_t*)(p + o_cu),
                                   seg_doc ? (int64_t*)(p + o_sd) : nullptr, b->pk_stream)))
        return rc;
    HIP_TRY(hipStreamSynchronize(b->pk_stream));
    if (rows && cells) HIP_TRY(hipMemcpy(rows, p, cells * 4, hipMemcpyDeviceToHost));
    if (positions && cells) HIP_TRY(hipMemcpy(positions, p + o_pos, cells * 4, hipMemcpyDeviceToHost));
    if (cu_seqlens) HIP_TRY(hipMemcpy(cu_seqlens, p + o_cu, (ns + 1) * 4, hipMemcpyDeviceToHost));
    if (seg_doc && ns) HIP_TRY(hipMemcpy(seg_doc, p + o_sd, ns * 8, hipMemcpyDeviceToHost));
    return JTK_OK;
}


// ---- labels of the packed rows from byte spans (jtk_label.hip) ---------------------------------------------------------
int jtk_batch_token_spans(jtk_batch* b, const int64_t* d_span_begin, const int64_t* d_span_end, int64_t n_spans, int rule,
                          int32_t* d_tok_span, void* stream_or_null) {
    int rc;
    if ((rc = need_encode(b, NEED_IDS | NEED_TEXT_POS))) return rc;
    if (rule != JTK_SPAN_WHOLE && rule != JTK_SPAN_START && rule != JTK_SPAN_ANY)
        return fail(JTK_ERR_INVALID_ARGUMENT, "rule: JTK_SPAN_WHOLE, JTK_SPAN_START or JTK_SPAN_ANY");
    if (n_spans < 0 || n_spans > INT32_MAX) return fail(JTK_ERR_INVALID_ARGUMENT, "n_spans must be in [0, 2^31 - 1]");
    if (n_spans > 0 && (!d_span_begin || !d_span_end)) return fail(JTK_ERR_INVALID_ARGUMENT, "d_span_begin or d_span_end is NULL");
    if (((uintptr_t)d_span_begin & 7u) || ((uintptr_t)d_span_end & 7u) || ((uintptr_t)d_tok_span & 3u))
        return fail(JTK_ERR_INVALID_ARGUMENT, "unaligned array (8-byte int64 spans, 4-byte int32 tok_span)");
    HIP_TRY(hipSetDevice(b->enc->device));
    hipStream_t s = pick_stream(b, stream_or_null);
    if ((rc = ck_byte_scan(b, s))) return rc;
    if (b->ck.n_tok > 0 && !d_tok_span) return fail(JTK_ERR_INVALID_ARGUMENT, "d_tok_span is NULL");
    jtk_launch_label_spans(b->ck, d_span_begin, d_span_end, n_spans, rule, d_tok_span, s);
    HIP_TRY(hipGetLastError());
    return JTK_OK;
}

int jtk_batch_pack_labels(jtk_batch* b, const int32_t* d_tok_span_or_null, int32_t ignore_index, uint32_t flags,
                          int32_t* d_labels, void* stream_or_null) {
    if (!b || !b->have_pack) return fail(JTK_ERR_INVALID_ARGUMENT, "jtk_batch_pack has not run on the last encode of this batch");
    if (flags & ~(uint32_t)(JTK_LABEL_SHIFT | JTK_LABEL_SEP)) return fail(JTK_ERR_INVALID_ARGUMENT, "flags: JTK_LABEL_SHIFT, JTK_LABEL_SEP");
    if (b->pk.n_rows > 0 && !d_labels) return fail(JTK_ERR_INVALID_ARGUMENT, "d_labels is NULL");
    if (((uintptr_t)d_tok_span_or_null & 3u) || ((uintptr_t)d_labels & 3u)) return fail(JTK_ERR_INVALID_ARGUMENT, "unaligned array (4-byte int32)");
    HIP_TRY(hipSetDevice(b->enc->device));
    hipStream_t s = pick_stream(b, stream_or_null);
    int rc;
    if ((rc = ck_order(b, b->pk_stream, s))) return rc;
    JtkLabelView lv;
    lv.tok_span = d_tok_span_or_null; lv.ignore_index = ignore_index; lv.label_sep = (flags & JTK_LABEL_SEP) != 0;
    jtk_launch_label_pack(b->pk, lv, (flags & JTK_LABEL_SHIFT) != 0, d_labels, s);
    HIP_TRY(hipGetLastError());
    return JTK_OK;
}

int jtk_batch_pack_labels_fetch(jtk_batch* b, const int32_t* d_tok_span_or_null, int32_t ignore_index, uint32_t flags,
                                int32_t* labels) {
    if (!b || !b->have_pack) return fail(JTK_ERR_INVALID_ARGUMENT, "jtk_batch_pack has not run on the last encode of this batch");
    const size_t cells = (size_t)(b->pk.n_rows * b->pk.v.L);
    if (cells && !labels) return fail(JTK_ERR_INVALID_ARGUMENT, "labels is NULL");
    HIP_TRY(hipSetDevice(b->enc->device));
    DevBuf tmp;                                                  // (staging that lives for this call)
    int rc;
    if ((rc = tmp.ensure(cells * 4 + 16)) ||
        (rc = jtk_batch_pack_labels(b, d_tok_span_or_null, ignore_index, flags, (int32_t*)tmp.p, b->pk_stream)))
        return rc;
    HIP_TRY(hipStreamSynchronize(b->pk_stream));
    if (cells) HIP_TRY(hipMemcpy(labels, tmp.p, cells * 4, hipMemcpyDeviceToHost));
    return JTK_OK;
}


// ---- character positions of the last encode's text (jtk_charpos.hip; the rule is jtk_charpos_rules.h) -----------------------
static_assert(JTK_UNIT_BYTE == JTK_CP_UNIT_BYTE && JTK_UNIT_UTF16 == JTK_CP_UNIT_UTF16 && JTK_UNIT_CODEPOINT == JTK_CP_UNIT_CODEPOINT &&
              JTK_CHAR_FLOOR == JTK_CP_FLOOR && JTK_CHAR_CEIL == JTK_CP_CEIL, "the rule header's values are the ABI's");
static int cp_check(jtk_batch* b, int unit, unsigned also = 0) {
    int rc;
    if ((rc = need_encode(b, NEED_TEXT_POS | also))) return rc;
    if (!jtk_cp_valid_unit(unit)) return fail(JTK_ERR_INVALID_ARGUMENT, "unit: JTK_UNIT_BYTE, JTK_UNIT_UTF16 or JTK_UNIT_CODEPOINT");
    return JTK_OK;
}

// the index of the last encode's text for `unit`, ready on s: the cached one, or a new build behind the encode
static int cp_index(jtk_batch* b, int unit, hipStream_t s) {
    int rc;
    if (b->cp_unit == unit) {
        if ((rc = ck_order(b, b->cp_stream, s))) return rc;
        b->cp_stream = s;
        return JTK_OK;
    }
    if ((rc = ck_order(b, b->last_stream, s))) return rc;
    if (b->cp_stream && (rc = ck_order(b, b->cp_stream, s))) return rc;       // (readers of the index that this one replaces)
    b->cp_unit = -1;
    const int64_t n_bytes = b->job_bytes, nd = b->job_docs;
    const int64_t n_sup = (n_bytes + JTK_CP_SUPER - 1) / JTK_CP_SUPER;
    const size_t o_dunit = ((size_t)n_sup + 1) * 8, o_cnt = o_dunit + ((size_t)nd + 1) * 8, o_sub = align_up(o_cnt + (size_t)n_sup * 4 + 4, 16);
    if ((rc = b->cp_buf.ensure(o_sub + (size_t)n_sup * JTK_CP_BLOCKS_PER_SUPER * 2 + 16))) return rc;
    uint8_t* z = (uint8_t*)b->cp_buf.p;
    JtkCharIndex& ix = b->cp;
    ix.text = b->job_text; ix.n_bytes = n_bytes; ix.n_sup = n_sup; ix.unit = unit;
    ix.sup = (const int64_t*)z; ix.sub = (const uint16_t*)(z + o_sub);
    b->cp_dunit = (int64_t*)(z + o_dunit);
    jtk_launch_charpos_build(ix, (uint32_t*)(z + o_cnt), (int64_t*)z, (uint16_t*)(z + o_sub), b->job_doc_off, nd, b->cp_dunit, s);
    HIP_TRY(hipGetLastError());
    b->cp_unit = unit;
    b->cp_stream = s;
    return JTK_OK;
}

int jtk_batch_char_index(jtk_batch* b, int unit, int64_t* d_doc_units_or_null, void* stream_or_null) {
    int rc;
    if ((rc = cp_check(b, unit))) return rc;
    if ((uintptr_t)d_doc_units_or_null & 7u) return fail(JTK_ERR_INVALID_ARGUMENT, "unaligned array (8-byte int64)");
    if (b->job_docs == 0) return JTK_OK;
    HIP_TRY(hipSetDevice(b->enc->device));
    hipStream_t s = pick_stream(b, stream_or_null);
    if ((rc = cp_index(b, unit, s))) return rc;
    if (d_doc_units_or_null) {
        jtk_launch_charpos_doc_units(b->job_doc_off, b->cp_dunit, b->job_docs, d_doc_units_or_null, s);
        HIP_TRY(hipGetLastError());
    }
    return JTK_OK;
}

int jtk_batch_char_positions(jtk_batch* b, int unit, int round, const int64_t* d_doc_or_null, const int64_t* d_byte_pos, int64_t n,
                             int64_t* d_char_pos, void* stream_or_null) {
    int rc;
    if ((rc = cp_check(b, unit))) return rc;
    if (!jtk_cp_valid_round(round)) return fail(JTK_ERR_INVALID_ARGUMENT, "round: JTK_CHAR_FLOOR or JTK_CHAR_CEIL");
    if (n < 0) return fail(JTK_ERR_INVALID_ARGUMENT, "n must not be negative");
    if (n > 0 && (!d_byte_pos || !d_char_pos)) return fail(JTK_ERR_INVALID_ARGUMENT, "d_byte_pos or d_char_pos is NULL");
    if (((uintptr_t)d_doc_or_null & 7u) || ((uintptr_t)d_byte_pos & 7u) || ((uintptr_t)d_char_pos & 7u))
        return fail(JTK_ERR_INVALID_ARGUMENT, "unaligned array (8-byte int64)");
    if (n == 0) return JTK_OK;
    HIP_TRY(hipSetDevice(b->enc->device));
    hipStream_t s = pick_stream(b, stream_or_null);
    if ((rc = cp_index(b, unit, s))) return rc;
    jtk_launch_charpos_rank(b->cp, b->job_doc_off, b->cp_dunit, b->job_docs, round, d_doc_or_null, d_byte_pos, n, d_char_pos, s);
    HIP_TRY(hipGetLastError());
    return JTK_OK;
}

int jtk_batch_byte_positions(jtk_batch* b, int unit, const int64_t* d_doc, const int64_t* d_char_pos, int64_t n, int64_t* d_byte_pos,
                             void* stream_or_null) {
    int rc;
    if ((rc = cp_check(b, unit))) return rc;
    if (n < 0) return fail(JTK_ERR_INVALID_ARGUMENT, "n must not be negative");
    if (n > 0 && (!d_doc || !d_char_pos || !d_byte_pos)) return fail(JTK_ERR_INVALID_ARGUMENT, "d_doc, d_char_pos or d_byte_pos is NULL");
    if (((uintptr_t)d_doc & 7u) || ((uintptr_t)d_char_pos & 7u) || ((uintptr_t)d_byte_pos & 7u))
        return fail(JTK_ERR_INVALID_ARGUMENT, "unaligned array (8-byte int64)");
    if (n == 0) return JTK_OK;
    HIP_TRY(hipSetDevice(b->enc->device));
    hipStream_t s = pick_stream(b, stream_or_null);
    if ((rc = cp_index(b, unit, s))) return rc;
    jtk_launch_charpos_select(b->cp, b->job_doc_off, b->cp_dunit, b->job_docs, d_doc, d_char_pos, n, d_byte_pos, s);
    HIP_TRY(hipGetLastError());
    return JTK_OK;
}

int jtk_batch_token_char_offsets(jtk_batch* b, int unit, int64_t* d_begin, int64_t* d_end_or_null, void* stream_or_null) {
    int rc;
    if ((rc = cp_check(b, unit, NEED_IDS))) return rc;
    if (((uintptr_t)d_begin & 7u) || ((uintptr_t)d_end_or_null & 7u)) return fail(JTK_ERR_INVALID_ARGUMENT, "unaligned array (8-byte int64)");
    HIP_TRY(hipSetDevice(b->enc->device));
    hipStream_t s = pick_stream(b, stream_or_null);
    if ((rc = ck_byte_scan(b, s))) return rc;
    if (b->ck.n_tok == 0) return JTK_OK;
    if (!d_begin) return fail(JTK_ERR_INVALID_ARGUMENT, "d_begin is NULL");
    if ((rc = cp_index(b, unit, s))) return rc;
    jtk_launch_charpos_tokens(b->ck, b->cp, b->cp_dunit, d_begin, d_end_or_null, s);
    HIP_TRY(hipGetLastError());
    return JTK_OK;
}

// ---- UTF-16 in and out (jtk_utf16.hip; the rules are jtk_utf16_rules.h) -------------------------------------------------------
// E into u16_enc_* (for_encode: the text of a new encode, so the last encode's result goes before a byte of it is written) or
// u16_tx_* of the batch: count, the one wait (size of the output, offsets check), write
static int u16_transcode(jtk_batch* b, bool for_encode, const uint16_t* d_units, const int64_t* d_unit_off, int64_t n_docs,
                         int64_t n_units, void* stream_or_null, int64_t* n_bytes) {
    if (!b || n_docs < 0 || n_units < 0 || (n_units > 0 && !d_units) || !d_unit_off) return fail(JTK_ERR_INVALID_ARGUMENT, "bad arguments");
    if ((uintptr_t)d_units & 1u) return fail(JTK_ERR_INVALID_ARGUMENT, "d_units must be 2-byte aligned");
    if ((uintptr_t)d_unit_off & 7u) return fail(JTK_ERR_INVALID_ARGUMENT, "unaligned array (8-byte int64)");
    if (n_units >= (int64_t)1 << 35) return fail(JTK_ERR_INVALID_ARGUMENT, "batch too large (32 Gi units per call at most)");
    HIP_TRY(hipSetDevice(b->enc->device));
    if (for_encode) drop_encode_result(b);
    DevBuf& text = for_encode ? b->u16_enc_text : b->u16_tx_text;
    DevBuf& off = for_encode ? b->u16_enc_off : b->u16_tx_off;
    hipStream_t s = pick_stream(b, stream_or_null);
    JtkU16EncWork w{};
    w.units = d_units; w.n_units = n_units; w.unit_off = d_unit_off; w.n_docs = n_docs;
    w.n_tiles = (n_units + JTK_U16_E_TILE - 1) / JTK_U16_E_TILE;
    const size_t nt = (size_t)w.n_tiles;
    const size_t o_cnt = 16 + (nt + 1) * 8, o_sub = o_cnt + align_up(nt * 4 + 4, 16);
    int rc;
    if ((rc = b->u16_scratch.ensure(o_sub + nt * JTK_U16_LANES * 2 + 16)) || (rc = off.ensure(((size_t)n_docs + 1) * 8))) return rc;
    uint8_t* z = (uint8_t*)b->u16_scratch.p;
    w.hdr = (int64_t*)z; w.tile_off = (int64_t*)(z + 16); w.tile_cnt = (uint32_t*)(z + o_cnt); w.sub = (uint16_t*)(z + o_sub);
    w.doc_off = (int64_t*)off.p;
    const bool aligned = ((uintptr_t)d_units & 15u) == 0;
    b->have_u16 = false;
    if (b->u16_stream && (rc = ck_order(b, b->u16_stream, s))) return rc;    // (the last write pass still reads sub and tile_off)
    b->u16_stream = s;
    HIP_TRY(hipMemsetAsync(w.hdr, 0, 16, s));
    jtk_launch_u16_enc_count(w, aligned, s);
    HIP_TRY(hipGetLastError());
    int64_t hdr[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(hdr, w.hdr, 16, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (hdr[1] != 0) return fail(JTK_ERR_INVALID_ARGUMENT, "unit_off must start at or above 0, never decrease and end at or below n_units");
    if ((rc = text.ensure((size_t)hdr[0] + 64))) return rc;
    w.out = (uint8_t*)text.p;
    jtk_launch_u16_enc_write(w, aligned, s);
    HIP_TRY(hipGetLastError());
    b->u16_last_text = w.out; b->u16_last_off = w.doc_off; b->u16_last_bytes = hdr[0];
    b->have_u16 = true;
    if (n_bytes) *n_bytes = hdr[0];
    return JTK_OK;
}

int jtk_batch_transcode_utf16_device(jtk_batch* b, const uint16_t* d_units, const int64_t* d_unit_off, int64_t n_docs, int64_t n_units,
                                     void* stream_or_null, int64_t* n_bytes) {
    return u16_transcode(b, /*for_encode=*/false, d_units, d_unit_off, n_docs, n_units, stream_or_null, n_bytes);
}

int jtk_batch_utf8_device_result(jtk_batch* b, const uint8_t** d_utf8, const int64_t** d_doc_off, int64_t* n_bytes) {
    if (!b || !b->have_u16) return fail(JTK_ERR_INVALID_ARGUMENT, "no UTF-16 transcode has run on this batch");
    if (d_utf8) *d_utf8 = b->u16_last_text;
    if (d_doc_off) *d_doc_off = b->u16_last_off;
    if (n_bytes) *n_bytes = b->u16_last_bytes;
    return JTK_OK;
}

static int u16_encode_flags(uint32_t flags) {
    if (flags & JTK_ENCODE_FIM) return fail(JTK_ERR_INVALID_ARGUMENT, FIM_ELSEWHERE);
    if (flags & (JTK_ENCODE_TO_HOST | JTK_ENCODE_COMPACT_IDS))
        return fail(JTK_ERR_INVALID_ARGUMENT, "JTK_ENCODE_TO_HOST and JTK_ENCODE_COMPACT_IDS are not for the UTF-16 entry points (the result stays on the device: jtk_batch_fetch, jtk_batch_compact)");
    return JTK_OK;
}

int jtk_batch_encode_utf16_device(jtk_batch* b, const uint16_t* d_units, const int64_t* d_unit_off, int64_t n_docs, int64_t n_units,
                                  uint32_t flags, void* stream_or_null, int64_t* n_tokens) {
    int rc;
    if ((rc = u16_encode_flags(flags))) return rc;
    int64_t n_bytes = 0;
    // (true: into u16_enc_*, and the last encode's result is dropped there, behind the argument checks, before the first write)
    if ((rc = u16_transcode(b, /*for_encode=*/true, d_units, d_unit_off, n_docs, n_units, stream_or_null, &n_bytes))) return rc;
    return jtk_batch_encode_device(b, (const uint8_t*)b->u16_enc_text.p, (const int64_t*)b->u16_enc_off.p, n_docs, n_bytes, flags, stream_or_null, n_tokens);
}

int jtk_batch_encode_utf16(jtk_batch* b, const uint16_t* units, const int64_t* unit_off, int64_t n_docs, uint32_t flags, int64_t* n_tokens) {
    if (!b || n_docs < 0 || !unit_off) return fail(JTK_ERR_INVALID_ARGUMENT, "bad arguments");
    int rc;
    if ((rc = u16_encode_flags(flags))) return rc;
    if (unit_off[0] < 0) return fail(JTK_ERR_INVALID_ARGUMENT, "unit_off must not be negative");
    for (int64_t d = 0; d < n_docs; d++)
        if (unit_off[d + 1] < unit_off[d]) return fail(JTK_ERR_INVALID_ARGUMENT, "unit_off must be non-decreasing");
    const int64_t n_units = unit_off[n_docs];                             // (the units behind the last document are not read)
    if (n_units > 0 && !units) return fail(JTK_ERR_INVALID_ARGUMENT, "units is NULL");
    if (n_units >= (int64_t)1 << 35) return fail(JTK_ERR_INVALID_ARGUMENT, "batch too large (32 Gi units per call at most)");
    HIP_TRY(hipSetDevice(b->enc->device));
    drop_encode_result(b);
    // one upload: units | offsets, then the device call (not chunk-pipelined)
    const size_t o_off = align_up((size_t)n_units * 2 + 16, 256);
    if ((rc = b->u16_in.ensure(o_off + ((size_t)n_docs + 1) * 8))) return rc;
    uint8_t* z = (uint8_t*)b->u16_in.p;
    if (n_units > 0) HIP_TRY(hipMemcpyAsync(z, units, (size_t)n_units * 2, hipMemcpyHostToDevice, b->stream));
    HIP_TRY(hipMemcpyAsync(z + o_off, unit_off, ((size_t)n_docs + 1) * 8, hipMemcpyHostToDevice, b->stream));
    int64_t nt = 0;
    if ((rc = jtk_batch_encode_utf16_device(b, (const uint16_t*)z, (const int64_t*)(z + o_off), n_docs, n_units, flags, nullptr, &nt))) return rc;
    if (n_tokens) *n_tokens = nt;
    return JTK_OK;
}

int jtk_batch_decode_utf16(jtk_batch* b, void* stream_or_null, int64_t* n_units) {
    if (!b || !b->have_decode) return fail(JTK_ERR_INVALID_ARGUMENT, "no decode has run on this batch");
    HIP_TRY(hipSetDevice(b->enc->device));
    hipStream_t s = pick_stream(b, stream_or_null);
    JtkU16DecWork w{};
    w.text = b->dwork.out; w.n_bytes = b->dec_total; w.byte_off = b->dwork.byte_off; w.n_seqs = b->dwork.n_seqs;
    w.n_tiles = (w.n_bytes + JTK_U16_D_TILE - 1) / JTK_U16_D_TILE;
    const size_t nt = (size_t)w.n_tiles;
    const size_t o_cnt = 16 + (nt + 1) * 8, o_sub = o_cnt + align_up(nt * 4 + 4, 16);
    int rc;
    if ((rc = b->u16_dscratch.ensure(o_sub + nt * JTK_U16_LANES * 2 + 16)) || (rc = b->u16_unit_off.ensure(((size_t)w.n_seqs + 1) * 8))) return rc;
    uint8_t* z = (uint8_t*)b->u16_dscratch.p;
    w.hdr = (int64_t*)z; w.tile_off = (int64_t*)(z + 16); w.tile_cnt = (uint32_t*)(z + o_cnt); w.sub = (uint16_t*)(z + o_sub);
    w.unit_off = (int64_t*)b->u16_unit_off.p;
    b->have_u16_dec = false;                                              // (this call replaces its own result)
    jtk_launch_u16_dec_count(w, s);
    HIP_TRY(hipGetLastError());
    int64_t total = 0;
    HIP_TRY(hipMemcpyAsync(&total, w.hdr, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if ((rc = b->u16_units.ensure((size_t)total * 2 + 64))) return rc;
    w.out = (uint16_t*)b->u16_units.p;
    jtk_launch_u16_dec_write(w, s);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s));                                     // (as decode: the fetch copies on no stream)
    b->u16_dec_units = total; b->u16_dec_seqs = w.n_seqs;
    b->have_u16_dec = true;
    if (n_units) *n_units = total;
    return JTK_OK;
}

int jtk_batch_decode_utf16_fetch(jtk_batch* b, uint16_t* units, int64_t units_cap, int64_t* unit_off, int32_t* status) {
    if (!b || !b->have_u16_dec) return fail(JTK_ERR_INVALID_ARGUMENT, "no jtk_batch_decode_utf16 has run on the last decode of this batch");
    HIP_TRY(hipSetDevice(b->enc->device));
    if (units) {
        if (units_cap < b->u16_dec_units) return fail(JTK_ERR_CAPACITY, "output buffer too small");
        if (b->u16_dec_units > 0) HIP_TRY(hipMemcpy(units, b->u16_units.p, (size_t)b->u16_dec_units * 2, hipMemcpyDeviceToHost));
    }
    if (unit_off) HIP_TRY(hipMemcpy(unit_off, b->u16_unit_off.p, ((size_t)b->u16_dec_seqs + 1) * 8, hipMemcpyDeviceToHost));
    if (status && b->u16_dec_seqs > 0) HIP_TRY(hipMemcpy(status, b->dwork.status, (size_t)b->u16_dec_seqs * 4, hipMemcpyDeviceToHost));
    return JTK_OK;
}

int jtk_batch_decode_utf16_device_result(jtk_batch* b, const uint16_t** d_units, const int64_t** d_unit_off, const int32_t** d_status) {
    if (!b || !b->have_u16_dec) return fail(JTK_ERR_INVALID_ARGUMENT, "no jtk_batch_decode_utf16 has run on the last decode of this batch");
    if (d_units) *d_units = (const uint16_t*)b->u16_units.p;
    if (d_unit_off) *d_unit_off = (const int64_t*)b->u16_unit_off.p;
    if (d_status) *d_status = b->dwork.status;
    return JTK_OK;
}

// ---- stop strings over the last decode (jtk_stop.hip) -------------------------------------------------
static_assert(JTK_STOP_MAX_STRINGS == JTK_ST_MAX_STRINGS && JTK_STOP_MAX_BYTES == JTK_ST_MAX_BYTES, "the rule header holds what the ABI takes");

int jtk_batch_decode_find_stops(jtk_batch* b, const uint8_t* strings, const uint32_t* str_off, int n_strings,
                                const int64_t* d_from_or_null, const int64_t* d_cell_byte_or_null, int64_t width,
                                void* stream_or_null) {
    if (!b || !b->have_decode) return fail(JTK_ERR_INVALID_ARGUMENT, "no decode has run on this batch");
    JtkStopWork& w = b->stop;
    b->have_stops = false;                                                // (this call replaces its own result, b->stop, in place)
    if (!jtk_stop_set_init(&w.set, strings, str_off, n_strings))
        return fail(JTK_ERR_INVALID_ARGUMENT, "stop strings: 0..16 strings of 1..64 bytes, str_off increasing from 0");
    // cell_byte belongs to a rows decode: the last decode must be one, of this width (after a flat decode there are no cells)
    if (d_cell_byte_or_null && (width < 1 || width != b->dec_rows_width))
        return fail(JTK_ERR_INVALID_ARGUMENT, "cell_byte needs the width of the rows decode it came from");
    HIP_TRY(hipSetDevice(b->enc->device));
    hipStream_t s = pick_stream(b, stream_or_null);
    const int64_t n = b->dwork.n_seqs;
    w.out = b->dwork.out; w.n_bytes = b->dec_total; w.byte_off = b->dwork.byte_off; w.n_seqs = n;
    w.n_tiles = (w.n_bytes + JTK_STOP_TILE - 1) / JTK_STOP_TILE;
    if (w.n_tiles >= ((int64_t)1 << 31) - 1) return fail(JTK_ERR_INVALID_ARGUMENT, "output too large");
    w.from = d_from_or_null; w.cell_byte = d_cell_byte_or_null; w.width = width;
    const size_t nn = (size_t)(n > 0 ? n : 1);
    int rc;
    if ((rc = b->stop_buf.ensure(nn * (4 * 8 + 2 * 4)))) return rc;
    uint8_t* z = (uint8_t*)b->stop_buf.p;
    w.keys = (unsigned long long*)z;
    w.stop_pos = (int64_t*)(z + nn * 16);
    w.stop_col = (int64_t*)(z + nn * 24);
    w.stop_which = (int32_t*)(z + nn * 32);
    w.hold = (int32_t*)(z + nn * 36);
    if (n > 0 && w.n_bytes == 0) {
        // every sequence is empty: stop_pos = E = 0, no match, nothing held, no column
        HIP_TRY(hipMemsetAsync(w.stop_pos, 0, nn * 8, s));
        HIP_TRY(hipMemsetAsync(w.stop_col, 0xFF, nn * 8 + nn * 4, s));         // stop_col | stop_which: -1
        HIP_TRY(hipMemsetAsync(w.hold, 0, nn * 4, s));
    } else if (n > 0) {
        HIP_TRY(hipMemsetAsync(w.keys, 0xFF, nn * 16, s));                      // JTK_STOP_NONE
        jtk_launch_stop_find(w, s);
        HIP_TRY(hipGetLastError());
    }
    b->stop_stream = s;
    b->have_stops = true;
    return JTK_OK;
}

int jtk_batch_decode_stops_fetch(jtk_batch* b, int64_t* stop_pos, int32_t* stop_which, int32_t* hold, int64_t* stop_col) {
    if (!b || !b->have_decode || !b->have_stops)
        return fail(JTK_ERR_INVALID_ARGUMENT, "no jtk_batch_decode_find_stops has run on the last decode of this batch");
    HIP_TRY(hipSetDevice(b->enc->device));
    HIP_TRY(hipStreamSynchronize(b->stop_stream));
    const size_t n = (size_t)b->stop.n_seqs;
    if (n == 0) return JTK_OK;
    if (stop_pos) HIP_TRY(hipMemcpy(stop_pos, b->stop.stop_pos, n * 8, hipMemcpyDeviceToHost));
    if (stop_which) HIP_TRY(hipMemcpy(stop_which, b->stop.stop_which, n * 4, hipMemcpyDeviceToHost));
    if (hold) HIP_TRY(hipMemcpy(hold, b->stop.hold, n * 4, hipMemcpyDeviceToHost));
    if (stop_col) HIP_TRY(hipMemcpy(stop_col, b->stop.stop_col, n * 8, hipMemcpyDeviceToHost));
    return JTK_OK;
}

int jtk_batch_decode_stops_device_result(jtk_batch* b, const int64_t** d_stop_pos, const int32_t** d_stop_which,
                                         const int32_t** d_hold, const int64_t** d_stop_col) {
    if (!b || !b->have_decode || !b->have_stops)
        return fail(JTK_ERR_INVALID_ARGUMENT, "no jtk_batch_decode_find_stops has run on the last decode of this batch");
    if (d_stop_pos) *d_stop_pos = b->stop.stop_pos;
    if (d_stop_which) *d_stop_which = b->stop.stop_which;
    if (d_hold) *d_hold = b->stop.hold;
    if (d_stop_col) *d_stop_col = b->stop.stop_col;
    return JTK_OK;
}

}  // extern "C"
