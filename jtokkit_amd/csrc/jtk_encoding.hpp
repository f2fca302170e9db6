// jtk_encoding.hpp -- header-only C++ mirror of the reference's `Encoding` interface
// (reference lib/src/main/java/com/knuddels/jtokkit/api/Encoding.java:29-189) over the C ABI.
// The reference is compiled (JVM) code and no JDK exists in the build image, so this class is the
// host-side stand-in for the Java `HipEncoding implements Encoding` shown in INTEGRATION.md:
// same method names, argument meaning and error behaviour (status codes become exceptions).
// Like the Java shim, the per-call methods go through the encoding's jtk_service (thread-safe, concurrent callers
// coalesced into device batches); the batch methods use the object's own jtk_batch (one caller at a time).
// Compiled and run by the CPU test tier (tests/test_abi_and_host.py: no device -> IllegalStateException) and used by
// tools/percall for nothing: it is the C++ face of the boundary, kept honest by that test.
#ifndef JTK_ENCODING_HPP
#define JTK_ENCODING_HPP

#include <cstdint>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../../include/jtokkit_amd.h"

namespace jtokkit {

struct UnsupportedOperationException : std::runtime_error { using std::runtime_error::runtime_error; };
struct IllegalArgumentException : std::invalid_argument { using std::invalid_argument::invalid_argument; };
struct IllegalStateException : std::runtime_error { using std::runtime_error::runtime_error; };

struct EncodingResult {                       // api/EncodingResult.java
    std::vector<int32_t> tokens;
    bool truncated;
    const std::vector<int32_t>& getTokens() const { return tokens; }
    bool isTruncated() const { return truncated; }
};

class Encoding {
public:
    Encoding(const std::string& name, int patternKind, const std::string& tiktokenBytes,
             const std::vector<std::pair<std::string, int32_t>>& specials, int device = 0) {
        std::vector<const char*> lits;
        std::vector<int32_t> ids;
        for (auto& s : specials) { lits.push_back(s.first.c_str()); ids.push_back(s.second); }
        check(jtk_encoding_create(name.c_str(), patternKind, (const uint8_t*)tiktokenBytes.data(), tiktokenBytes.size(),
                                  lits.data(), ids.data(), (int)lits.size(), device, &enc_));
        check(jtk_batch_create(enc_, &batch_));
        check(jtk_service_create(enc_, 2, &svc_));
    }
    ~Encoding() { jtk_service_destroy(svc_); jtk_batch_destroy(batch_); jtk_encoding_destroy(enc_); }
    Encoding(const Encoding&) = delete;
    Encoding& operator=(const Encoding&) = delete;

    std::vector<int32_t> encode(const std::string& text) { return run(text, 0, -1).tokens; }
    EncodingResult encode(const std::string& text, int maxTokens) { return run(text, 0, maxTokens); }
    std::vector<int32_t> encodeOrdinary(const std::string& text) { return run(text, JTK_ENCODE_ORDINARY, -1).tokens; }
    EncodingResult encodeOrdinary(const std::string& text, int maxTokens) { return run(text, JTK_ENCODE_ORDINARY, maxTokens); }
    int countTokens(const std::string& text) { return (int)encode(text).size(); }
    int countTokensOrdinary(const std::string& text) { return (int)encodeOrdinary(text).size(); }
    std::string decodeBytes(const std::vector<int32_t>& tokens) const {
        int64_t len = 0;
        check(jtk_decode(enc_, tokens.data(), (int64_t)tokens.size(), nullptr, 0, &len));
        std::string out((size_t)len, '\0');
        check(jtk_decode(enc_, tokens.data(), (int64_t)tokens.size(), (uint8_t*)&out[0], len, &len));
        return out;
    }
    std::string decode(const std::vector<int32_t>& tokens) const { return decodeBytes(tokens); }
    std::string getName() const { return jtk_encoding_name(enc_); }

    // batch: documents back to back in `utf8`, n+1 offsets -> packed ids + n+1 token offsets + per-doc status
    void encodeBatch(const uint8_t* utf8, const std::vector<int64_t>& docOff, bool ordinary,
                     std::vector<int32_t>& tokens, std::vector<int64_t>& tokOff, std::vector<int32_t>& status) {
        int64_t nt = 0;
        const int64_t n = (int64_t)docOff.size() - 1;
        check(jtk_batch_encode(batch_, utf8, docOff.data(), n, ordinary ? JTK_ENCODE_ORDINARY : 0u, &nt));
        tokens.resize((size_t)nt); tokOff.resize((size_t)n + 1); status.resize((size_t)n);
        check(jtk_batch_fetch(batch_, tokens.data(), nt, tokOff.data(), status.data()));
    }

    // encodeBatch with the allowed special ids encoded as ids (JTK_ENCODE_ALLOW_SPECIAL; the rule is in jtokkit_amd.h);
    // allowedIds empty: none allowed, as the call without the flag
    void encodeBatchWithSpecialTokens(const uint8_t* utf8, const std::vector<int64_t>& docOff, const std::vector<int32_t>& allowedIds,
                                      bool ordinary, std::vector<int32_t>& tokens, std::vector<int64_t>& tokOff,
                                      std::vector<int32_t>& status) {
        int64_t nt = 0;
        const int64_t n = (int64_t)docOff.size() - 1;
        check(jtk_batch_set_allowed_special(batch_, allowedIds.data(), (int)allowedIds.size()));
        check(jtk_batch_encode(batch_, utf8, docOff.data(), n, (ordinary ? JTK_ENCODE_ORDINARY : 0u) | JTK_ENCODE_ALLOW_SPECIAL, &nt));
        tokens.resize((size_t)nt); tokOff.resize((size_t)n + 1); status.resize((size_t)n);
        check(jtk_batch_fetch(batch_, tokens.data(), nt, tokOff.data(), status.data()));
    }

    // custom split pattern: the caller's matches (byte ranges in the whole batch) instead of the device's split
    // (api/GptBytePairEncodingParams.java:36-46); text between matches is skipped as matcher.find() does
    void encodeBatchPieces(const uint8_t* utf8, const std::vector<int64_t>& docOff, const std::vector<int64_t>& pieceBegin,
                           const std::vector<int64_t>& pieceEnd, bool ordinary, std::vector<int32_t>& tokens,
                           std::vector<int64_t>& tokOff, std::vector<int32_t>& status) {
        int64_t nt = 0;
        const int64_t n = (int64_t)docOff.size() - 1;
        check(jtk_batch_encode_pieces(batch_, utf8, docOff.data(), n, pieceBegin.data(), pieceEnd.data(), (int64_t)pieceBegin.size(),
                                      ordinary ? JTK_ENCODE_ORDINARY : 0u, &nt));
        tokens.resize((size_t)nt); tokOff.resize((size_t)n + 1); status.resize((size_t)n);
        check(jtk_batch_fetch(batch_, tokens.data(), nt, tokOff.data(), status.data()));
    }

    // batch encode(text, maxTokens): after encodeBatch, how many of each document's tokens survive the limit (incl. the
    // reference's back-off to a code-point boundary) and EncodingResult.isTruncated() per document
    void truncateBatch(int64_t maxTokens, std::vector<int64_t>& kept, std::vector<uint8_t>& truncated, size_t nDocs) {
        check(jtk_batch_truncate(batch_, maxTokens));
        kept.resize(nDocs); truncated.resize(nDocs);
        check(jtk_batch_fetch_truncated(batch_, kept.data(), truncated.data()));
    }

    // character positions of the last encodeBatch's text (device arrays; unit JTK_UNIT_UTF16 for indices into a Java String):
    // every document's length, byte positions -> indices, indices -> byte positions, and every token's [begin, end)
    void charIndex(int unit, int64_t* dDocUnits = nullptr, void* stream = nullptr) {
        check(jtk_batch_char_index(batch_, unit, dDocUnits, stream));
    }
    void charPositions(int unit, int round, const int64_t* dDoc, const int64_t* dBytePos, int64_t n, int64_t* dCharPos,
                       void* stream = nullptr) {
        check(jtk_batch_char_positions(batch_, unit, round, dDoc, dBytePos, n, dCharPos, stream));
    }
    void bytePositions(int unit, const int64_t* dDoc, const int64_t* dCharPos, int64_t n, int64_t* dBytePos, void* stream = nullptr) {
        check(jtk_batch_byte_positions(batch_, unit, dDoc, dCharPos, n, dBytePos, stream));
    }
    void tokenCharOffsets(int unit, int64_t* dBegin, int64_t* dEnd = nullptr, void* stream = nullptr) {
        check(jtk_batch_token_char_offsets(batch_, unit, dBegin, dEnd, stream));
    }

    // token n-gram sets for decontamination (the rule is in jtokkit_amd.h): a set of this encoding, owned by the caller and freed
    // with ngramSetDestroy before the Encoding; the n-grams of the last encodeBatch or host keys into it; its size and keys; and
    // the overlap of the last encodeBatch with it into device arrays (each may be NULL)
    jtk_ngram_set* ngramSetCreate(int32_t ngram, uint64_t seed = 0) {
        const jtk_ngram_params p{seed, ngram, 0u};
        jtk_ngram_set* s = nullptr;
        check(jtk_ngram_set_create(enc_, &p, &s));
        return s;
    }
    static void ngramSetDestroy(jtk_ngram_set* s) { jtk_ngram_set_destroy(s); }
    void ngramSetAddLastEncode(jtk_ngram_set* s, void* stream = nullptr) { check(jtk_ngram_set_add_batch(s, batch_, stream)); }
    static void ngramSetAddKeys(jtk_ngram_set* s, const std::vector<uint64_t>& keys) {
        check(jtk_ngram_set_add_keys(s, keys.data(), (int64_t)keys.size()));
    }
    static std::vector<uint64_t> ngramSetKeys(const jtk_ngram_set* s, int64_t* capacity = nullptr) {
        int64_t n = 0;
        check(jtk_ngram_set_size(s, &n, capacity));
        std::vector<uint64_t> keys((size_t)n);
        check(jtk_ngram_set_keys(s, keys.data(), n));
        return keys;
    }
    void ngramOverlap(const jtk_ngram_set* s, uint8_t* dTokFlags, int32_t* dNHit = nullptr, int32_t* dNCovered = nullptr,
                      int64_t* dFirstHit = nullptr, void* stream = nullptr) {
        check(jtk_batch_ngram_overlap(batch_, s, dTokFlags, dNHit, dNCovered, dFirstHit, stream));
    }
    // repeated n-grams inside the documents of the last encode (jtk_batch_ngram_repeats); every output may be nullptr
    void ngramRepeats(const jtk_repeat_params& params, uint8_t* dTokFlags, int32_t* dNRepeat = nullptr, int32_t* dNCovered = nullptr,
                      int32_t* dTopCount = nullptr, int64_t* dTopFirst = nullptr, void* stream = nullptr) {
        check(jtk_batch_ngram_repeats(batch_, &params, dTokFlags, dNRepeat, dNCovered, dTopCount, dTopFirst, stream));
    }

    // duplicate lines / paragraphs inside the documents of the last encode's text: lineUnits finds and hashes the units and
    // returns their number (jtk_batch_line_units), lineRepeats writes what `out` asks for (jtk_batch_line_repeats; same params)
    int64_t lineUnits(const jtk_lines_params& params, void* stream = nullptr) {
        int64_t n = 0;
        check(jtk_batch_line_units(batch_, &params, stream, &n));
        return n;
    }
    void lineRepeats(const jtk_lines_params& params, const jtk_lines_out& out, void* stream = nullptr) {
        check(jtk_batch_line_repeats(batch_, &params, &out, stream));
    }

    // batch decodeBytes: token lists back to back in `ids`, n+1 offsets -> bytes back to back + n+1 byte offsets + status
    void decodeBatch(const int32_t* ids, const std::vector<int64_t>& seqOff, std::string& bytes,
                     std::vector<int64_t>& byteOff, std::vector<int32_t>& status) {
        int64_t nb = 0;
        const int64_t n = (int64_t)seqOff.size() - 1;
        check(jtk_batch_decode(batch_, ids, seqOff.data(), n, &nb));
        bytes.resize((size_t)nb); byteOff.resize((size_t)n + 1); status.resize((size_t)n);
        check(jtk_batch_decode_fetch(batch_, (uint8_t*)&bytes[0], nb, byteOff.data(), status.data()));
    }

    // batch decodeBytes of the rows of an id matrix (IdT = int32_t or int64_t; nRows x width, row r at element r * rowStride): each
    // row's window [begin[r], end[r]) (empty vectors: the whole row), cut at its first stop id, pad cells skipped with
    // JTK_DECODE_SKIP_PAD in flags -> bytes back to back + nRows+1 byte offsets + status (+ the byte position of every cell)
    template <class IdT>
    void decodeRows(const IdT* rows, int64_t nRows, int64_t width, int64_t rowStride, const std::vector<int64_t>& begin,
                    const std::vector<int64_t>& end, int64_t padId, const std::vector<int64_t>& stopIds, uint32_t flags,
                    std::string& bytes, std::vector<int64_t>& byteOff, std::vector<int32_t>& status,
                    std::vector<int64_t>* cellByte = nullptr) {
        static_assert(sizeof(IdT) == 4 || sizeof(IdT) == 8, "ids are 32 or 64 bits");
        int64_t nb = 0;
        if (cellByte) cellByte->resize((size_t)(nRows * width));
        check(jtk_batch_decode_rows(batch_, rows, (int)sizeof(IdT), nRows, width, rowStride, begin.empty() ? nullptr : begin.data(),
                                    end.empty() ? nullptr : end.data(), padId, stopIds.empty() ? nullptr : stopIds.data(),
                                    (int)stopIds.size(), flags, cellByte ? cellByte->data() : nullptr, &nb));
        bytes.resize((size_t)nb); byteOff.resize((size_t)nRows + 1); status.resize((size_t)nRows);
        check(jtk_batch_decode_fetch(batch_, (uint8_t*)&bytes[0], nb, byteOff.data(), status.data()));
    }

private:
    EncodingResult run(const std::string& text, uint32_t flags, int64_t maxTokens) {
        EncodingResult r{std::vector<int32_t>(text.size() + 1), false};
        int64_t n = 0; int tr = 0;
        check(jtk_service_encode(svc_, (const uint8_t*)text.data(), (int64_t)text.size(), flags, maxTokens, r.tokens.data(),
                                 (int64_t)r.tokens.size(), &n, &tr));
        r.tokens.resize((size_t)n);
        r.truncated = tr != 0;
        return r;
    }
    static void check(int rc) {
        if (rc == JTK_OK) return;
        const std::string msg = jtk_last_error();
        if (rc == JTK_ERR_UNSUPPORTED_SPECIAL) throw UnsupportedOperationException("Encoding special tokens is not supported yet.");
        if (rc == JTK_ERR_UNKNOWN_TOKEN || rc == JTK_ERR_INVALID_ARGUMENT) throw IllegalArgumentException(msg);
        throw IllegalStateException(msg);
    }
    jtk_encoding* enc_ = nullptr;
    jtk_batch* batch_ = nullptr;
    jtk_service* svc_ = nullptr;
};

}  // namespace jtokkit
#endif
