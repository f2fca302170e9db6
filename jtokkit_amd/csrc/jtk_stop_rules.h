// jtk_stop_rules.h -- stop strings over the last decode of a batch (jtk_batch_decode_find_stops): the rule the device kernels
// (jtk_stop.hip) and the CPU test shim tests/stop_sim share.  A stop string is a property of the decoded text, not of the
// ids: the search runs over the bytes `out` with byte_off[n_seqs + 1] of a flat or a rows decode.
//
// The rule.  n strings of 1..JTK_ST_MAX_BYTES bytes, in the caller's order; maxlen = the longest.  For sequence q:
//   range   [S, E): S = byte_off[q] + from[q] clamped into [0, byte_off[q + 1] - byte_off[q]] (without the array: 0),
//           E = byte_off[q + 1].  String i of length L matches at p when S <= p, p + L <= E and the bytes are equal: a match
//           never reaches into the next sequence, and one that starts before S does not count.
//   match   the match with the smallest p, among those the smallest i (duplicates are allowed: the first wins):
//           stop_pos = p (a position in `out`), stop_which = i, hold = 0.
//   none    stop_pos = E, stop_which = -1, hold = E - p* where p* is the smallest p in [max(S, E - (maxlen - 1)), E) for which
//           out[p, E) is a PROPER prefix of some string (0 without such a p): the trailing bytes that may still grow into a
//           stop string, which a streaming server must not emit yet.  hold < maxlen.
//   column  with the cell_byte [n_rows, width] of the rows decode and a match: stop_col = the largest column c with
//           cell_byte[q * width + c] <= stop_pos, the cell that holds the byte at stop_pos (cells without bytes in front of it
//           share its position and are smaller columns); -1 otherwise.
//
// How it is computed: `out` in tiles of JTK_STOP_TILE bytes, JTK_STOP_LANE consecutive bytes per lane.  A lane looks only at
// positions whose byte starts some string (jtk_stop_cand16), steps its sequence along (jtk_stop_lane) and reports, per
// sequence, its first match as the key p * JTK_ST_MAX_STRINGS + i and its first proper-prefix tail as p; the minimum of
// either over all lanes, JTK_STOP_NONE without one, is what jtk_stop_result reads.
#ifndef JTK_STOP_RULES_H
#define JTK_STOP_RULES_H

#include "jtk_device_prims.h"

#define JTK_ST_MAX_STRINGS 16                                // == JTK_STOP_MAX_STRINGS of the C ABI
#define JTK_ST_MAX_BYTES 64                                  // == JTK_STOP_MAX_BYTES
#define JTK_STOP_LANE 16                                     // bytes per lane: one aligned 16-byte word
#define JTK_STOP_LANES 256
#define JTK_STOP_TILE (JTK_STOP_LANES * JTK_STOP_LANE)       // bytes per workgroup
#define JTK_STOP_NONE 0xFFFFFFFFFFFFFFFFull                  // key of a sequence without a hit (all bytes 0xFF)

// The strings as the kernels take them (by value, as a launch argument): string i at byte i * JTK_ST_MAX_BYTES of `bytes`.
struct JtkStopSet {
    uint32_t bytes[JTK_ST_MAX_STRINGS * JTK_ST_MAX_BYTES / 4];
    uint32_t first[8];                                       // bit b: some string starts with byte b
    uint8_t len[JTK_ST_MAX_STRINGS];
    int32_t n, maxlen;
};

// the set from a blob and str_off[n + 1]; false when the arguments break the limits (nothing else is checked later)
inline bool jtk_stop_set_init(JtkStopSet* set, const uint8_t* strings, const uint32_t* str_off, int n) {
    *set = JtkStopSet{};
    if (n < 0 || n > JTK_ST_MAX_STRINGS) return false;
    if (n > 0 && (!strings || !str_off || str_off[0] != 0)) return false;
    uint8_t* sb = (uint8_t*)set->bytes;
    for (int i = 0; i < n; i++) {
        if (str_off[i + 1] <= str_off[i] || str_off[i + 1] - str_off[i] > JTK_ST_MAX_BYTES) return false;
        const uint32_t l = str_off[i + 1] - str_off[i];
        for (uint32_t k = 0; k < l; k++) sb[i * JTK_ST_MAX_BYTES + k] = strings[str_off[i] + k];
        set->len[i] = (uint8_t)l;
        set->first[sb[i * JTK_ST_MAX_BYTES] >> 5] |= 1u << (sb[i * JTK_ST_MAX_BYTES] & 31);
        if ((int32_t)l > set->maxlen) set->maxlen = (int32_t)l;
    }
    set->n = n;
    return true;
}

JTK_HD uint64_t jtk_stop_key(int64_t p, int i) { return (uint64_t)p * JTK_ST_MAX_STRINGS + (uint64_t)i; }

// S of sequence q
JTK_HD int64_t jtk_stop_start(const int64_t* byte_off, const int64_t* from, int64_t q) {
    const int64_t len = byte_off[q + 1] - byte_off[q];
    int64_t f = from ? from[q] : 0;
    f = f < 0 ? 0 : f > len ? len : f;
    return byte_off[q] + f;
}

// bit j: byte j of the 16-byte word w (the bytes at p0 .. p0 + 15, `left` of them inside `out`) starts some string
JTK_HD uint32_t jtk_stop_cand16(const uint32_t* first, const uint32_t (&w)[4], int64_t left) {
    uint32_t cand = 0;
#pragma unroll
    for (int j = 0; j < JTK_STOP_LANE; j++) {
        const uint32_t b = (w[j >> 2] >> (8 * (j & 3))) & 0xFFu;
        cand |= ((first[b >> 5] >> (b & 31)) & 1u) << j;
    }
    if (left < JTK_STOP_LANE) cand &= (1u << left) - 1u;
    return cand;
}

// the first string of the list that matches at p and ends at or before E; -1: none.  at(x) = out[x], read for p <= x < E only.
template <class At>
JTK_HD int jtk_stop_match_at(const uint8_t* sb, const uint8_t* len, int n, At at, int64_t p, int64_t E) {
    for (int i = 0; i < n; i++) {
        const int l = len[i];
        if (p + l > E) continue;
        int k = 0;
        while (k < l && at(p + k) == sb[i * JTK_ST_MAX_BYTES + k]) k++;
        if (k == l) return i;
    }
    return -1;
}

// is out[p, E) (1 <= E - p) a proper prefix of some string?
template <class At>
JTK_HD bool jtk_stop_prefix_at(const uint8_t* sb, const uint8_t* len, int n, At at, int64_t p, int64_t E) {
    const int64_t m = E - p;
    for (int i = 0; i < n; i++) {
        if ((int64_t)len[i] <= m) continue;
        int64_t k = 0;
        while (k < m && at(p + k) == sb[i * JTK_ST_MAX_BYTES + k]) k++;
        if (k == m) return true;
    }
    return false;
}

// One lane: the candidate positions p0 + j (bits of cand, ascending) of `out`.  The sequence of a position is searched when
// the position lies past the current one (empty sequences are skipped: the last k with byte_off[k] <= p holds p), never
// walked.  emit(q, false, key) for the lane's first match in sequence q, emit(q, true, p) for its first proper-prefix tail
// there when no match came before it: every later hit of the lane in q is larger.  The index q is clamped, so that offsets
// that do not ascend are never followed out of range.
template <class At, class Emit>
JTK_HD void jtk_stop_lane(const uint8_t* sb, const uint8_t* len, int n, int maxlen, uint32_t cand, int64_t p0, const int64_t* byte_off,
                          int64_t n_seqs, const int64_t* from, At at, Emit emit) {
    int64_t q = -1, S = 0, E = 0;
    bool sent_match = false, sent_hold = false;
    for (uint32_t m = cand; m;) {
        const int j = __builtin_ctz(m);
        m &= m - 1;
        const int64_t p = p0 + j;
        if (p >= E) {
            q = jtk_first_gt(byte_off, q + 1, n_seqs + 1, p) - 1;
            if (q > n_seqs - 1) q = n_seqs - 1;
            if (q < 0) q = 0;
            S = jtk_stop_start(byte_off, from, q);
            E = byte_off[q + 1];
            sent_match = sent_hold = false;
        }
        if (p < S || sent_match) continue;
        const int i = jtk_stop_match_at(sb, len, n, at, p, E);
        if (i >= 0) {
            emit(q, false, jtk_stop_key(p, i));
            sent_match = true;
        } else if (!sent_hold && E - p < (int64_t)maxlen && jtk_stop_prefix_at(sb, len, n, at, p, E)) {
            emit(q, true, (uint64_t)p);
            sent_hold = true;
        }
    }
}

struct JtkStopResult { int64_t pos; int32_t which, hold; };

// from the two minima of a sequence that ends at E
JTK_HD JtkStopResult jtk_stop_result(uint64_t key, uint64_t hold_key, int64_t E) {
    JtkStopResult r;
    if (key != JTK_STOP_NONE) {
        r.pos = (int64_t)(key / JTK_ST_MAX_STRINGS); r.which = (int32_t)(key % JTK_ST_MAX_STRINGS); r.hold = 0;
    } else {
        r.pos = E; r.which = -1; r.hold = hold_key != JTK_STOP_NONE ? (int32_t)(E - (int64_t)hold_key) : 0;
    }
    return r;
}

// the column of row q that holds the byte at pos (byte_off[q] <= pos): the one before the first c with cell_byte > pos
JTK_HD int64_t jtk_stop_col(const int64_t* cell_byte, int64_t q, int64_t width, int64_t pos) {
    return jtk_first_gt(cell_byte + q * width, 0, width, pos) - 1;
}

#endif
