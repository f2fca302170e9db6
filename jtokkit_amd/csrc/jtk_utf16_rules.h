// jtk_utf16_rules.h -- UTF-16 in and out (jtk_batch_transcode_utf16_device, jtk_batch_encode_utf16*, jtk_batch_decode_utf16):
// the two transcoding rules that the device kernels (jtk_utf16.hip) and the CPU test shim tests/utf16_sim share.  Each rule is
// defined for ANY input and is a function of one position and a bounded window around it, so the count pass, the write pass,
// the shim and the plain reference (tests/utf16_ref.py) cannot drift apart.
//
// E -- UTF-16 -> UTF-8, the rule of String.getBytes(UTF_8).  Document d is units [unit_off[d], unit_off[d + 1]) of a uint16
// array in the byte order of host and device (little-endian).  No BOM handling: a U+FEFF is a character.  The bytes that the
// unit u at position i of its document contributes (window: one unit back, one ahead):
//   u < 0x80                          1 byte
//   u < 0x800                         2 bytes
//   any other non-surrogate           3 bytes
//   a high surrogate (D800..DBFF) whose next unit is IN THE SAME DOCUMENT and is a low surrogate (DC00..DFFF)
//                                     the 4 bytes of the pair's code point, at the high surrogate's place
//   the low surrogate of such a pair  0 bytes
//   every other surrogate             the single byte 0x3F ('?'): a lone high, a lone low, a high that is the last unit of its
//                                     document even if the next document starts with a low, the first high of `high high low`
// A unit outside [unit_off[0], unit_off[n_docs]) belongs to no document and contributes nothing.  doc_off[d] = the bytes
// contributed by the units before unit_off[d]; doc_off[0] = 0.
// CONSEQUENCE: for the transcoded text, U(a, e) of jtk_charpos_rules.h in JTK_UNIT_UTF16 equals the document's original unit
// count ('?' weighs 1, a 4-byte character weighs 2, every other character 1), so every UTF-16 position the library hands out
// after such an encode is an index into the caller's original char[].
//
// D -- UTF-8 -> UTF-16, the rule of new String(bytes, UTF_8).  Sequence q is bytes [byte_off[q], byte_off[q + 1]).  The
// well-formed sequences are those of Unicode Table 3-7: a lead C2..DF and one continuation byte (80..BF); E0 A0..BF, E1..EC
// 80..BF, ED 80..9F, EE..EF 80..BF and one more continuation byte; F0 90..BF, F1..F3 80..BF, F4 80..8F and two more.  C0, C1 and
// F5..FF are never leads.
//   a byte j that is no continuation byte: L(j) = the bytes the automaton of that table accepts from j on; it stops at the first
//       byte it rejects and at the end of the sequence, L(j) >= 1.  When those L(j) bytes are a complete character, byte j emits
//       its unit, or its two units (a surrogate pair) for a 4-byte character; otherwise it emits one U+FFFD.
//   a continuation byte i emits nothing when it is CONSUMED, else one U+FFFD.  It is consumed when the nearest byte j before
//       it that is no continuation byte lies within i - 3 .. i - 1 and inside the sequence, and i - j < L(j).
// So the window is 3 bytes back and 3 ahead, clipped to the sequence.  unit_off[q] = the units emitted before byte_off[q].
// This is one U+FFFD per maximal ill-formed subpart: CPython's bytes.decode("utf-8", "replace") followed by
// .encode("utf-16-le").  No JVM is at hand where this is built: the parity claim of D (and of E: str.encode("utf-8") of the
// units with every unpaired surrogate replaced by '?') is against those codecs, which the CPU tier checks exhaustively.
//
// How the kernels use it: fixed tiles (JTK_U16_E_TILE units, JTK_U16_D_TILE bytes), 256 lanes, one 16-byte granule per lane;
// count per lane -> prefix inside the tile (sub) and tile totals -> scan of the tile totals -> write.  jtk_u16_e_lane and
// jtk_u16_d_lane are a lane's whole work in either pass (out == NULL: count only).
#ifndef JTK_UTF16_RULES_H
#define JTK_UTF16_RULES_H

#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define JTK_U16_HD __host__ __device__ inline
#else
#define JTK_U16_HD inline
#endif

#define JTK_U16_LANES 256                                   // lanes per tile
#define JTK_U16_E_PER_LANE 8                                // units per lane: one 16-byte granule
#define JTK_U16_D_PER_LANE 16                               // bytes per lane: one 16-byte granule
#define JTK_U16_E_TILE (JTK_U16_LANES * JTK_U16_E_PER_LANE) // 2048 units, at most 6144 bytes out
#define JTK_U16_D_TILE (JTK_U16_LANES * JTK_U16_D_PER_LANE) // 4096 bytes, at most 4096 units out

struct alignas(16) JtkU16Quad { uint32_t w[4]; };           // 16 bytes: 8 units (unit k in bits 16 (k % 2) .. of w[k / 2]) or 16 bytes

// ---- E
JTK_U16_HD bool jtk_u16_is_high(uint32_t u) { return (u & 0xFC00u) == 0xD800u; }
JTK_U16_HD bool jtk_u16_is_low(uint32_t u) { return (u & 0xFC00u) == 0xDC00u; }
JTK_U16_HD bool jtk_u16_is_surrogate(uint32_t u) { return (u & 0xF800u) == 0xD800u; }

// whether unit u at position g needs to know a document edge: a high in front of a low (is g + 1 an edge?), a low behind a
// high (is g an edge?).  Only then is the edge looked up.
JTK_U16_HD bool jtk_u16_e_needs_edge(uint32_t u, uint32_t prev, uint32_t next) {
    return (jtk_u16_is_high(u) && jtk_u16_is_low(next)) || (jtk_u16_is_low(u) && jtk_u16_is_high(prev));
}
// the bytes of unit u.  prev / next: the units before and after it (any value where there is none); edge: a document starts
// or the batch ends between u and that partner (asked only when jtk_u16_e_needs_edge)
JTK_U16_HD uint32_t jtk_u16_e_len(uint32_t u, uint32_t prev, uint32_t next, bool edge) {
    if (!jtk_u16_is_surrogate(u)) return 1u + (u >= 0x80u ? 1u : 0u) + (u >= 0x800u ? 1u : 0u);
    if (jtk_u16_is_high(u)) return (jtk_u16_is_low(next) && !edge) ? 4u : 1u;
    return (jtk_u16_is_high(prev) && !edge) ? 0u : 1u;
}
// writes the len bytes of unit u (len from jtk_u16_e_len) to out
JTK_U16_HD void jtk_u16_e_put(uint32_t u, uint32_t next, uint32_t len, uint8_t* out) {
    if (len == 1u) {
        out[0] = jtk_u16_is_surrogate(u) ? (uint8_t)0x3F : (uint8_t)u;
    } else if (len == 2u) {
        out[0] = (uint8_t)(0xC0u | u >> 6); out[1] = (uint8_t)(0x80u | (u & 0x3Fu));
    } else if (len == 3u) {
        out[0] = (uint8_t)(0xE0u | u >> 12); out[1] = (uint8_t)(0x80u | (u >> 6 & 0x3Fu)); out[2] = (uint8_t)(0x80u | (u & 0x3Fu));
    } else if (len == 4u) {
        const uint32_t c = 0x10000u + ((u & 0x3FFu) << 10) + (next & 0x3FFu);
        out[0] = (uint8_t)(0xF0u | c >> 18); out[1] = (uint8_t)(0x80u | (c >> 12 & 0x3Fu));
        out[2] = (uint8_t)(0x80u | (c >> 6 & 0x3Fu)); out[3] = (uint8_t)(0x80u | (c & 0x3Fu));
    }
}
// all 8 units of the granule are below 0x80 (one byte each, no window needed)
JTK_U16_HD bool jtk_u16_e_all_ascii(const JtkU16Quad& g) { return ((g.w[0] | g.w[1] | g.w[2] | g.w[3]) & 0xFF80FF80u) == 0u; }
JTK_U16_HD uint32_t jtk_u16_quad_unit(const JtkU16Quad& g, int k) { return g.w[k >> 1] >> (16 * (k & 1)) & 0xFFFFu; }

// A lane of E: units g0 .. g0 + 7 (those in [lo, hi) are live), prev = unit g0 - 1, next = unit g0 + 8 (any value where there
// is none).  is_edge(x): a document starts at unit x or the documents end there (x is one of unit_off[0 .. n_docs]); called
// only where jtk_u16_e_needs_edge.  Returns the lane's bytes; out != NULL: writes them there.
template <class Edge>
JTK_U16_HD uint32_t jtk_u16_e_lane(const JtkU16Quad& g, uint32_t prev, uint32_t next, int64_t g0, int64_t lo, int64_t hi, Edge is_edge,
                                   uint8_t* out) {
    if (g0 >= lo && g0 + JTK_U16_E_PER_LANE <= hi && jtk_u16_e_all_ascii(g)) {
        if (out)
#pragma unroll
            for (int k = 0; k < JTK_U16_E_PER_LANE; k++) out[k] = (uint8_t)jtk_u16_quad_unit(g, k);
        return JTK_U16_E_PER_LANE;
    }
    uint32_t n = 0;
#pragma unroll
    for (int k = 0; k < JTK_U16_E_PER_LANE; k++) {
        const int64_t x = g0 + k;
        if (x < lo || x >= hi) continue;
        const uint32_t u = jtk_u16_quad_unit(g, k);
        const uint32_t p = k ? jtk_u16_quad_unit(g, k ? k - 1 : 0) : prev;
        const uint32_t q = k + 1 < JTK_U16_E_PER_LANE ? jtk_u16_quad_unit(g, k + 1 < JTK_U16_E_PER_LANE ? k + 1 : 0) : next;
        bool edge = false;
        if (jtk_u16_e_needs_edge(u, p, q)) edge = is_edge(jtk_u16_is_high(u) ? x + 1 : x);
        const uint32_t len = jtk_u16_e_len(u, p, q, edge);
        if (out) jtk_u16_e_put(u, q, len, out + n);
        n += len;
    }
    return n;
}

// ---- D
JTK_U16_HD bool jtk_u16_is_cont(uint32_t x) { return (x & 0xC0u) == 0x80u; }

// L(j): the bytes the automaton accepts from the byte b0 (no continuation byte) on, given the bytes b1, b2, b3 after it, of
// which `ahead` (0 .. 3) are inside the sequence; *need = the length of the character that b0 leads (1 for a byte that leads
// none: the character is complete exactly when the return value equals *need and b0 is a valid lead)
JTK_U16_HD int jtk_u16_d_accept(uint32_t b0, uint32_t b1, uint32_t b2, uint32_t b3, int ahead, int* need, bool* lead_ok) {
    *lead_ok = true;
    if (b0 < 0x80u) { *need = 1; return 1; }
    uint32_t lo2 = 0x80u, hi2 = 0xBFu;
    int n;
    if (b0 >= 0xC2u && b0 <= 0xDFu) n = 2;
    else if (b0 >= 0xE0u && b0 <= 0xEFu) { n = 3; if (b0 == 0xE0u) lo2 = 0xA0u; if (b0 == 0xEDu) hi2 = 0x9Fu; }
    else if (b0 >= 0xF0u && b0 <= 0xF4u) { n = 4; if (b0 == 0xF0u) lo2 = 0x90u; if (b0 == 0xF4u) hi2 = 0x8Fu; }
    else { *need = 1; *lead_ok = false; return 1; }                     // C0, C1, F5..FF (and a continuation byte, never asked)
    *need = n;
    if (ahead < 1 || b1 < lo2 || b1 > hi2) return 1;
    if (n == 2) return 2;
    if (ahead < 2 || !jtk_u16_is_cont(b2)) return 2;
    if (n == 3) return 3;
    if (ahead < 3 || !jtk_u16_is_cont(b3)) return 3;
    return 4;
}

// The units of the byte in the middle of the window: win holds bytes i - 3 .. i + 3 in bits 0 .. 55 (byte i in bits 24 .. 31);
// back / ahead (0 .. 3): how many of the bytes before / after i are inside its sequence (the others may hold anything).
// Returns 0, 1 or 2 and writes that many units to o (o[0], o[1] are always written).
JTK_U16_HD int jtk_u16_d_emit(uint64_t win, int back, int ahead, uint16_t* o) {
#define JTK_U16_B(k) ((uint32_t)(win >> (8 * ((k) + 3))) & 0xFFu)
    const uint32_t x = JTK_U16_B(0);
    int need;
    bool ok;
    o[0] = 0xFFFDu; o[1] = 0;
    if (!jtk_u16_is_cont(x)) {
        const uint32_t b1 = JTK_U16_B(1), b2 = JTK_U16_B(2), b3 = JTK_U16_B(3);
        const int L = jtk_u16_d_accept(x, b1, b2, b3, ahead, &need, &ok);
        if (!ok || L != need) return 1;
        if (need == 1) { o[0] = (uint16_t)x; return 1; }
        if (need == 2) { o[0] = (uint16_t)((x & 0x1Fu) << 6 | (b1 & 0x3Fu)); return 1; }
        if (need == 3) { o[0] = (uint16_t)((x & 0x0Fu) << 12 | (b1 & 0x3Fu) << 6 | (b2 & 0x3Fu)); return 1; }
        const uint32_t c = ((x & 0x07u) << 18 | (b1 & 0x3Fu) << 12 | (b2 & 0x3Fu) << 6 | (b3 & 0x3Fu)) - 0x10000u;
        o[0] = (uint16_t)(0xD800u | c >> 10); o[1] = (uint16_t)(0xDC00u | (c & 0x3FFu));
        return 2;
    }
    // a continuation byte: the nearest byte before it that is none, at most 3 back and inside the sequence
    for (int k = 1; k <= 3 && k <= back; k++) {
        const uint32_t j = JTK_U16_B(-k);
        if (jtk_u16_is_cont(j)) continue;
        // (the bytes after j: up to i + 2, all inside the window; k + ahead of them are inside the sequence)
        const int L = jtk_u16_d_accept(j, JTK_U16_B(1 - k), JTK_U16_B(2 - k), JTK_U16_B(3 - k), k + ahead > 3 ? 3 : k + ahead, &need, &ok);
        return k < L ? 0 : 1;
    }
    return 1;
#undef JTK_U16_B
}

// all 16 bytes of the granule are below 0x80 (one unit each, no window needed)
JTK_U16_HD bool jtk_u16_d_all_ascii(const JtkU16Quad& g) { return ((g.w[0] | g.w[1] | g.w[2] | g.w[3]) & 0x80808080u) == 0u; }

// back / ahead of byte b (0 .. 15) of a lane from the lane's edge mask: bit x + 2 set when a sequence starts or the sequences end
// at byte g0 + x, for x = -2 .. 18
JTK_U16_HD void jtk_u16_d_avail(uint32_t edges, int b, int* back, int* ahead) {
    const uint32_t m = edges >> b;                                      // bit 2: an edge at byte i itself
    *back = (m & 4u) ? 0 : (m & 2u) ? 1 : (m & 1u) ? 2 : 3;
    *ahead = (m & 8u) ? 0 : (m & 16u) ? 1 : (m & 32u) ? 2 : 3;
}

// A lane of D: bytes g0 .. g0 + 15 (those below n_bytes are live), prev = the 4 bytes before g0 (byte g0 - 1 in bits 24 .. 31),
// next = the 4 bytes from g0 + 16 on (any value where there is none: the edges clip them).  edge_mask(): the lane's edge mask
// (above), asked for only when the lane holds a byte >= 0x80.  Returns the lane's units; out != NULL: writes them there.
template <class Edges>
JTK_U16_HD uint32_t jtk_u16_d_lane(const JtkU16Quad& g, uint32_t prev, uint32_t next, int64_t g0, int64_t n_bytes, Edges edge_mask,
                                   uint16_t* out) {
    const int64_t left = n_bytes - g0;
    if (left <= 0) return 0;
    if (left >= JTK_U16_D_PER_LANE && jtk_u16_d_all_ascii(g)) {
        if (out)
#pragma unroll
            for (int b = 0; b < JTK_U16_D_PER_LANE; b++) out[b] = (uint16_t)(g.w[b >> 2] >> (8 * (b & 3)) & 0xFFu);
        return JTK_U16_D_PER_LANE;
    }
    const uint32_t edges = edge_mask();
    const uint32_t w[6] = {prev, g.w[0], g.w[1], g.w[2], g.w[3], next};
    uint32_t n = 0;
#pragma unroll
    for (int b = 0; b < JTK_U16_D_PER_LANE; b++) {
        if (b >= left) continue;
        // bytes g0 + b - 3 .. g0 + b + 3 = bytes b + 1 .. b + 7 of w[]
        const int s = b + 1, k = s >> 2, r = 8 * (s & 3);
        const uint64_t a = (uint64_t)w[k] | (uint64_t)w[k + 1] << 32;
        const uint64_t c = k + 2 < 6 ? (uint64_t)w[k + 2 < 6 ? k + 2 : 0] : 0u;
        const uint64_t win = (r ? (a >> r | c << (64 - r)) : a) & 0x00FFFFFFFFFFFFFFull;
        int back, ahead;
        jtk_u16_d_avail(edges, b, &back, &ahead);
        uint16_t o[2];
        const int m = jtk_u16_d_emit(win, back, ahead, o);
        if (out) { if (m > 0) out[n] = o[0]; if (m > 1) out[n + 1] = o[1]; }
        n += (uint32_t)m;
    }
    return n;
}

#endif
