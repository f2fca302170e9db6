// special_sim.cpp -- TEST INFRASTRUCTURE.  Runs the match selection of the allow-special encode the device kernels use
// (jtokkit_amd/csrc/jtk_special_rules.h) on the CPU -- candidates, the certain test, the chain walk --, so that the CPU test
// tier can check it against a restatement.  Nothing in the product loads this library.
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../jtokkit_amd/csrc/jtk_special_rules.h"

extern "C" {

// One document of n bytes; literal i = blob[off[i], off[i + 1]), allowed[i].  Writes kept match k as (s[k], e[k], lit[k])
// for k < cap and returns the match count; *dis = some literal outside the allowed set occurs in the document.
int64_t sim_special(const uint8_t* text, int64_t n, int n_lits, const uint32_t* off, const uint8_t* blob, const uint8_t* allowed,
                    int64_t* s, int64_t* e, int32_t* lit, int64_t cap, int32_t* dis) {
    auto at = [&](int64_t q) -> uint32_t { return text[q]; };
    int64_t maxlen = 0;
    for (int i = 0; i < n_lits; i++) if (allowed[i] && (int64_t)(off[i + 1] - off[i]) > maxlen) maxlen = off[i + 1] - off[i];
    std::vector<int64_t> cp, ce;
    std::vector<int32_t> cl;
    *dis = 0;
    for (int64_t p = 0; p < n; p++) {
        int len, idx;
        if (jtk_special_scan_at(p, n, at, n_lits, off, blob, allowed, &len, &idx)) *dis = 1;
        if (len > 0) { cp.push_back(p); ce.push_back(p + len); cl.push_back(idx); }
    }
    const int64_t nc = (int64_t)cp.size();
    auto fs = [&](int64_t k) { return cp[(size_t)k]; };
    auto fe = [&](int64_t k) { return ce[(size_t)k]; };
    std::vector<uint8_t> keep((size_t)nc, 0);
    for (int64_t i = 0; i < nc; i++) keep[(size_t)i] = jtk_special_certain(i, maxlen, fs, fe) ? 1 : 2;
    for (int64_t i = 0; i + 1 < nc; i++)
        if (keep[(size_t)i] == 1 && keep[(size_t)i + 1] != 1)
            jtk_special_walk(i, nc, fs, fe, [&](int64_t k) { return keep[(size_t)k] == 1; },
                             [&](int64_t k, bool kept) { keep[(size_t)k] = kept ? 3 : 0; });
    int64_t m = 0;
    for (int64_t i = 0; i < nc; i++) {
        if (keep[(size_t)i] != 1 && keep[(size_t)i] != 3) continue;
        if (m < cap) { s[m] = cp[(size_t)i]; e[m] = ce[(size_t)i]; lit[m] = cl[(size_t)i]; }
        m++;
    }
    return m;
}

// ---- the batch: what the kernels of jtk_special.hip do around the rule header, in plain loops, with one wrong rule switched in
// by `mutant` (0: none) so that the case set of tests/special_cases.py can show that it tells each from the right one.
enum {
    M_none = 0,
    M_batch_end = 1,      // the second scan is bounded by n_bytes, not by the document's end
    M_no_tail_mask = 2,   // the last granule's mask is off (its padding bytes are looked at); the scans keep their bounds
    M_doc_ge = 3,         // the document lookup is first->= instead of first-> minus one
    M_first_match = 4,    // the first allowed literal that matches, not the longest
    M_window = 5,         // the look-back window is s(j) > p - maxlen + 1
    M_chain_docs = 6,     // certain and walk see match ends bounded by the batch only: a document's first candidate is not
                          // certain after a straddling match, and the walk continues into it
    M_empty_at_self = 7,  // an unkept candidate's empty slots sit at its own position
    M_keep_j = 8,         // the gather never relocates once j is set
    M_pad_end = 9,        // M_no_tail_mask, and the batch ends where its last granule does (both scans)
};

namespace {

int64_t first_gt(const int64_t* a, int64_t lo, int64_t hi, int64_t x) { while (lo < hi && !(a[lo] > x)) lo++; return lo; }
int64_t first_ge(const int64_t* a, int64_t lo, int64_t hi, int64_t x) { while (lo < hi && !(a[lo] >= x)) lo++; return lo; }

struct Lits { int n; const uint32_t* off; const uint8_t* blob; const uint8_t* allowed; };

// the header's scan, or (first_match) the first allowed literal in table order
bool scan(const uint8_t* text, int64_t p, int64_t end, const Lits& L, bool first_match, int* len, int* lit) {
    auto at = [&](int64_t q) -> uint32_t { return text[q]; };
    bool dis = jtk_special_scan_at(p, end, at, L.n, L.off, L.blob, L.allowed, len, lit);
    if (!first_match || *len == 0) return dis;
    for (int i = 0; i < L.n; i++) {
        const int l = (int)(L.off[i + 1] - L.off[i]);
        if (!L.allowed[i] || l < 1 || p + l > end) continue;
        bool eq = true;
        for (int j = 0; j < l && eq; j++) eq = text[p + j] == L.blob[L.off[i] + j];
        if (eq) { *len = l; *lit = i; break; }
    }
    return dis;
}

}  // namespace

// A batch of n_docs documents, doc_off [n_docs + 1]; `text` is readable to the next multiple of 16 behind n_bytes, as device text
// is.  Writes the candidates in position order (cand_pos, cand_len, cand_lit = literal index, cand_doc, keep = 1 certain / 3 kept
// by a walk / 0 dropped; capacity cap), doc_first [n_docs], the n_docs + 2 * candidates sub-documents (sub_off [+1], sub_lit =
// literal index / -1 segment / -2 empty, sub_doc) and status [n_docs] (-2: a literal outside the allowed set, under check_dis).
// Returns the candidate count, -1 past cap.
int64_t sim_special_batch(const uint8_t* text, int64_t n_bytes, const int64_t* doc_off, int64_t n_docs, int n_lits, const uint32_t* off,
                          const uint8_t* blob, const uint8_t* allowed, int check_dis, int mutant, int64_t* cand_pos, int32_t* cand_len,
                          int32_t* cand_lit, int64_t* cand_doc, uint8_t* keep, int64_t cap, int64_t* doc_first, int64_t* sub_off,
                          int32_t* sub_lit, int64_t* sub_doc, int32_t* status) {
    const Lits L{n_lits, off, blob, allowed};
    uint32_t first[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int64_t maxlen = 0;
    for (int i = 0; i < n_lits; i++) {
        const int64_t l = (int64_t)(off[i + 1] - off[i]);
        if (allowed[i]) { if (l > maxlen) maxlen = l; }
        else if (!check_dis) continue;
        first[blob[off[i]] >> 5] |= 1u << (blob[off[i]] & 31);
    }
    for (int64_t d = 0; d < n_docs; d++) status[d] = 0;
    const int64_t pad_end = (n_bytes + 15) / 16 * 16;
    const int64_t batch_end = mutant == M_pad_end ? pad_end : n_bytes;
    std::vector<int64_t> end_b;            // per candidate: the end of the longest allowed match bounded by the batch only
    int64_t nc = 0;
    if (n_docs > 0)
        for (int64_t p0 = 0; p0 < n_bytes; p0 += 16) {
            uint32_t cand = 0;
            for (int j = 0; j < 16; j++) cand |= ((first[text[p0 + j] >> 5] >> (text[p0 + j] & 31)) & 1u) << j;
            const int64_t left = n_bytes - p0;
            if (left < 16 && mutant != M_no_tail_mask && mutant != M_pad_end) cand &= (1u << left) - 1u;
            for (int j = 0; j < 16; j++) {
                if (!((cand >> j) & 1u)) continue;
                const int64_t p = p0 + j;
                int len, lit;
                bool dis = scan(text, p, batch_end, L, mutant == M_first_match, &len, &lit);
                if (len == 0 && !(dis && check_dis)) continue;
                const int64_t e_batch = p + len;
                int64_t d = mutant == M_doc_ge ? first_ge(doc_off, 0, n_docs + 1, p) : first_gt(doc_off, 0, n_docs + 1, p) - 1;
                if (d < 0) d = 0;
                if (d > n_docs - 1) d = n_docs - 1;
                int64_t end = doc_off[d + 1] < n_bytes ? doc_off[d + 1] : batch_end;
                if (mutant == M_batch_end) end = n_bytes;
                dis = scan(text, p, end, L, mutant == M_first_match, &len, &lit);
                if (dis && check_dis) status[d] = -2;
                if (len == 0) continue;
                if (nc >= cap) return -1;
                cand_pos[nc] = p; cand_len[nc] = len; cand_lit[nc] = lit; cand_doc[nc] = d;
                end_b.push_back(e_batch);
                nc++;
            }
        }
    auto s = [&](int64_t k) { return cand_pos[k]; };
    auto e = [&](int64_t k) { return mutant == M_chain_docs ? end_b[(size_t)k] : cand_pos[k] + cand_len[k]; };
    for (int64_t i = 0; i < nc; i++) keep[i] = jtk_special_certain(i, mutant == M_window ? maxlen - 1 : maxlen, s, e) ? 1 : 2;
    for (int64_t i = 0; i + 1 < nc; i++)
        if (keep[i] == 1 && keep[i + 1] != 1)
            jtk_special_walk(i, nc, s, e, [&](int64_t k) { return keep[k] == 1; }, [&](int64_t k, bool kept) { keep[k] = kept ? 3 : 0; });
    auto kept = [&](int64_t i) { return keep[i] == 1 || keep[i] == 3; };
    const int64_t n_sub = n_docs + 2 * nc;
    sub_off[n_sub] = doc_off[n_docs];
    for (int64_t d = 0; d < n_docs; d++) {
        const int64_t f = d + 2 * first_ge(cand_pos, 0, nc, doc_off[d]);
        doc_first[d] = f;
        sub_off[f] = doc_off[d]; sub_lit[f] = -1; sub_doc[f] = d;
    }
    for (int64_t i = 0; i < nc; i++) {
        const int64_t d = cand_doc[i], a = d + 2 * i + 1;
        sub_doc[a] = sub_doc[a + 1] = d;
        if (kept(i)) {
            sub_off[a] = cand_pos[i]; sub_off[a + 1] = cand_pos[i] + cand_len[i];
            sub_lit[a] = cand_lit[i]; sub_lit[a + 1] = -1;
            continue;
        }
        int64_t j = i + 1;
        while (j < nc && cand_doc[j] == d && !kept(j)) j++;
        int64_t v = (j < nc && cand_doc[j] == d) ? cand_pos[j] : doc_off[d + 1];
        if (mutant == M_empty_at_self) v = cand_pos[i];
        sub_off[a] = sub_off[a + 1] = v;
        sub_lit[a] = sub_lit[a + 1] = -2;
    }
    return nc;
}

// The stitch over the sub-documents of sim_special_batch: seg_count [n_sub] = the tokens of each segment's encodeOrdinary (read for
// sub_lit == -1 only), status [n_docs] = the documents' final statuses.  Writes cnt [n_sub + 1] (the scanned counts), tok_off
// [n_docs + 1] and, for output token t < cap, its source (src_sub[t], src_idx[t]): found as the gather finds it, gt lanes a
// workgroup, gper tokens a lane at a stride of gt, n_bytes / (4 * gt * gper) + 1 workgroups in a grid-stride loop.  Returns the
// token total.
int64_t sim_special_stitch(int64_t n_sub, int64_t n_docs, const int32_t* sub_lit, const int64_t* sub_doc, const int32_t* status,
                           const int64_t* seg_count, const int64_t* doc_first, int64_t n_bytes, int gt, int gper, int mutant, int64_t* cnt,
                           int64_t* tok_off, int64_t* src_sub, int64_t* src_idx, int64_t cap) {
    int64_t run = 0;
    for (int64_t j = 0; j < n_sub; j++) {
        int64_t c = 0;
        if (status[sub_doc[j]] >= 0) c = sub_lit[j] >= 0 ? 1 : (sub_lit[j] == -2 ? 0 : seg_count[j]);
        cnt[j] = run;
        run += c;
    }
    cnt[n_sub] = run;
    const int64_t total = run;
    for (int64_t d = 0; d < n_docs; d++) tok_off[d] = cnt[doc_first[d]];
    tok_off[n_docs] = total;
    const int64_t grid = n_bytes / (4 * (int64_t)gt * gper) + 1, per = (int64_t)gt * gper;
    for (int64_t blk = 0; blk < grid; blk++)
        for (int lane = 0; lane < gt; lane++)
            for (int64_t base = blk * per; base < total; base += grid * per) {
                int64_t j = -1;
                for (int k = 0; k < gper; k++) {
                    const int64_t t = base + (int64_t)k * gt + lane;
                    if (t >= total) break;
                    if (j < 0 || (cnt[j + 1] <= t && mutant != M_keep_j)) j = first_gt(cnt, j < 0 ? 0 : j + 1, n_sub, t) - 1;
                    if (t < cap) { src_sub[t] = j; src_idx[t] = t - cnt[j]; }
                }
            }
    return total;
}

}  // extern "C"
