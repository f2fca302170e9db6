// pack_sim.cpp -- TEST INFRASTRUCTURE.  Runs the packing rule the device kernels use (jtokkit_amd/csrc/jtk_pack_rules.h) on
// the CPU, so that the CPU test tier can check it against a restatement (tests/pack_ref.py).  The per-document passes of
// jtk_pack.hip run here as loops and the chain of row groups is walked serially (the kernels find it by binary lifting);
// the cells are produced by the header's row and cell functions with fresh cursors every `run` cells, as the lanes of the
// write kernel start theirs.  Nothing in the product loads this library.
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../jtokkit_amd/csrc/jtk_pack_rules.h"

namespace {

struct Plan {
    std::vector<int64_t> P, SEG, RS;
    std::vector<uint8_t> flag;
    std::vector<int32_t> nxt;
    JtkPackView v{};
    int64_t n_rows = 0, n_seg = 0, longest = 0;
};

void plan(const int32_t* tokens, const int64_t* tok_off, const int32_t* status, int64_t n, int64_t L, int32_t sep_id,
          bool sep_first, bool whole, bool drop, Plan& p) {
    p.P.assign(n + 1, 0); p.SEG.assign(n + 1, 0); p.RS.assign(n + 1, 0); p.flag.assign(n + 1, 0); p.nxt.assign(n + 1, (int32_t)n);
    for (int64_t d = 0; d < n; d++) p.P[d + 1] = p.P[d] + jtk_pack_unit_len(tok_off[d + 1] - tok_off[d], status[d], sep_id);
    const int64_t S = p.P[n];
    std::vector<int64_t> cnt(n, 0);
    if (!whole) {
        p.n_rows = jtk_pack_concat_rows(S, L, drop);
        const int64_t K = p.n_rows * L;
        for (int64_t d = 0; d < n; d++) {
            cnt[d] = jtk_pack_concat_segs(p.P[d], p.P[d + 1], L, K);
            const int64_t m = jtk_pack_concat_max(p.P[d], p.P[d + 1], L, K);
            if (m > p.longest) p.longest = m;
        }
    } else {
        for (int64_t d = 0; d < n; d++)
            if (p.P[d + 1] > p.P[d]) p.nxt[d] = (int32_t)jtk_pack_next_head(p.P.data(), n, d, L);
        int64_t h = 0;
        while (h < n && p.P[h + 1] == p.P[h]) h++;
        for (; h < n; h = p.nxt[h]) {
            p.flag[h] |= JTK_PK_HEAD;
            const int64_t nx = p.nxt[h], pad = jtk_pack_group_pad(p.P.data(), h, nx, L);
            if (pad > 0) p.flag[jtk_pack_last_le(p.P.data(), h, nx - 1, p.P[nx] - 1)] |= JTK_PK_PAD_AFTER;
            if (pad > p.longest) p.longest = pad;
        }
        for (int64_t d = 0; d < n; d++) {
            const int64_t l = p.P[d + 1] - p.P[d];
            const bool head = (p.flag[d] & JTK_PK_HEAD) != 0;
            p.RS[d + 1] = p.RS[d] + (head ? jtk_pack_unit_rows(l, L) : 0);
            cnt[d] = (l > 0 ? (head ? jtk_pack_unit_rows(l, L) : 1) : 0) + ((p.flag[d] & JTK_PK_PAD_AFTER) ? 1 : 0);
            const int64_t m = l < L ? l : L;
            if (m > p.longest) p.longest = m;
        }
        p.n_rows = p.RS[n];
    }
    for (int64_t d = 0; d < n; d++) p.SEG[d + 1] = p.SEG[d] + cnt[d];
    p.n_seg = p.SEG[n];
    if (!whole && p.n_rows * L > S) {
        p.n_seg++;
        if (p.n_rows * L - S > p.longest) p.longest = p.n_rows * L - S;
    }
    JtkPackView& v = p.v;
    v.tokens = tokens; v.tok_off = tok_off; v.P = p.P.data(); v.SEG = p.SEG.data(); v.RS = p.RS.data(); v.flag = p.flag.data();
    v.nxt = p.nxt.data(); v.n = n; v.L = L; v.sep_id = sep_id; v.sep_first = sep_first && sep_id >= 0; v.whole = whole;
}

}  // namespace

extern "C" {

// counts[3] = (n_rows, n_segments, max_seqlen)
void sim_pack_counts(const int32_t* tokens, const int64_t* tok_off, const int32_t* status, int64_t n, int64_t L, int32_t sep_id,
                     int sep_first, int whole, int drop, int64_t* counts) {
    Plan p;
    plan(tokens, tok_off, status, n, L, sep_id, sep_first != 0, whole != 0, drop != 0, p);
    counts[0] = p.n_rows; counts[1] = p.n_seg; counts[2] = p.longest;
}

// The outputs, sized by sim_pack_counts: rows, positions [n_rows * L], cu_seqlens [n_seg + 1], seg_doc [n_seg].
void sim_pack(const int32_t* tokens, const int64_t* tok_off, const int32_t* status, int64_t n, int64_t L, int32_t sep_id,
              int sep_first, int whole, int drop, int32_t pad_id, int64_t run, int32_t* rows, int32_t* positions,
              int32_t* cu_seqlens, int64_t* seg_doc) {
    Plan p;
    plan(tokens, tok_off, status, n, L, sep_id, sep_first != 0, whole != 0, drop != 0, p);
    const int64_t total = p.n_rows * L;
    cu_seqlens[p.n_seg] = (int32_t)total;
    int64_t h = -1;
    JtkPackUnit u{};
    u.d = -1;
    for (int64_t x = 0; x < total; x++) {
        if (run > 0 && x % run == 0) { h = -1; u.d = -1; }
        const int64_t r = x / L, c = x % L;
        const JtkPackRow row = jtk_pack_row(p.v, r, h);
        const JtkPackCell cell = jtk_pack_cell(p.v, row, r, c, pad_id, u);
        rows[x] = cell.id;
        positions[x] = cell.pos;
        if (cell.start) { cu_seqlens[cell.seg] = (int32_t)x; seg_doc[cell.seg] = cell.doc; }
    }
}

}  // extern "C"
