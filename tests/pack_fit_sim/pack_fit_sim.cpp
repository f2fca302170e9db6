// pack_fit_sim.cpp -- TEST INFRASTRUCTURE.  Runs the best-fit rule the device kernels use
// (jtokkit_amd/csrc/jtk_pack_fit_rules.h) on the CPU, so that the CPU test tier can check the batched step against the
// one-rest-at-a-time restatement (tests/pack_fit_ref.py).  The per-document passes of jtk_pack_fit.hip run here as loops and
// the radix sort is a stable sort; the driver, the record expansion and the cells are the header's functions, with a fresh
// cursor every `run` cells, as the lanes of the write kernel start theirs.  Nothing in the product loads this library.
#include <algorithm>
#include <cstdint>
#include <numeric>
#include <vector>

#include "../../jtokkit_amd/csrc/jtk_pack_fit_rules.h"

namespace {

struct Plan {
    std::vector<int64_t> FR, ITEM, SEGR;
    std::vector<int32_t> row_fill, item_doc, item_col;
    JtkFitView v{};
    int64_t n_rows = 0, n_seg = 0, longest = 0, steps = 0;
};

void plan(const int32_t* tokens, const int64_t* tok_off, const int32_t* status, int64_t n, int64_t L, int32_t sep_id,
          bool sep_first, Plan& p) {
    p.FR.assign(n + 1, 0); p.ITEM.assign(n + 1, 0); p.SEGR.assign(n + 1, 0);
    p.row_fill.assign(n + 1, 0); p.item_doc.assign(n + 1, 0); p.item_col.assign(n + 1, 0);
    std::vector<int64_t> key(n);
    for (int64_t d = 0; d < n; d++) {
        const int64_t l = jtk_pack_unit_len(tok_off[d + 1] - tok_off[d], status[d], sep_id);
        p.FR[d + 1] = p.FR[d] + l / L;
        key[d] = l % L ? L - l % L : L;
    }
    const int64_t F = p.FR[n];
    std::vector<int32_t> order(n);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return key[a] < key[b]; });
    int64_t R = 0;
    while (R < n && key[order[R]] < L) R++;
    // the driver
    std::vector<uint64_t> bits(JTK_FIT_WORDS, 0), sum(JTK_FIT_SUMS, 0);
    std::vector<int32_t> head(L + 1), tail(L + 1);
    std::vector<JtkFitRun> runs(2 * R + 1);
    std::vector<JtkFitRec> recs(R + 1);
    JtkFitState st{bits.data(), sum.data(), head.data(), tail.data(), runs.data(), recs.data(), L, 0, 0, 0};
    for (int64_t i = 0; i < R;) {
        int64_t j = i;
        while (j < R && key[order[j]] == key[order[i]]) j++;
        while (i < j) i += jtk_fit_step(st, L - key[order[i]], i, j - i);
    }
    p.steps = st.n_recs;
    const int64_t opened = st.next_row;
    p.longest = F > 0 ? L : (R > 0 ? L - key[order[0]] : 0);
    for (int32_t r = 0; r < st.n_runs; r++)
        for (int32_t t = 0; t < runs[r].count; t++) {
            const int64_t i = runs[r].row_lo + t;
            p.ITEM[i] = runs[r].pieces;
            p.SEGR[i] = runs[r].pieces + (runs[r].free > 0 ? 1 : 0);
            p.row_fill[i] = (int32_t)(L - runs[r].free);
            if (runs[r].free > p.longest) p.longest = runs[r].free;
        }
    int64_t a = 0, b = 0;
    for (int64_t i = 0; i <= n; i++) {
        const int64_t x = p.ITEM[i], y = p.SEGR[i];
        p.ITEM[i] = a; p.SEGR[i] = b;
        a += x; b += y;
    }
    for (int64_t i = 0; i < R; i++) {
        const JtkFitRec& rec = recs[jtk_fit_rec_of(recs.data(), st.n_recs, i)];
        const int64_t x = i - rec.slot, row = rec.row_lo + x / rec.per, at = p.ITEM[row] + rec.pieces + x % rec.per;
        p.item_doc[at] = order[i];
        p.item_col[at] = (int32_t)(L - rec.c + (x % rec.per) * rec.l);
    }
    p.n_rows = F + opened;
    p.n_seg = F + p.SEGR[n];
    JtkFitView& v = p.v;
    v.tokens = tokens; v.tok_off = tok_off; v.FR = p.FR.data(); v.ITEM = p.ITEM.data(); v.SEGR = p.SEGR.data();
    v.row_fill = p.row_fill.data(); v.item_doc = p.item_doc.data(); v.item_col = p.item_col.data();
    v.n = n; v.L = L; v.F = F; v.sep_id = sep_id; v.sep_first = sep_first && sep_id >= 0;
}

}  // namespace

extern "C" {

// counts[4] = (n_rows, n_segments, max_seqlen, steps of the driver)
void sim_fit_counts(const int32_t* tokens, const int64_t* tok_off, const int32_t* status, int64_t n, int64_t L, int32_t sep_id,
                    int sep_first, int64_t* counts) {
    Plan p;
    plan(tokens, tok_off, status, n, L, sep_id, sep_first != 0, p);
    counts[0] = p.n_rows; counts[1] = p.n_seg; counts[2] = p.longest; counts[3] = p.steps;
}

// The outputs, sized by sim_fit_counts: rows, positions [n_rows * L], cu_seqlens [n_seg + 1], seg_doc [n_seg].
void sim_fit(const int32_t* tokens, const int64_t* tok_off, const int32_t* status, int64_t n, int64_t L, int32_t sep_id,
             int sep_first, int32_t pad_id, int64_t run, int32_t* rows, int32_t* positions, int32_t* cu_seqlens, int64_t* seg_doc) {
    Plan p;
    plan(tokens, tok_off, status, n, L, sep_id, sep_first != 0, p);
    const int64_t total = p.n_rows * L;
    cu_seqlens[p.n_seg] = (int32_t)total;
    JtkFitCursor k{};
    k.rank = -1;
    for (int64_t x = 0; x < total; x++) {
        const int64_t r = x / L, c = x % L;
        if (c == 0 || (run > 0 && x % run == 0)) k.rank = -1;
        const JtkFitRow f = jtk_fit_row(p.v, r);
        const JtkPackCell cell = jtk_fit_cell(p.v, f, r, c, pad_id, k);
        rows[x] = cell.id;
        positions[x] = cell.pos;
        if (cell.start) { cu_seqlens[cell.seg] = (int32_t)x; seg_doc[cell.seg] = cell.doc; }
    }
}

}  // extern "C"
