// label_sim.cpp -- TEST INFRASTRUCTURE.  Runs the label rule the device kernels use (jtokkit_amd/csrc/jtk_label_rules.h) on
// the CPU, so that the CPU test tier can check it against a restatement (tests/label_ref.py).  The span pass walks the tokens
// in lanes of `lane` tokens whose span cursor starts afresh, as the lanes of k_lb_spans do; the label pass walks the cells in
// lanes of `run` cells (0: one lane for all) with fresh cursors over heads and units, and with shift maps the cell after the
// lane's last one in the same lane, as k_lb_pack does.  The plan of the rows is pack_sim's.  Nothing in the product loads this
// library.
#include "../pack_sim/pack_sim.cpp"

#include "../../jtokkit_amd/csrc/jtk_label_rules.h"

extern "C" {

// tok_len[n_tok]: decoded length of every token; tok_off[n + 1], doc_off[n + 1]; out tok_span[n_tok]
void sim_tok_spans(const uint32_t* tok_len, const int64_t* tok_off, const int64_t* doc_off, int64_t n, const int64_t* begin,
                   const int64_t* end, int64_t n_spans, int rule, int64_t lane, int32_t* tok_span) {
    const int64_t n_tok = tok_off[n];
    std::vector<int64_t> p(n_tok + 1, 0);
    for (int64_t d = 0; d < n; d++) {
        int64_t pos = doc_off[d];
        for (int64_t t = tok_off[d]; t < tok_off[d + 1]; t++) { p[t] = pos; pos += tok_len[t]; }
    }
    int64_t cur = JTK_LB_FRESH;
    for (int64_t t = 0; t < n_tok; t++) {
        if (lane > 0 && t % lane == 0) cur = JTK_LB_FRESH;
        tok_span[t] = jtk_label_tok_span(begin, end, n_spans, rule, p[t], p[t] + tok_len[t], cur);
    }
}

// labels[n_rows * L] (sized by sim_pack_counts); tok_span may be NULL
void sim_labels(const int32_t* tokens, const int64_t* tok_off, const int32_t* status, int64_t n, int64_t L, int32_t sep_id,
                int sep_first, int whole, int drop, const int32_t* tok_span, int32_t ignore_index, int shift, int label_sep,
                int64_t run, int32_t* labels) {
    Plan p;
    plan(tokens, tok_off, status, n, L, sep_id, sep_first != 0, whole != 0, drop != 0, p);
    const int64_t total = p.n_rows * L;
    JtkLabelView lv;
    lv.tok_span = tok_span; lv.ignore_index = ignore_index; lv.label_sep = label_sep != 0;
    const int64_t step = run > 0 ? run : (total > 0 ? total : 1);
    std::vector<int32_t> lab;
    std::vector<int64_t> seg;
    for (int64_t x0 = 0; x0 < total; x0 += step) {
        const int64_t m = x0 + step <= total ? step : total - x0;
        lab.assign(m + 1, ignore_index); seg.assign(m + 1, -1);
        int64_t h = -1;
        JtkPackUnit u{};
        u.d = -1;
        for (int64_t j = 0; j < m + (shift ? 1 : 0); j++) {
            const int64_t x = x0 + j, r = x / L, c = x % L;
            if (x >= total || (j == m && c == 0)) continue;          // the extra cell only when it continues the row
            const JtkPackRow row = jtk_pack_row(p.v, r, h);
            const JtkPackCell cell = jtk_pack_cell(p.v, row, r, c, 0, u);
            lab[j] = jtk_label_cell(p.v, row, c, cell, u, lv);
            seg[j] = cell.seg;
        }
        for (int64_t j = 0; j < m; j++)
            labels[x0 + j] = shift ? jtk_label_shift((x0 + j) % L, L, seg[j], seg[j + 1], lab[j + 1], ignore_index) : lab[j];
    }
}

}  // extern "C"
