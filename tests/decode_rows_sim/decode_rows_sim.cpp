// decode_rows_sim.cpp -- TEST INFRASTRUCTURE.  Runs the rule of the id-matrix decode that the device kernels use
// (jtokkit_amd/csrc/jtk_decode_rows_rules.h) serially on the CPU, so that the CPU test tier can check it against a restatement
// (tests/decode_rows_ref.py): the first stop column of every row by walking its window, then the cells in row-major order.
// Nothing in the product loads this library.
#include <cstdint>
#include <cstring>

#include "../../jtokkit_amd/csrc/jtk_decode_rows_rules.h"

namespace {
int64_t cell_id(const void* rows, int id_bytes, int64_t at) {
    return id_bytes == 8 ? ((const int64_t*)rows)[at] : (int64_t)((const int32_t*)rows)[at];
}
}  // namespace

extern "C" {

int sim_dr_max_stop() { return JTK_DR_MAX_STOP; }

// -> total bytes; out (may be NULL: sizes only) holds them when cap suffices.  byte_off[n_rows + 1], status[n_rows],
// cell_byte[n_rows * width], first_stop[n_rows] (-1: none).  tab_off[n_ids_table + 1] / tab_blob: the decode table.
int64_t sim_decode_rows(const void* rows, int id_bytes, int64_t n_rows, int64_t width, int64_t row_stride, const int64_t* begin,
                        const int64_t* end, int64_t pad_id, const int64_t* stop, int n_stop, int skip_pad, int keep_stop,
                        const uint32_t* tab_off, const uint8_t* tab_blob, uint32_t n_ids_table, uint8_t* out, int64_t cap,
                        int64_t* byte_off, int32_t* status, int64_t* cell_byte, int64_t* first_stop) {
    JtkDecodeRowsRule rule{};
    rule.pad_id = pad_id; rule.n_stop = n_stop; rule.skip_pad = skip_pad != 0; rule.keep_stop = keep_stop != 0;
    for (int k = 0; k < n_stop; k++) rule.stop[k] = stop[k];
    int64_t n = 0;
    for (int64_t r = 0; r < n_rows; r++) {
        const JtkDecodeRowsSpan win = jtk_dr_window(begin, end, r, width);
        uint64_t first = JTK_DR_NO_STOP;
        for (int64_t c = win.b; c < win.e && first == JTK_DR_NO_STOP; c++)
            if (jtk_dr_is_stop(rule, cell_id(rows, id_bytes, r * row_stride + c))) first = (uint64_t)c;
        first_stop[r] = first == JTK_DR_NO_STOP ? -1 : (int64_t)first;
        const JtkDecodeRowsSpan span = jtk_dr_cut(win, first, rule.keep_stop);
        byte_off[r] = n;
        status[r] = 0;
        for (int64_t c = 0; c < width; c++) {
            const int64_t id = cell_id(rows, id_bytes, r * row_stride + c);
            bool unknown = false;
            const uint32_t l = jtk_dr_cell_len(rule, tab_off, n_ids_table, id, c, span, &unknown);
            if (unknown) status[r] = -3;                                   // JTK_ERR_UNKNOWN_TOKEN
            cell_byte[r * width + c] = n;
            if (l && out && n + l <= cap) memcpy(out + n, tab_blob + tab_off[id], l);
            n += l;
        }
    }
    byte_off[n_rows] = n;
    return n;
}

}
