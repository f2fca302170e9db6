// stop_sim_main -- the shim of stop_sim.cpp as a stand-alone program for a sanitizer build (g++ -fsanitize=address,undefined):
// it catches the look-ahead reads that a search past a tile or a sequence invites.  Every case of the file argv[1] is loaded
// into heap buffers of EXACTLY the size the ABI documents as readable -- `out` up to the next multiple of 16 bytes, every other
// array its own length -- and the results are written to argv[2] for the test to compare.  CPU only, never inside Python.
//   case file    per case int64 {n_seqs, n_bytes, n_strings, has_from, width (0: no cell_byte)}, int64 byte_off[n_seqs + 1],
//                the bytes, uint32 str_off[n_strings + 1], the strings' bytes, int64 from[n_seqs] when has_from,
//                int64 cell_byte[n_seqs * width]
//   result file  per case int64 stop_pos[n_seqs], int32 stop_which[n_seqs], int32 hold[n_seqs], int64 stop_col[n_seqs]
#include <stdio.h>
#include <stdlib.h>

#include "stop_sim.cpp"

static size_t up16(size_t v) { return (v + 15) / 16 * 16; }

template <class T>
static T* load(FILE* in, size_t n) {                        // exactly n items (NULL for none)
    if (n == 0) return nullptr;
    T* a = (T*)malloc(n * sizeof(T));
    if (!a || fread(a, sizeof(T), n, in) != n) exit(3);
    return a;
}

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: stop_sim_main cases.bin results.bin\n"); return 2; }
    FILE* in = fopen(argv[1], "rb");
    FILE* res = fopen(argv[2], "wb");
    if (!in || !res) { fprintf(stderr, "cannot open the files\n"); return 2; }
    int64_t hdr[5];
    int n_cases = 0;
    while (fread(hdr, 8, 5, in) == 5) {
        const int64_t n = hdr[0], n_bytes = hdr[1], n_strings = hdr[2], has_from = hdr[3], width = hdr[4];
        int64_t* byte_off = load<int64_t>(in, (size_t)n + 1);
        uint8_t* out = n_bytes ? (uint8_t*)aligned_alloc(16, up16((size_t)n_bytes)) : nullptr;
        if (n_bytes) memset(out, 'a', up16((size_t)n_bytes));                                  // (bytes past the end must not count)
        if (n_bytes && fread(out, 1, (size_t)n_bytes, in) != (size_t)n_bytes) return 3;
        uint32_t* str_off = load<uint32_t>(in, (size_t)n_strings + 1);
        uint8_t* blob = load<uint8_t>(in, str_off[n_strings]);
        int64_t* from = has_from ? load<int64_t>(in, (size_t)n) : nullptr;
        int64_t* cell_byte = width ? load<int64_t>(in, (size_t)(n * width)) : nullptr;
        int64_t* pos = (int64_t*)malloc((size_t)(n ? n : 1) * 8);
        int64_t* col = (int64_t*)malloc((size_t)(n ? n : 1) * 8);
        int32_t* which = (int32_t*)malloc((size_t)(n ? n : 1) * 4);
        int32_t* hold = (int32_t*)malloc((size_t)(n ? n : 1) * 4);
        if (sim_find_stops(out, n_bytes, byte_off, n, blob, str_off, (int)n_strings, from, cell_byte, width, pos, which, hold, col) != 0) return 4;
        fwrite(pos, 8, (size_t)n, res); fwrite(which, 4, (size_t)n, res); fwrite(hold, 4, (size_t)n, res); fwrite(col, 8, (size_t)n, res);
        free(byte_off); free(out); free(str_off); free(blob); free(from); free(cell_byte); free(pos); free(col); free(which); free(hold);
        n_cases++;
    }
    fclose(in);
    if (fclose(res) != 0) return 6;
    printf("%d cases\n", n_cases);
    return 0;
}
