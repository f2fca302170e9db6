// utf16_sim_main -- the shim of utf16_sim.cpp as a stand-alone program for a sanitizer build (g++ -fsanitize=address,undefined):
// it catches the look-back and look-ahead reads that the two rules invite.  Every case of the file argv[1] is loaded into heap
// buffers of EXACTLY the size the ABI documents as readable -- E: the units up to the end of the 16-byte granule that holds the
// last one (16-byte aligned input), and the n_units units alone behind a pointer that is only 2-byte aligned; D: the bytes up to
// the next multiple of 16 -- both directions run, every output goes into a buffer of exactly its size, and the results are
// written to argv[2] for the test to compare.
//   case file    per case int64 {dir (0 E, 1 D), n, n_items}, int64 off[n + 1], then the items (uint16 / uint8)
//   result file  per case int64 total, int64 off[n + 1], then the output (uint8 / uint16)
#include <stdio.h>

#include "utf16_sim.cpp"

static size_t up16(size_t v) { return (v + 15) / 16 * 16; }

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: utf16_sim_main cases.bin results.bin\n"); return 2; }
    FILE* in = fopen(argv[1], "rb");
    FILE* res = fopen(argv[2], "wb");
    if (!in || !res) { fprintf(stderr, "cannot open the files\n"); return 2; }
    int64_t hdr[3];
    int n_cases = 0;
    while (fread(hdr, 8, 3, in) == 3) {
        const int64_t dir = hdr[0], n = hdr[1], n_items = hdr[2];
        std::vector<int64_t> off((size_t)n + 1), out_off((size_t)n + 1, -7);
        if (fread(off.data(), 8, (size_t)n + 1, in) != (size_t)n + 1) return 3;
        int64_t total;
        if (dir == 0) {
            uint16_t* a = n_items ? (uint16_t*)aligned_alloc(16, up16((size_t)n_items * 2)) : nullptr;
            uint16_t* raw = n_items ? (uint16_t*)malloc((size_t)n_items * 2 + 2) : nullptr;     // its units start one unit in
            if (n_items) memset(a, 0xDC, up16((size_t)n_items * 2));                              // (units past the end: low surrogates that must pair with nothing)
            if (n_items && fread(a, 2, (size_t)n_items, in) != (size_t)n_items) return 3;
            if (n_items) memcpy(raw + 1, a, (size_t)n_items * 2);
            total = sim_u16_encode(a, off.data(), n, n_items, 1, nullptr, 0, nullptr);
            if (total < 0) return 4;
            uint8_t* o1 = total ? (uint8_t*)malloc((size_t)total) : nullptr;
            uint8_t* o2 = total ? (uint8_t*)malloc((size_t)total) : nullptr;
            std::vector<int64_t> off2((size_t)n + 1, -7);
            if (sim_u16_encode(a, off.data(), n, n_items, 1, o1, total, out_off.data()) != total) return 4;
            if (sim_u16_encode(n_items ? raw + 1 : nullptr, off.data(), n, n_items, 0, o2, total, off2.data()) != total) return 4;
            if ((total && memcmp(o1, o2, (size_t)total) != 0) || off2 != out_off) { fprintf(stderr, "case %d: the alignments disagree\n", n_cases); return 5; }
            fwrite(&total, 8, 1, res); fwrite(out_off.data(), 8, (size_t)n + 1, res); if (total) fwrite(o1, 1, (size_t)total, res);
            free(a); free(raw); free(o1); free(o2);
        } else {
            uint8_t* a = n_items ? (uint8_t*)aligned_alloc(16, up16((size_t)n_items)) : nullptr;
            if (n_items) memset(a, 0xBF, up16((size_t)n_items));                                 // (bytes past the end must not count)
            if (n_items && fread(a, 1, (size_t)n_items, in) != (size_t)n_items) return 3;
            total = sim_u16_decode(a, off.data(), n, n_items, nullptr, 0, nullptr);
            uint16_t* o = total ? (uint16_t*)malloc((size_t)total * 2) : nullptr;
            if (sim_u16_decode(a, off.data(), n, n_items, o, total, out_off.data()) != total) return 4;
            fwrite(&total, 8, 1, res); fwrite(out_off.data(), 8, (size_t)n + 1, res); if (total) fwrite(o, 2, (size_t)total, res);
            free(a); free(o);
        }
        n_cases++;
    }
    fclose(in);
    if (fclose(res) != 0) return 6;
    printf("%d cases\n", n_cases);
    return 0;
}
