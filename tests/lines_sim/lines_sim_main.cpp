// lines_sim_main -- the shim of lines_sim.cpp as a stand-alone program for a sanitizer build (g++ -fsanitize=address,undefined):
// it catches a granule read past the text's end, a plane word outside the planes, a tile summary or carry outside its array, a
// unit written outside the list of exactly the counted size, a walk that leaves doc_off or status, a probe or an update
// outside the group's table, and a flag or per-document result outside its array.  Every record of the file argv[1] is loaded
// into heap buffers of EXACTLY the size the arrays have, and the results are written to argv[2] for the test to compare.  CPU
// only, never inside Python.
//   case file    per record int64 {n_docs, n_bytes, seed (its bits), doc_index_base (its bits), unit, flags, budget, order, n_units},
//                int64 doc_off[n_docs + 1], int32 status[n_docs], uint8 text[n_bytes]
//   result file  per record int64 begin[n_units], end[n_units], uint8 flags[n_units], int64 unit_off[n_docs + 1], int32 n_dup[n_docs],
//                int64 dup_bytes, dup_chars, unit_bytes, unit_chars, doc_chars [n_docs], int32 top_count[n_docs], int64 top_first[n_docs]
#include <stdio.h>
#include <stdlib.h>

#include "lines_sim.cpp"

template <class T>
static T* load(FILE* in, size_t n) {                        // exactly n items (NULL for none)
    if (n == 0) return nullptr;
    T* a = (T*)malloc(n * sizeof(T));
    if (!a || fread(a, sizeof(T), n, in) != n) exit(3);
    return a;
}
template <class T>
static T* room(size_t n) { return n ? (T*)malloc(n * sizeof(T)) : nullptr; }
static void put(FILE* out, const void* p, size_t size, size_t n) { if (n && fwrite(p, size, n, out) != n) exit(6); }

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: lines_sim_main cases.bin results.bin\n"); return 2; }
    FILE* in = fopen(argv[1], "rb");
    FILE* res = fopen(argv[2], "wb");
    if (!in || !res) { fprintf(stderr, "cannot open the files\n"); return 2; }
    int64_t hdr[9];
    int n_cases = 0;
    while (fread(hdr, 8, 9, in) == 9) {
        const size_t n = (size_t)hdr[0], nb = (size_t)hdr[1], nu = (size_t)hdr[8];
        int64_t* doc_off = load<int64_t>(in, n + 1);
        int32_t* status = load<int32_t>(in, n);
        uint8_t* text = load<uint8_t>(in, nb);
        int64_t *begin = room<int64_t>(nu), *end = room<int64_t>(nu), *unit_off = room<int64_t>(n + 1);
        uint8_t* flags = room<uint8_t>(nu);
        int32_t *n_dup = room<int32_t>(n), *top_count = room<int32_t>(n);
        int64_t* d64[6];
        for (auto& p : d64) p = room<int64_t>(n);
        int64_t info[4];
        const int rc = sim_ln_repeats(text, (int64_t)nb, doc_off, status, (int64_t)n, (uint64_t)hdr[2], (uint64_t)hdr[3], (int32_t)hdr[4], (uint32_t)hdr[5],
                                      hdr[6], (int)hdr[7], (uint64_t)n_cases, begin, end, flags, unit_off, n_dup, d64[0], d64[1], d64[2], d64[3], d64[4],
                                      top_count, d64[5], nullptr, info);
        if (rc || info[3] != (int64_t)nu) return 4;
        put(res, begin, 8, nu); put(res, end, 8, nu); put(res, flags, 1, nu); put(res, unit_off, 8, n + 1); put(res, n_dup, 4, n);
        for (int i = 0; i < 5; i++) put(res, d64[i], 8, n);
        put(res, top_count, 4, n); put(res, d64[5], 8, n);
        free(doc_off); free(status); free(text); free(begin); free(end); free(unit_off); free(flags); free(n_dup); free(top_count);
        for (auto& p : d64) free(p);
        n_cases++;
    }
    fclose(in);
    if (fclose(res) != 0) return 6;
    printf("%d cases\n", n_cases);
    return 0;
}
