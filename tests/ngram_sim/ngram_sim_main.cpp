// ngram_sim_main -- the shim of ngram_sim.cpp as a stand-alone program for a sanitizer build (g++ -fsanitize=address,undefined):
// it catches an n-gram that reads past its document's last token or the batch's, a backward halo that reads before token 0, a
// walk that leaves tok_off or status, a probe that leaves the table, and a flag or per-document result outside its array.  Every
// record of the file argv[1] is loaded into heap buffers of EXACTLY the size the arrays have -- the tokens their total, the
// table `capacity` slots -- and the results are written to argv[2] for the test to compare.  CPU only, never inside Python.
//   case file    per record int64 {n_docs, n_tokens, seed (its bits), ngram, n_keys, capacity, order, insert_batch},
//                int64 tok_off[n_docs + 1], int32 status[n_docs], int32 tokens[n_tokens], uint64 keys[n_keys].  The table gets
//                the keys, then (insert_batch != 0) every n-gram of the batch; the batch is then overlapped with it.
//   result file  per record int64 n_keys_in_table, uint64 the table's keys in ascending order, uint8 flags[n_tokens],
//                int32 n_hit[n_docs], int32 n_covered[n_docs], int64 first_hit[n_docs]
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>

#include "ngram_sim.cpp"

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
    if (argc != 3) { fprintf(stderr, "usage: ngram_sim_main cases.bin results.bin\n"); return 2; }
    FILE* in = fopen(argv[1], "rb");
    FILE* res = fopen(argv[2], "wb");
    if (!in || !res) { fprintf(stderr, "cannot open the files\n"); return 2; }
    int64_t hdr[8];
    int n_cases = 0;
    while (fread(hdr, 8, 8, in) == 8) {
        const size_t n = (size_t)hdr[0], n_tok = (size_t)hdr[1], n_keys = (size_t)hdr[4], cap = (size_t)hdr[5];
        const uint64_t seed = (uint64_t)hdr[2];
        const int32_t ngram = (int32_t)hdr[3];
        const int order = (int)hdr[6];
        int64_t* tok_off = load<int64_t>(in, n + 1);
        int32_t* status = load<int32_t>(in, n);
        int32_t* tokens = load<int32_t>(in, n_tok);
        uint64_t* keys = load<uint64_t>(in, n_keys);
        uint64_t* table = (uint64_t*)calloc(cap, 8);
        uint8_t* flags = room<uint8_t>(n_tok);
        int32_t* n_hit = room<int32_t>(n);
        int32_t* n_covered = room<int32_t>(n);
        int64_t* first_hit = room<int64_t>(n);
        if (!table) return 3;
        int64_t in_table = sim_ng_insert_keys(keys, (int64_t)n_keys, table, (int64_t)cap, (uint64_t)n_cases);
        if (hdr[7]) in_table += sim_ng_insert_batch(tokens, tok_off, status, (int64_t)n, seed, ngram, table, (int64_t)cap, order, (uint64_t)n_cases);
        if (sim_ng_overlap(tokens, tok_off, status, (int64_t)n, seed, ngram, table, (int64_t)cap, order, flags, n_hit, n_covered, first_hit) < 0) return 4;
        uint64_t* sorted = room<uint64_t>((size_t)in_table);
        size_t found = 0;
        for (size_t i = 0; i < cap; i++)
            if (table[i]) {
                if (found == (size_t)in_table) return 5;       // (more keys in the table than the inserts counted)
                sorted[found++] = table[i];
            }
        if (found != (size_t)in_table) return 5;
        std::sort(sorted, sorted + found);
        put(res, &in_table, 8, 1); put(res, sorted, 8, found); put(res, flags, 1, n_tok);
        put(res, n_hit, 4, n); put(res, n_covered, 4, n); put(res, first_hit, 8, n);
        free(tok_off); free(status); free(tokens); free(keys); free(table); free(flags); free(n_hit); free(n_covered); free(first_hit); free(sorted);
        n_cases++;
    }
    fclose(in);
    if (fclose(res) != 0) return 6;
    printf("%d cases\n", n_cases);
    return 0;
}
