// repeat_sim_main -- the shim of repeat_sim.cpp as a stand-alone program for a sanitizer build (g++ -fsanitize=address,undefined):
// it catches an n-gram that reads past its document's last token or the batch's, a backward halo that reads before the group's
// first token, a walk that leaves tok_off or status, a probe or an atomic target that leaves the group's table, and a flag or
// per-document result outside its array.  Every record of the file argv[1] is loaded into heap buffers of EXACTLY the size the
// arrays have, the shim allocates every group's table at exactly its capacity, and the results are written to argv[2] for the
// test to compare.  CPU only, never inside Python.
//   case file    per record int64 {n_docs, n_tokens, seed (its bits), doc_index_base (its bits), ngram, mode, budget, order},
//                int64 tok_off[n_docs + 1], int32 status[n_docs], int32 tokens[n_tokens]
//   result file  per record uint8 flags[n_tokens], int32 n_repeat[n_docs], int32 n_covered[n_docs], int32 top_count[n_docs],
//                int64 top_first[n_docs]
#include <stdio.h>
#include <stdlib.h>

#include "repeat_sim.cpp"

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
    if (argc != 3) { fprintf(stderr, "usage: repeat_sim_main cases.bin results.bin\n"); return 2; }
    FILE* in = fopen(argv[1], "rb");
    FILE* res = fopen(argv[2], "wb");
    if (!in || !res) { fprintf(stderr, "cannot open the files\n"); return 2; }
    int64_t hdr[8];
    int n_cases = 0;
    while (fread(hdr, 8, 8, in) == 8) {
        const size_t n = (size_t)hdr[0], n_tok = (size_t)hdr[1];
        int64_t* tok_off = load<int64_t>(in, n + 1);
        int32_t* status = load<int32_t>(in, n);
        int32_t* tokens = load<int32_t>(in, n_tok);
        uint8_t* flags = room<uint8_t>(n_tok);
        int32_t* n_repeat = room<int32_t>(n);
        int32_t* n_covered = room<int32_t>(n);
        int32_t* top_count = room<int32_t>(n);
        int64_t* top_first = room<int64_t>(n);
        int64_t info[4];
        const int rc = sim_rp_repeats(tokens, tok_off, status, (int64_t)n, (uint64_t)hdr[2], (uint64_t)hdr[3], (int32_t)hdr[4], (uint32_t)hdr[5], hdr[6],
                                      (int)hdr[7], (uint64_t)n_cases, flags, n_repeat, n_covered, top_count, top_first, info);
        if (rc) return 4;
        put(res, flags, 1, n_tok); put(res, n_repeat, 4, n); put(res, n_covered, 4, n); put(res, top_count, 4, n); put(res, top_first, 8, n);
        free(tok_off); free(status); free(tokens); free(flags); free(n_repeat); free(n_covered); free(top_count); free(top_first);
        n_cases++;
    }
    fclose(in);
    if (fclose(res) != 0) return 6;
    printf("%d cases\n", n_cases);
    return 0;
}
