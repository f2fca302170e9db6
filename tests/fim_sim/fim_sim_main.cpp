// fim_sim_main -- the shim of fim_sim.cpp as a stand-alone program for a sanitizer build (g++ -fsanitize=address,undefined): it
// catches a cut that reads a byte outside its document's text and a gather that leaves its arrays.  Every case of the file
// argv[1] is loaded into heap buffers of EXACTLY the size the arrays have -- the text n_bytes, the result's tokens their total --
// and the results are written to argv[2] for the test to compare.  CPU only, never inside Python.
//   case file    per case int64 {n_docs, n_bytes, n_sub_tokens, seed (its bits), doc_index_base, fim_rate, spm_rate, prefix_id,
//                middle_id, suffix_id}, int64 doc_off[n_docs + 1], the bytes, and the sub-documents' encode: int64
//                sub_tok_off[3 n_docs + 1], int32 sub_status[3 n_docs], int32 sub_tokens[n_sub_tokens]
//   result file  per case uint8 kind[n_docs], int64 cut[2 n_docs], int64 sub_off[3 n_docs + 1], int32 status[n_docs], int64
//                part_tok[3 n_docs], int64 tok_off[n_docs + 1], int32 tokens[tok_off[n_docs]]
#include <stdio.h>
#include <stdlib.h>

#include "fim_sim.cpp"

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
    if (argc != 3) { fprintf(stderr, "usage: fim_sim_main cases.bin results.bin\n"); return 2; }
    FILE* in = fopen(argv[1], "rb");
    FILE* res = fopen(argv[2], "wb");
    if (!in || !res) { fprintf(stderr, "cannot open the files\n"); return 2; }
    int64_t hdr[10];
    int n_cases = 0;
    while (fread(hdr, 8, 10, in) == 10) {
        const size_t n = (size_t)hdr[0], n_bytes = (size_t)hdr[1], n_sub_tok = (size_t)hdr[2];
        int64_t* doc_off = load<int64_t>(in, n + 1);
        uint8_t* text = load<uint8_t>(in, n_bytes);
        int64_t* sub_tok_off = load<int64_t>(in, 3 * n + 1);
        int32_t* sub_status = load<int32_t>(in, 3 * n);
        int32_t* sub_tokens = load<int32_t>(in, n_sub_tok);
        uint8_t* kind = room<uint8_t>(n);
        int64_t* cut = room<int64_t>(2 * n);
        int64_t* sub_off = room<int64_t>(3 * n + 1);
        int32_t* status = room<int32_t>(n);
        int64_t* part_tok = room<int64_t>(3 * n);
        int64_t* tok_off = room<int64_t>(n + 1);
        const int bad = sim_fim_cuts(text, doc_off, (int64_t)n, (int64_t)n_bytes, (uint64_t)hdr[3], hdr[4], (uint32_t)hdr[5], (uint32_t)hdr[6],
                                     kind, cut, sub_off);
        if (bad) return 4;
        const int64_t total = sim_fim_stitch((int64_t)n, bad, kind, sub_tok_off, sub_status, sub_tokens, (int32_t)hdr[7], (int32_t)hdr[8],
                                             (int32_t)hdr[9], 1, status, part_tok, tok_off, nullptr);
        int32_t* tokens = room<int32_t>((size_t)total);                // (NULL for an empty result: nothing is gathered)
        if (sim_fim_stitch((int64_t)n, bad, kind, sub_tok_off, sub_status, sub_tokens, (int32_t)hdr[7], (int32_t)hdr[8], (int32_t)hdr[9],
                           3, status, part_tok, tok_off, tokens) != total) return 5;
        put(res, kind, 1, n); put(res, cut, 8, 2 * n); put(res, sub_off, 8, 3 * n + 1); put(res, status, 4, n);
        put(res, part_tok, 8, 3 * n); put(res, tok_off, 8, n + 1); put(res, tokens, 4, (size_t)total);
        free(doc_off); free(text); free(sub_tok_off); free(sub_status); free(sub_tokens); free(kind); free(cut); free(sub_off);
        free(status); free(part_tok); free(tok_off); free(tokens);
        n_cases++;
    }
    fclose(in);
    if (fclose(res) != 0) return 6;
    printf("%d cases\n", n_cases);
    return 0;
}
