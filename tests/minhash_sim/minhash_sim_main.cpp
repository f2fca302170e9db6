// minhash_sim_main -- the shim of minhash_sim.cpp as a stand-alone program for a sanitizer build (g++
// -fsanitize=address,undefined): it catches a shingle that reads past its document's last token or the batch's, a walk that
// leaves tok_off or status, and a flush outside a signature row.  Every case of the file argv[1] is loaded into heap buffers of
// EXACTLY the size the arrays have -- the tokens their total, the signatures n_docs * K words -- and the results are written to
// argv[2] for the test to compare.  CPU only, never inside Python.
//   case file    per case int64 {n_docs, n_tokens, seed (its bits), ngram, num_hashes, bands, n_pairs}, int64 tok_off[n_docs + 1],
//                int32 status[n_docs], int32 tokens[n_tokens], int64 pair_a[n_pairs], int64 pair_b[n_pairs]
//   result file  per case uint32 sig[n_docs * num_hashes], int32 n_shingles[n_docs], uint64 band_keys[n_docs * bands],
//                int32 agree[n_pairs]
#include <stdio.h>
#include <stdlib.h>

#include "minhash_sim.cpp"

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
    if (argc != 3) { fprintf(stderr, "usage: minhash_sim_main cases.bin results.bin\n"); return 2; }
    FILE* in = fopen(argv[1], "rb");
    FILE* res = fopen(argv[2], "wb");
    if (!in || !res) { fprintf(stderr, "cannot open the files\n"); return 2; }
    int64_t hdr[7];
    int n_cases = 0;
    while (fread(hdr, 8, 7, in) == 7) {
        const size_t n = (size_t)hdr[0], n_tok = (size_t)hdr[1], K = (size_t)hdr[4], bands = (size_t)hdr[5], n_pairs = (size_t)hdr[6];
        int64_t* tok_off = load<int64_t>(in, n + 1);
        int32_t* status = load<int32_t>(in, n);
        int32_t* tokens = load<int32_t>(in, n_tok);
        int64_t* pair_a = load<int64_t>(in, n_pairs);
        int64_t* pair_b = load<int64_t>(in, n_pairs);
        uint32_t* sig = room<uint32_t>(n * K);
        int32_t* n_shingles = room<int32_t>(n);
        uint64_t* band_keys = room<uint64_t>(n * bands);
        int32_t* agree = room<int32_t>(n_pairs);
        if (sim_mh_batch(tokens, tok_off, status, (int64_t)n, (uint64_t)hdr[2], (int32_t)hdr[3], (int32_t)K, (int32_t)bands, n_cases & 1, sig,
                         n_shingles, band_keys) < 0) return 4;
        sim_mh_agree(sig, (int64_t)n, (int32_t)K, pair_a, pair_b, (int64_t)n_pairs, agree);
        put(res, sig, 4, n * K); put(res, n_shingles, 4, n); put(res, band_keys, 8, n * bands); put(res, agree, 4, n_pairs);
        free(tok_off); free(status); free(tokens); free(pair_a); free(pair_b); free(sig); free(n_shingles); free(band_keys); free(agree);
        n_cases++;
    }
    fclose(in);
    if (fclose(res) != 0) return 6;
    printf("%d cases\n", n_cases);
    return 0;
}
