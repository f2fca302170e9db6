// validate_sim_main -- the shim of validate_sim.cpp as a stand-alone program for a sanitizer build (g++ -fsanitize=address,undefined):
// it catches the look-back (p - 1 .. p - 3) and look-ahead (p + 1 .. p + 3) reads that the rule invites at the first and last
// bytes of a batch.  Every case of the file argv[1] is loaded into a heap buffer of EXACTLY n_bytes, run chunk by chunk, and the
// statuses are written to argv[2] for the test to compare.
//   case file    per case int64 {n_docs, n_bytes, n_chunks, tile}, int64 doc_off[n_docs + 1], int64 chunk_doc[n_chunks + 1], the text
//   result file  per case int32 status[n_docs]
#include <stdio.h>

#include "validate_sim.cpp"

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: validate_sim_main cases.bin results.bin\n"); return 2; }
    FILE* in = fopen(argv[1], "rb");
    FILE* res = fopen(argv[2], "wb");
    if (!in || !res) { fprintf(stderr, "cannot open the files\n"); return 2; }
    int64_t hdr[4];
    int n_cases = 0;
    while (fread(hdr, 8, 4, in) == 4) {
        const int64_t n_docs = hdr[0], n_bytes = hdr[1], n_chunks = hdr[2], tile = hdr[3];
        std::vector<int64_t> off((size_t)n_docs + 1), chunk_doc((size_t)n_chunks + 1);
        if (fread(off.data(), 8, off.size(), in) != off.size() || fread(chunk_doc.data(), 8, chunk_doc.size(), in) != chunk_doc.size()) return 3;
        uint8_t* text = n_bytes ? (uint8_t*)malloc((size_t)n_bytes) : nullptr;
        if (n_bytes && fread(text, 1, (size_t)n_bytes, in) != (size_t)n_bytes) return 3;
        std::vector<int32_t> status((size_t)n_docs, 0);
        for (int64_t c = 0; c < n_chunks; c++)
            if (sim_validate_chunk(text, off.data(), chunk_doc[(size_t)c], chunk_doc[(size_t)c + 1], tile, status.data()) != 0) return 4;
        if (n_docs) fwrite(status.data(), 4, (size_t)n_docs, res);
        free(text);
        n_cases++;
    }
    fclose(in);
    if (fclose(res) != 0) return 6;
    printf("%d cases\n", n_cases);
    return 0;
}
