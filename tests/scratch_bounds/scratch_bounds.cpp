// Prints what jtk_scratch_rules.h says, as JSON, for tests/test_scratch_bounds.py: the bin of every queued length, each bin's
// shortest piece and per-tile bound, the default numbers of scratch sets, and for every byte count given on the command line
// the tiles, the per-shard capacity of every bin and the bytes of one scratch set.  Host code only.
#include <cstdio>
#include <cstdlib>

#include "../../jtokkit_amd/csrc/jtk_kernels.h"

int main(int argc, char** argv) {
    printf("{\"tile\": %d, \"shards\": %d, \"nbins\": %d, \"tiny\": %d, \"maxlen\": %d,\n", JTK_TILE, JTK_Q_SHARDS, JTK_NBINS, JTK_BIN_TINY, JTK_BIN_MAXLEN);
    printf(" \"sets_default\": %d, \"sets_default_device\": %d, \"sets_max\": %d,\n", JTK_SETS_DEFAULT, JTK_SETS_DEFAULT_DEVICE, JTK_SETS_MAX);
    printf(" \"bin_of_len\": {");
    for (uint32_t len = 2; len <= JTK_BIN_MAXLEN; len++) printf("%s\"%u\": %u", len > 2 ? ", " : "", len, jtk_piece_bin(len));
    printf("},\n \"min_len\": [");
    for (int b = 0; b <= JTK_NBINS; b++) printf("%s%u", b ? ", " : "", jtk_bin_min_len(b));
    printf("],\n \"tile_cap\": [");
    for (int b = 0; b <= JTK_NBINS; b++) printf("%s%u", b ? ", " : "", jtk_bin_tile_cap(b));
    printf("],\n \"lds_cap\": [%d, %d, %d, %d, %d, %d, %d, %d],\n \"sizes\": {", JTK_BIN_CAP0, JTK_BIN_CAP1, JTK_BIN_CAP2, JTK_BIN_CAP3, JTK_BIN_CAP4,
           JTK_BIN_CAP5, JTK_BIN_CAP6, JTK_TINY_CAP);
    for (int i = 1; i < argc; i++) {
        const long long n = atoll(argv[i]);
        const JtkSetSizes z = jtk_set_sizes(n);
        printf("%s\"%lld\": {\"n_tiles\": %lld, \"queues\": %lld, \"total\": %lld, \"docpre\": %lld, \"plist\": %lld, \"htok\": %lld, \"shard_cap\": [", i > 1 ? ", " : "", n,
               (long long)z.n_tiles, (long long)z.queues, (long long)z.total(), (long long)z.docpre, (long long)z.plist, (long long)z.htok);
        for (int b = 0; b <= JTK_NBINS; b++) printf("%s%lld", b ? ", " : "", (long long)jtk_bin_shard_cap(b, z.n_tiles));
        printf("]}");
    }
    printf("}}\n");
    return 0;
}
