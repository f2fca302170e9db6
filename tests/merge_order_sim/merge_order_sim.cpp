// merge_order_sim -- jtokkit_amd/csrc/jtk_merge_order_rules.h on the CPU, a plain host program (built once as it is and once
// with -fsanitize=address,undefined by tests/test_merge_order_rules_cpu.py).  Reads commands from stdin, one per line:
//   order R nc k[0] ... k[64 R - 1]    -> "n_live perm[0] ... perm[64 R - 1]"     (k = nc: the entry needs no merge)
//   rounds left span                   -> "R"
//   class len lo nc                    -> "c"
//   const                              -> "JTK_MO_RMAX JTK_MO_W JTK_MO_NC_MAX"
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../jtokkit_amd/csrc/jtk_merge_order_rules.h"

int main() {
    char cmd[16];
    while (std::scanf("%15s", cmd) == 1) {
        if (!std::strcmp(cmd, "order")) {
            unsigned R, nc;
            if (std::scanf("%u %u", &R, &nc) != 2 || R < 1 || R > JTK_MO_RMAX || nc < 1 || nc > JTK_MO_NC_MAX) return 2;
            std::vector<uint8_t> key(64 * R);
            for (auto& k : key) {
                unsigned v;
                if (std::scanf("%u", &v) != 1 || v > nc) return 2;
                k = (uint8_t)v;
            }
            // exactly as large as the rule may write: a place beyond the window is an error the sanitizer build reports
            std::vector<uint16_t> place(64 * R, 0xFFFF), perm(64 * R, 0xFFFF);
            const uint32_t n_live = jtk_mo_order(key.data(), R, nc, place.data(), perm.data());
            std::string out = std::to_string(n_live);
            for (uint16_t p : perm) out += " " + std::to_string(p);
            std::puts(out.c_str());
        } else if (!std::strcmp(cmd, "rounds")) {
            unsigned left, span;
            if (std::scanf("%u %u", &left, &span) != 2) return 2;
            std::printf("%u\n", jtk_mo_rounds(left, span));
        } else if (!std::strcmp(cmd, "class")) {
            unsigned len, lo, nc;
            if (std::scanf("%u %u %u", &len, &lo, &nc) != 3) return 2;
            std::printf("%u\n", jtk_mo_class(len, lo, nc));
        } else if (!std::strcmp(cmd, "const")) {
            std::printf("%d %d %d\n", JTK_MO_RMAX, JTK_MO_W, JTK_MO_NC_MAX);
        } else {
            return 2;
        }
    }
    return 0;
}
