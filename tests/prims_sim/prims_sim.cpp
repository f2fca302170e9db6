// prims_sim.cpp -- TEST INFRASTRUCTURE.  Runs the host-compilable primitives of jtokkit_amd/csrc/jtk_device_prims.h on the CPU:
// the two offset searches, the token length, and the document lookups of the kernels, each written here exactly as its kernel
// calls the shared search (clamping and meaning at the call site).  The mutants are wrong on purpose: the CPU test must tell
// each of them from the real thing.  Nothing in the product loads this library.
#include <cstddef>
#include <cstdint>

#include "../../jtokkit_amd/csrc/jtk_device_prims.h"

extern "C" {

int64_t sim_first_gt(const int64_t* a, int64_t lo, int64_t hi, int64_t x) { return jtk_first_gt(a, lo, hi, x); }
int64_t sim_first_ge(const int64_t* a, int64_t lo, int64_t hi, int64_t x) { return jtk_first_ge(a, lo, hi, x); }
uint32_t sim_tok_len(const uint32_t* tab_off, uint32_t n_ids_table, int32_t id, uint32_t unknown) {
    return jtk_tok_len(tab_off, n_ids_table, id, unknown);
}
uint32_t sim_blocks_for(int64_t n, int per) { return jtk_blocks_for(n, per); }

// find_doc of jtk_kernels.hip: p is a position in the chunk, doc_off holds positions in the whole batch
int64_t sim_find_doc(const int64_t* doc_off, int64_t n_docs, int64_t text_base, int64_t p) {
    return jtk_first_gt(doc_off, 0, n_docs, p + text_base) - 1;
}
// sp_find_doc of jtk_special.hip: clamped to a valid index
int64_t sim_sp_find_doc(const int64_t* doc_off, int64_t n_docs, int64_t p) {
    int64_t d = jtk_first_gt(doc_off, 0, n_docs + 1, p) - 1;
    if (d < 0) d = 0;
    if (d > n_docs - 1) d = n_docs - 1;
    return d;
}
// mt_doc_of of jtk_maxtok.hip: the document holding [p, p + len) whole, or -1
int64_t sim_mt_doc_of(const int64_t* doc_off, int64_t n_docs, int64_t p, int64_t len) {
    const int64_t d = jtk_first_gt(doc_off, 0, n_docs, p) - 1;
    return (d >= 0 && p + len <= doc_off[d + 1]) ? d : -1;
}
// ck_doc_of of jtk_chunk.hip and lb_doc_of of jtk_label.hip (and k_flag_unencodable): the last d in [0, n_docs) with
// tok_off[d] <= t
int64_t sim_ck_doc_of(const int64_t* tok_off, int64_t n_docs, int64_t t) { return jtk_first_gt(tok_off, 1, n_docs, t) - 1; }
int64_t sim_lb_doc_of(const int64_t* tok_off, int64_t n_docs, int64_t t) { return jtk_first_gt(tok_off, 1, n_docs, t) - 1; }

// ---- mutants
// kind 0: >= for >;  1: hi = mid - 1 (drops the candidate);  2: lo = mid (never passes an equal run; bounded here);
// 3: the range without its first entry
int64_t sim_first_gt_mutant(int kind, const int64_t* a, int64_t lo, int64_t hi, int64_t x) {
    if (kind == 0) return jtk_first_ge(a, lo, hi, x);
    if (kind == 3) return jtk_first_gt(a, lo < hi ? lo + 1 : lo, hi, x);
    for (int guard = 0; lo < hi && guard < 128; guard++) {
        const int64_t mid = (lo + hi) >> 1;
        if (a[mid] > x) hi = kind == 1 ? mid - 1 : mid;
        else lo = kind == 2 ? mid : mid + 1;
    }
    return lo;
}
// kind 0: > for >=;  1: the range without its last entry
int64_t sim_first_ge_mutant(int kind, const int64_t* a, int64_t lo, int64_t hi, int64_t x) {
    if (kind == 0) return jtk_first_gt(a, lo, hi, x);
    return jtk_first_ge(a, lo, hi > lo ? hi - 1 : hi, x);
}
// the token-document lookup over [0, n_docs) instead of [1, n_docs): -1 for a token before tok_off[0]
int64_t sim_ck_doc_of_mutant(const int64_t* tok_off, int64_t n_docs, int64_t t) { return jtk_first_gt(tok_off, 0, n_docs, t) - 1; }
// sp_find_doc without its clamp
int64_t sim_sp_find_doc_mutant(const int64_t* doc_off, int64_t n_docs, int64_t p) { return jtk_first_gt(doc_off, 0, n_docs + 1, p) - 1; }

}  // extern "C"
