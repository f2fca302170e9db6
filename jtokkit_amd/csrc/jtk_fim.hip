// jtk_fim.hip -- fill-in-the-middle encode (JTK_ENCODE_FIM, orchestrated by jtk_abi.cpp): with probability fim_rate a document
// is cut at two random positions of its text into prefix, middle and suffix, which are encoded as encodeOrdinary() of each part
// and emitted around three sentinel ids in PSM or SPM order.  The rule is jtk_fim_rules.h; the four-kernel encode pipeline
// itself is untouched and runs on the sub-documents.
//
//   fim_cuts     one lane per offset: doc_off non-decreasing within [0, n_bytes], from 0 to n_bytes -> hdr[0]; per document
//                its kind and cuts (the draws and up to 6 bytes of text) and its three sub-documents
//   ... the encode pipeline on the 3 n_docs sub-documents (encodeOrdinary), then the stitch:
//   fim_count    one lane per document: the lowest of the three statuses, part_tok, its tokens in the result
//   scan         exclusive scan of the counts (jtk_launch_scan_i64) -> tok_off, n_tokens
//   fim_gather   tiles of JTK_FIM_TILE output cells, 4 per lane (one int4 store): a lane searches the document of its first
//                cell once per tile, from its cursor on, and moves forward; each cell comes from a part or is a sentinel
#include "jtk_device_prims.h"
#include "jtk_kernels.h"

namespace {

constexpr int FIM_MAX_BLOCKS = 4096;  // workgroups of the gather; each takes every gridDim.x-th tile

__global__ void __launch_bounds__(256) k_fim_cuts(JtkFimWork w) {
    const int64_t d = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (d > w.n_docs) return;
    // the offsets are caller memory: out-of-range or decreasing ones are reported (JTK_ERR_INVALID_ARGUMENT as the batch's
    // worst status), never followed
    if (jtk_fim_offset_bad(w.doc_off, w.n_docs, w.n_bytes, d)) {
        atomicMax((unsigned long long*)&w.hdr[0], 1ull);
        atomicMin(&w.result->worst_status, -1 /* JTK_ERR_INVALID_ARGUMENT */);
    }
    if (d == w.n_docs) { w.sub_off[3 * d] = w.doc_off[d]; return; }
    jtk_fim_cuts_doc(w.text, w.doc_off, w.n_bytes, d, w.seed, w.doc_index_base, w.fim_rate, w.spm_rate, w.kind, w.cut, w.sub_off);
}

__global__ void __launch_bounds__(256) k_fim_count(JtkFimWork w) {
    const int64_t d = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= w.n_docs) return;
    w.tok_off[d] = jtk_fim_count_doc(d, w.hdr[0] != 0, w.kind, w.sub_tok_off, w.sub_status, w.status, w.part_tok);
    if (w.status[d] < 0) atomicMin(&w.result->worst_status, w.status[d]);
}

__global__ void __launch_bounds__(256) k_fim_gather(JtkFimWork w) {
    const JtkFimView& v = w.v;
    const int64_t total = v.tok_off[v.n_docs];
    const int64_t n_tiles = (total + JTK_FIM_TILE - 1) / JTK_FIM_TILE;
    int64_t d = 0;
    for (int64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const int64_t e0 = t * JTK_FIM_TILE + threadIdx.x * 4;
        if (e0 >= total) break;
        int32_t id[4] = {0, 0, 0, 0};
        const int n = jtk_fim_cells4(v, e0, total, &d, id);
        int32_t* dst = w.tokens + e0;
        if (n == 4 && ((uintptr_t)dst & 15u) == 0) *reinterpret_cast<int4*>(dst) = make_int4(id[0], id[1], id[2], id[3]);
        else for (int j = 0; j < n; j++) dst[j] = id[j];
    }
}

}  // namespace

void jtk_launch_fim_cuts(const JtkFimWork& w, hipStream_t s) {
    hipLaunchKernelGGL(k_fim_cuts, dim3(jtk_blocks_for(w.n_docs + 1, 256)), dim3(256), 0, s, w);
}

void jtk_launch_fim_stitch(const JtkFimWork& w, hipStream_t s) {
    hipLaunchKernelGGL(k_fim_count, dim3(jtk_blocks_for(w.n_docs, 256)), dim3(256), 0, s, w);
    jtk_launch_scan_i64(w.tok_off, w.n_docs, &w.result->n_tokens, s);
    if (!w.count_only) {
        // (about one token per 4 bytes, three sentinels per document; the loop takes any total)
        int64_t g = (w.n_bytes / 4 + 3 * w.n_docs) / JTK_FIM_TILE + 1;
        if (g > FIM_MAX_BLOCKS) g = FIM_MAX_BLOCKS;
        hipLaunchKernelGGL(k_fim_gather, dim3((unsigned)g), dim3(256), 0, s, w);
    }
}
