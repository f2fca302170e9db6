// jtk_pack_fit.hip -- best-fit-decreasing packing of the last batch encode into rows of L tokens (jtk_batch_pack_best_fit in
// jtk_abi.cpp), by the rule of jtk_pack_fit_rules.h.  The rows are gathers of pieces from all over the batch, so neither the
// plan nor the cell walk of jtk_pack.hip (row r = one slice of the document stream) serves them.
//
//   plan   pf_len         per document: full pieces -> FR, key = L - rest (L without a rest), val = the document; scan -> F
//          sort           LSD radix sort of (key, val), 8 bits a pass, ceil(bits(L) / 8) passes, three launches each:
//            pf_hist        per tile of 1024 keys the 256 digit counts (LDS), stored digit-major
//            scan           jtk_launch_scan_i64 over (digit, tile): where each tile's keys of each digit begin
//            pf_scatter     a wave owns 256 consecutive keys of the tile and takes them 64 at a time.  Per-wave digit counts
//                           in LDS, prefixed over the waves on top of the scanned base; then a lane's rank among the lanes of
//                           its round with the same digit comes from 8 ballots (one per digit bit: the peers mask), and the
//                           peers' first lane moves the wave's offset on.  Order inside the tile is kept: the sort is stable.
//          pf_bounds      sorted slot i opens a new length when its key differs from slot i - 1's; R = the slots with a rest;
//          scan, pf_distinct   the distinct lengths, longest first, and the first slot of each
//          pf_drive       ONE workgroup of one wave.  The class bitmap (32 KiB + a summary level of 64 words, so a search is
//                         one word, one summary word and at most L / 4096 more) lives in LDS, cleared by all lanes; lane 0
//                         then walks the distinct lengths and calls jtk_fit_step until each length's rests are placed.
//                         Queue heads and tails, runs and records are in global memory.  The walk is serial in the number
//                         of steps, not of documents: a few thousand steps per million documents of a typical corpus, one
//                         step per document when all rests are distinct and longer than L / 2.
//          pf_rows        a wave per run, lanes over its rows: pieces, segments (pieces + 1 with pad) and fill of every opened
//                         row; two scans -> ITEM (CSR of the rows' pieces) and SEGR (first segment)
//          pf_expand      one lane per sorted rest: its record by binary search over the records' first slots, then row, rank
//                         and column in closed form -> item_doc / item_col at ITEM[row] + rank.  No atomics: the layout is
//                         the same on every run.
//   write  pf_write       row-centric as pk_write: a lane owns 4 consecutive cells (one int4 store of ids and one of positions
//                         where aligned), finds its row by division and its piece by one binary search over the row's CSR
//                         columns, then moves forward (jtk_fit_cell); segment records by the lane that holds a segment's
//                         first cell.  Rows below F hold one full piece.
//   labels pf_labels      the same cell walk with jtk_label_cell per cell; with shift a lane also maps the cell after its
//                         fourth, as lb_pack does.
// Scratch per document: FR, DF, ITEM, SEGR (8 B each), two (key, val) buffers (16 B), runs (40 B), records (32 B), row_fill,
// item_doc, item_col, dl_len, dl_slot (4 B each), the digit counts (2 B): 142 B, plus 8 B per class (8 L).  The cap on L,
// JTK_FIT_MAX_LEN = 262144, is what the class bitmap may take of the LDS.  Every round is a launch of its own: no data
// passes between workgroups inside one launch.
#include "jtk_device_prims.h"
#include "jtk_kernels.h"

namespace {

constexpr int PF_TILE = 1024;         // cells per workgroup step of write and labels (256 lanes x 4)
constexpr int PF_MAX_BLOCKS = 4096;   // workgroups of write and labels; each takes a contiguous run of tiles
constexpr int ST = JTK_FIT_SORT_TILE;
constexpr int PF_ROW_BLOCKS = 1024;   // workgroups of pf_rows (4 waves each, a run per wave and step)
static_assert(ST == 256 * 4, "a sort tile is 4 waves x 4 rounds of 64 keys");

__device__ __forceinline__ void pf_max(int64_t* dst, int64_t v) {        // max over the wave, one atomic (all lanes call it)
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const int64_t o = __shfl_xor(v, d);
        v = o > v ? o : v;
    }
    if ((threadIdx.x & 63) == 0 && v > 0) atomicMax((unsigned long long*)dst, (unsigned long long)v);
}

__global__ void __launch_bounds__(256) k_pf_len(JtkPackFitWork w) {
    const int64_t d = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= w.v.n) return;
    const int64_t L = w.v.L, l = jtk_pack_unit_len(w.v.tok_off[d + 1] - w.v.tok_off[d], w.status[d], w.v.sep_id);
    w.FR[d] = l / L;
    w.key[0][d] = (uint32_t)(l % L ? L - l % L : L);
    w.val[0][d] = (int32_t)d;
}

__global__ void __launch_bounds__(256) k_pf_hist(const uint32_t* key, int64_t n, int shift, int64_t tiles, int64_t* hist) {
    __shared__ uint32_t s_h[256];
    s_h[threadIdx.x] = 0;
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * ST;
    for (int j = 0; j < 4; j++) {
        const int64_t i = base + j * 256 + threadIdx.x;
        if (i < n) atomicAdd(&s_h[(key[i] >> shift) & 255u], 1u);
    }
    __syncthreads();
    hist[(int64_t)threadIdx.x * tiles + blockIdx.x] = s_h[threadIdx.x];
}

__global__ void __launch_bounds__(256) k_pf_scatter(const uint32_t* key, const int32_t* val, int64_t n, int shift, int64_t tiles,
                                                    const int64_t* hist, uint32_t* key_out, int32_t* val_out) {
    __shared__ uint32_t s_cnt[4][256];
    __shared__ uint32_t s_off[4][256];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t base = (int64_t)blockIdx.x * ST + wv * 256 + lane;      // the wave's keys: base + 64 j
    for (int k = 0; k < 4; k++) s_cnt[k][tid] = 0;
    __syncthreads();
    uint32_t ky[4];
    int32_t vl[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int64_t i = base + j * 64;
        ky[j] = 0; vl[j] = 0;
        if (i < n) { ky[j] = key[i]; vl[j] = val[i]; atomicAdd(&s_cnt[wv][(ky[j] >> shift) & 255u], 1u); }
    }
    __syncthreads();
    uint32_t run = (uint32_t)hist[(int64_t)tid * tiles + blockIdx.x];     // (positions are below n < 2^31)
    for (int k = 0; k < 4; k++) { s_off[k][tid] = run; run += s_cnt[k][tid]; }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const bool valid = base + j * 64 < n;
        const uint32_t dg = (ky[j] >> shift) & 255u;
        uint64_t peers = __ballot(valid);                                 // the valid lanes of the round with the same digit
#pragma unroll
        for (int b = 0; b < 8; b++) {
            const uint64_t m = __ballot((dg >> b) & 1u);
            peers &= ((dg >> b) & 1u) ? m : ~m;
        }
        const uint32_t rank = (uint32_t)__popcll(peers & ((1ull << lane) - 1));
        const uint32_t pos = s_off[wv][dg] + rank;
        __builtin_amdgcn_wave_barrier();                                  // (every peer has read the offset before it moves)
        if (valid && rank == 0) s_off[wv][dg] += (uint32_t)__popcll(peers);
        __builtin_amdgcn_wave_barrier();
        if (valid) { key_out[pos] = ky[j]; val_out[pos] = vl[j]; }
    }
}

__global__ void __launch_bounds__(256) k_pf_bounds(JtkPackFitWork w, const uint32_t* key) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t n = w.v.n;
    if (i >= n) return;
    const uint32_t L = (uint32_t)w.v.L, k = key[i];
    w.DF[i] = (k < L && (i == 0 || key[i - 1] != k)) ? 1 : 0;
    if (k < L && (i == n - 1 || key[i + 1] >= L)) w.hdr[1] = i + 1;
}

__global__ void __launch_bounds__(256) k_pf_distinct(JtkPackFitWork w, const uint32_t* key) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= w.v.n) return;
    const uint32_t L = (uint32_t)w.v.L, k = key[i];
    if (k < L && (i == 0 || key[i - 1] != k)) {
        const int64_t j = w.DF[i];
        w.dl_len[j] = (int32_t)(L - k);
        w.dl_slot[j] = (int32_t)i;
    }
}

__global__ void __launch_bounds__(64) k_pf_drive(JtkPackFitWork w) {
    __shared__ uint64_t s_bits[JTK_FIT_WORDS];
    __shared__ uint64_t s_sum[JTK_FIT_SUMS];
    const int64_t L = w.v.L;
    for (int64_t i = threadIdx.x; i < (L >> 6) + 1 && i < JTK_FIT_WORDS; i += 64) s_bits[i] = 0;
    s_sum[threadIdx.x] = 0;
    __syncthreads();
    if (threadIdx.x != 0) return;
    JtkFitState st;
    st.bits = s_bits; st.sum = s_sum; st.head = w.head; st.tail = w.tail; st.runs = w.runs; st.recs = w.recs;
    st.L = L; st.n_runs = 0; st.n_recs = 0; st.next_row = 0;
    const int64_t R = w.hdr[1], D = w.hdr[2];
    for (int64_t j = 0; j < D; j++) {
        const int64_t l = w.dl_len[j];
        int64_t slot = w.dl_slot[j], k = (j + 1 < D ? (int64_t)w.dl_slot[j + 1] : R) - slot;
        while (k > 0) {
            const int64_t m = jtk_fit_step(st, l, slot, k);
            slot += m; k -= m;
        }
    }
    w.hdr[3] = w.hdr[0] > 0 ? L : (D > 0 ? (int64_t)w.dl_len[0] : 0);     // the longest piece; pf_rows adds the pad runs
    w.hdr[4] = st.next_row;
    w.hdr[5] = st.n_recs;
    w.hdr[6] = st.n_runs;
}

__global__ void __launch_bounds__(256) k_pf_rows(JtkPackFitWork w) {
    const int lane = threadIdx.x & 63;
    const int64_t n_runs = w.hdr[6], L = w.v.L;
    int64_t pad = 0;
    for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < n_runs; r += (int64_t)gridDim.x * 4) {
        const JtkFitRun run = w.runs[r];
        for (int64_t t = lane; t < run.count; t += 64) {
            const int64_t i = run.row_lo + t;
            w.ITEM[i] = run.pieces;
            w.SEGR[i] = run.pieces + (run.free > 0 ? 1 : 0);
            w.row_fill[i] = (int32_t)(L - run.free);
            pad = run.free > pad ? run.free : pad;
        }
    }
    pf_max(&w.hdr[3], pad);
}

__global__ void __launch_bounds__(256) k_pf_expand(JtkPackFitWork w, const int32_t* val) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= w.hdr[1]) return;
    const JtkFitRec rec = w.recs[jtk_fit_rec_of(w.recs, w.hdr[5], i)];
    const int64_t x = i - rec.slot, row = rec.row_lo + x / rec.per, at = w.ITEM[row] + rec.pieces + x % rec.per;
    w.item_doc[at] = val[i];
    w.item_col[at] = (int32_t)(w.v.L - rec.c + (x % rec.per) * rec.l);
}

__global__ void __launch_bounds__(256) k_pf_write(JtkFitView v, int64_t n_seg, int32_t pad_id, int32_t* rows, int32_t* positions,
                                                  int32_t* cu_seqlens, int64_t* seg_doc, int64_t total, int64_t tiles_per_block) {
    const int64_t L = v.L;
    const int64_t n_tiles = (total + PF_TILE - 1) / PF_TILE;
    const int64_t t0 = (int64_t)blockIdx.x * tiles_per_block;
    const int64_t t1 = t0 + tiles_per_block < n_tiles ? t0 + tiles_per_block : n_tiles;
    if (blockIdx.x == 0 && threadIdx.x == 0 && cu_seqlens) cu_seqlens[n_seg] = (int32_t)total;
    for (int64_t t = t0; t < t1; t++) {
        const int64_t e0 = t * PF_TILE + threadIdx.x * 4;
        if (e0 >= total) break;
        int64_t r = e0 / L, c = e0 - r * L;
        JtkFitRow row = jtk_fit_row(v, r);
        JtkFitCursor k;
        k.rank = -1;
        int32_t id[4], pos[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            id[j] = pad_id; pos[j] = 0;
            if (e0 + j >= total) continue;
            if (c == L) { r++; c = 0; row = jtk_fit_row(v, r); k.rank = -1; }
            const JtkPackCell cell = jtk_fit_cell(v, row, r, c, pad_id, k);
            id[j] = cell.id; pos[j] = cell.pos;
            if (cell.start) {
                if (cu_seqlens) cu_seqlens[cell.seg] = (int32_t)(e0 + j);
                if (seg_doc) seg_doc[cell.seg] = cell.doc;
            }
            c++;
        }
        const bool full = e0 + 4 <= total;
        int32_t* dr = rows + e0;
        if (full && ((uintptr_t)dr & 15u) == 0) *reinterpret_cast<int4*>(dr) = make_int4(id[0], id[1], id[2], id[3]);
        else for (int j = 0; j < 4; j++) if (e0 + j < total) dr[j] = id[j];
        if (positions) {
            int32_t* dp = positions + e0;
            if (full && ((uintptr_t)dp & 15u) == 0) *reinterpret_cast<int4*>(dp) = make_int4(pos[0], pos[1], pos[2], pos[3]);
            else for (int j = 0; j < 4; j++) if (e0 + j < total) dp[j] = pos[j];
        }
    }
}

template <bool SHIFT>
__global__ void __launch_bounds__(256) k_pf_labels(JtkFitView v, JtkLabelView lv, int32_t* labels, int64_t total,
                                                   int64_t tiles_per_block) {
    const int64_t L = v.L;
    constexpr int NC = SHIFT ? 5 : 4;                                     // cells a lane maps: its four, and the one after
    JtkPackView pv{};                                                     // (what jtk_label_cell reads of it)
    pv.sep_id = v.sep_id; pv.sep_first = v.sep_first;
    const int64_t n_tiles = (total + PF_TILE - 1) / PF_TILE;
    const int64_t t0 = (int64_t)blockIdx.x * tiles_per_block;
    const int64_t t1 = t0 + tiles_per_block < n_tiles ? t0 + tiles_per_block : n_tiles;
    for (int64_t t = t0; t < t1; t++) {
        const int64_t e0 = t * PF_TILE + threadIdx.x * 4;
        if (e0 >= total) break;
        int64_t r = e0 / L, c = e0 - r * L;
        JtkFitRow row = jtk_fit_row(v, r);
        JtkFitCursor k;
        k.rank = -1;
        int32_t lab[NC];
        int64_t seg[NC], col[NC];
#pragma unroll
        for (int j = 0; j < NC; j++) {
            lab[j] = lv.ignore_index; seg[j] = -1; col[j] = c;
            // (the fifth cell is looked at only when it continues the fourth's row)
            if (e0 + j >= total || (j == 4 && c == L)) continue;
            if (c == L) { r++; c = 0; col[j] = 0; row = jtk_fit_row(v, r); k.rank = -1; }
            const JtkPackCell cell = jtk_fit_cell(v, row, r, c, 0, k);
            lab[j] = jtk_label_cell(pv, row.row, c, cell, k.u, lv);
            seg[j] = cell.seg;
            c++;
        }
        int32_t o[4];
#pragma unroll
        for (int j = 0; j < 4; j++)
            o[j] = SHIFT ? jtk_label_shift(col[j], L, seg[j], seg[j + NC - 4], lab[j + NC - 4], lv.ignore_index) : lab[j];
        int32_t* dl = labels + e0;
        if (e0 + 4 <= total && ((uintptr_t)dl & 15u) == 0) *reinterpret_cast<int4*>(dl) = make_int4(o[0], o[1], o[2], o[3]);
        else for (int j = 0; j < 4; j++) if (e0 + j < total) dl[j] = o[j];
    }
}

inline dim3 pf_cell_grid(int64_t total, int64_t* per) {
    const int64_t n_tiles = (total + PF_TILE - 1) / PF_TILE;
    const int64_t blocks = n_tiles < PF_MAX_BLOCKS ? n_tiles : PF_MAX_BLOCKS;
    *per = (n_tiles + blocks - 1) / blocks;
    return dim3((unsigned)((n_tiles + *per - 1) / *per));
}

}  // namespace

void jtk_launch_pack_fit_plan(const JtkPackFitWork& w, hipStream_t s) {
    const int64_t n = w.v.n;
    if (n <= 0) return;                                                   // (hdr is all zero: no rows)
    const dim3 docs(jtk_blocks_for(n, 256)), tiles((unsigned)w.tiles);
    hipLaunchKernelGGL(k_pf_len, docs, dim3(256), 0, s, w);
    jtk_launch_scan_i64(w.FR, n, &w.hdr[0], s);
    for (int p = 0; p < w.passes; p++) {
        const uint32_t* ki = w.key[p & 1];
        const int32_t* vi = w.val[p & 1];
        hipLaunchKernelGGL(k_pf_hist, tiles, dim3(256), 0, s, ki, n, 8 * p, w.tiles, w.hist);
        jtk_launch_scan_i64(w.hist, 256 * w.tiles, nullptr, s);
        hipLaunchKernelGGL(k_pf_scatter, tiles, dim3(256), 0, s, ki, vi, n, 8 * p, w.tiles, (const int64_t*)w.hist,
                           w.key[(p + 1) & 1], w.val[(p + 1) & 1]);
    }
    const uint32_t* key = w.key[w.passes & 1];
    hipLaunchKernelGGL(k_pf_bounds, docs, dim3(256), 0, s, w, key);
    jtk_launch_scan_i64(w.DF, n, &w.hdr[2], s);
    hipLaunchKernelGGL(k_pf_distinct, docs, dim3(256), 0, s, w, key);
    hipLaunchKernelGGL(k_pf_drive, dim3(1), dim3(64), 0, s, w);
    (void)hipMemsetAsync(w.ITEM, 0, (size_t)(n + 1) * 8, s);               // (rows that were not opened count nothing)
    (void)hipMemsetAsync(w.SEGR, 0, (size_t)(n + 1) * 8, s);
    hipLaunchKernelGGL(k_pf_rows, dim3(PF_ROW_BLOCKS), dim3(256), 0, s, w);
    jtk_launch_scan_i64(w.ITEM, n, nullptr, s);
    jtk_launch_scan_i64(w.SEGR, n, &w.hdr[7], s);
    hipLaunchKernelGGL(k_pf_expand, docs, dim3(256), 0, s, w, (const int32_t*)w.val[w.passes & 1]);
}

void jtk_launch_pack_fit_write(const JtkPackFitWork& w, int64_t n_rows, int64_t n_seg, int32_t pad_id, int32_t* rows,
                               int32_t* positions, int32_t* cu_seqlens, int64_t* seg_doc, hipStream_t s) {
    const int64_t total = n_rows * w.v.L;
    if (total <= 0) {
        if (cu_seqlens) (void)hipMemsetAsync(cu_seqlens, 0, 4, s);
        return;
    }
    int64_t per;
    const dim3 grid = pf_cell_grid(total, &per);
    hipLaunchKernelGGL(k_pf_write, grid, dim3(256), 0, s, w.v, n_seg, pad_id, rows, positions, cu_seqlens, seg_doc, total, per);
}

void jtk_launch_pack_fit_labels(const JtkPackFitWork& w, int64_t n_rows, const JtkLabelView& lv, bool shift, int32_t* labels,
                                hipStream_t s) {
    const int64_t total = n_rows * w.v.L;
    if (total <= 0) return;
    int64_t per;
    const dim3 grid = pf_cell_grid(total, &per);
    if (shift) hipLaunchKernelGGL(k_pf_labels<true>, grid, dim3(256), 0, s, w.v, lv, labels, total, per);
    else hipLaunchKernelGGL(k_pf_labels<false>, grid, dim3(256), 0, s, w.v, lv, labels, total, per);
}
