"""Compact token ids (jtk_batch_compact, JTK_ENCODE_COMPACT_IDS) on the headline corpus (bench.make_corpus as bench.py builds
it: corpus.mixed, cl100k_base, encodeOrdinary).

(a) kernel   the post-pass on a device-resident result (the first --kernel-docs documents): jtk_batch_compact timed with HIP
             events on its stream after warm-up.  "GB" is what the pass must move: 4 B read and 2 B + hb / 8 B written per
             token; the rate is that over the pass's time, against the ~6.3 TB/s HBM achieves (8 TB/s peak).
(b) end to end, as bench.py's end_to_end_cfg3: pinned input (jtk_host_alloc), 64 MiB host chunks, 3 in flight, result read in
             place in pinned memory -- the plain route (int32 ids up) and the compact route (two planes up) ALTERNATING in one
             process, --rounds timed calls each after a warm-up call each; min / median / max and the bytes each way.
(c) the same with JTK_ENCODE_COUNT_ONLY (no ids go up at all: what the input's way down alone allows), in the same alternation.
One batch serves all three modes (same streams, scratch and pinned buffers).  The compact planes are checked against the plain
ids: (a) lo everywhere, hi on the head and the tail; (b) lo on the first 50 M tokens, hi on the head, sampled documents widened.

  python tools/compact_rate.py [--docs 1000000] [--rounds 5] [--kernel-docs 200000] [--plain-only] [--skip-kernel]
--plain-only runs (b) and (c) without the compact route: for a library that predates it (JTOKKIT_AMD_LIB=path/to/older.so).
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1000000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--kernel-docs", type=int, default=200000)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--skip-kernel", action="store_true")
    ap.add_argument("--skip-e2e", action="store_true")
    args = ap.parse_args()
    import torch
    import bench
    import compact_ref
    import jtokkit_amd
    N = jtokkit_amd._native

    print("library: %s (%s)" % (N.lib().jtk_version().decode(), os.path.basename(N.LIB_PATH)), flush=True)
    enc = jtokkit_amd.get_encoding("cl100k_base")
    dev = torch.device("cuda:0")
    text, doc_off = bench.make_corpus("mixed", args.docs, 3, min(16, len(os.sched_getaffinity(0))))
    text, doc_off = np.ascontiguousarray(text), np.ascontiguousarray(doc_off)
    n_docs, n_bytes = len(doc_off) - 1, int(doc_off[-1])
    print("corpus.mixed (headline): %d documents, %.2f GB" % (n_docs, n_bytes / 1e9), flush=True)

    if not args.skip_kernel and not args.plain_only:
        hb = enc.id_bits - 16
        nd = min(args.kernel_docs, n_docs)
        nb = int(doc_off[nd])
        d_text = torch.zeros(nb + 32, dtype=torch.uint8, device=dev)
        d_text[:nb] = torch.from_numpy(text[:nb]).to(dev)
        d_off = torch.from_numpy(doc_off[:nd + 1]).to(dev)
        torch.cuda.synchronize()
        stream = torch.cuda.Stream(dev)          # (a real stream: the library reads a NULL handle as the batch's own stream)
        sp = stream.cuda_stream
        b = enc.new_batch()
        nt = b.encode_device(d_text.data_ptr(), d_off.data_ptr(), nd, nb, True, stream=sp)
        nw = compact_ref.hi_words(nt, hb)
        lo = torch.empty(nt, dtype=torch.int16, device=dev)
        hi = torch.empty(max(nw, 1), dtype=torch.int32, device=dev)
        for _ in range(3):
            b.compact(lo.data_ptr(), hi.data_ptr(), sp)
        stream.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(args.iters):
            b.compact(lo.data_ptr(), hi.data_ptr(), sp)
        e1.record(stream)
        e1.synchronize()
        ms = e0.elapsed_time(e1) / args.iters
        ids = b.fetch().tokens
        assert np.array_equal(lo.cpu().numpy().view(np.uint16), (ids & 0xFFFF).astype(np.uint16))
        h = hi.cpu().numpy().view(np.uint32)[:nw]
        k = min(nt, 1 << 20) // 32 * 32
        assert np.array_equal(h[:k * hb // 32], compact_ref.compact(ids[:k], hb)[1])
        t0 = (nt - min(nt, 1 << 20)) // 32 * 32
        assert np.array_equal(h[t0 * hb // 32:], compact_ref.compact(ids[t0:], hb)[1])
        gb = (4.0 * nt + 2.0 * nt + 4.0 * nw) / 1e9
        print("(a) post-pass, %d documents, %d tokens, id_bits %d: %.3f ms per pass (with its launch), %.3f GB moved "
              "(%.3f B per token) -> %.0f GB/s = %.0f %% of 6.3 TB/s achievable, %.0f %% of the 8 TB/s peak; planes == the plain ids"
              % (nd, nt, 16 + hb, ms, gb, gb * 1e9 / nt, gb / ms * 1e3, gb / ms * 1e3 / 63, gb / ms * 1e3 / 80), flush=True)
        b.close()
        del d_text, d_off, lo, hi
        torch.cuda.empty_cache()
    if args.skip_e2e:
        return

    hbuf = jtokkit_amd.HostBuffer(n_bytes)
    hbuf.array[:] = text
    modes = ["plain", "count_only"] if args.plain_only else ["plain", "compact", "count_only"]
    # ONE batch serves every mode: the same streams (the runtime maps a process's streams onto a few hardware queues in the
    # order they were made, so a second batch's copy stream may share a queue with kernels that the first one's does not),
    # the same device scratch and the same pinned buffers
    eb = enc.new_batch()
    eb.set_option(N.JTK_OPT_HOST_CHUNK_BYTES, 64 << 20)
    eb.set_option(N.JTK_OPT_CHUNKS_IN_FLIGHT, 3)

    def run(m):
        kw = dict(ordinary=True, to_host=True)
        if m == "compact":
            kw["compact"] = True
        if m == "count_only":
            kw["count_only"] = True
        t0 = time.perf_counter()
        nt = eb.encode_host(hbuf.array, doc_off, **kw)
        return time.perf_counter() - t0, nt

    nt = 0
    for m in modes:                               # warm-up: the buffers grow on the first call
        nt = run(m)[1]
    times = {m: [] for m in modes}
    for _ in range(args.rounds):
        for m in modes:
            times[m].append(run(m)[0])
    if "compact" in modes:
        run("plain")
        plain = eb.host_result()
        p_off, p_status = plain.tok_off.copy(), plain.status.copy()
        head = min(nt, 50000000)
        p_head = plain.tokens[:head].copy()
        pick = np.random.default_rng(3).choice(n_docs, 3000, replace=False)
        p_docs = [plain.doc(d).copy() for d in pick]
        run("compact")                            # (overwrites the pinned buffers the views above pointed into)
        comp = eb.host_result_compact()
        assert np.array_equal(p_off, comp.tok_off) and np.array_equal(p_status, comp.status)
        assert np.array_equal(comp.lo[:head], (p_head & 0xFFFF).astype(np.uint16))
        k = min(head, 1 << 22) // 32 * 32
        assert np.array_equal(comp.hi[:k * (comp.id_bits - 16) // 32], compact_ref.compact(p_head[:k], comp.id_bits - 16)[1])
        for d, want in zip(pick, p_docs):
            assert np.array_equal(comp.doc(d), want)
        id_bits = comp.id_bits
    else:
        id_bits = 17
    side = 12 * (n_docs + 1)
    up = {"plain": 4 * nt + side, "compact": 2 * nt + 4 * ((nt * (id_bits - 16) + 31) // 32) + side, "count_only": side}
    down = n_bytes + 8 * (n_docs + 1)
    print("end to end, %d tokens, pinned input, 64 MiB host chunks, 3 in flight, %d alternating rounds after a warm-up each; "
          "%.2f GB go down per call" % (nt, args.rounds, down / 1e9), flush=True)
    for tag, m in (("(b)", "plain"), ("(b)", "compact"), ("(c)", "count_only")):
        if m not in modes:
            continue
        r = sorted(n_bytes / t / 1e9 for t in times[m])
        print("%s %-10s GB/s of input: min %.2f  median %.2f  max %.2f   (ms per call: %s)   %.2f GB up per call (%.3f B per token)"
              % (tag, m, r[0], statistics.median(r), r[-1], " ".join("%.0f" % (t * 1e3) for t in times[m]), up[m] / 1e9,
                 (up[m] - side) / max(nt, 1)), flush=True)
    if "compact" in modes:
        p = sorted(n_bytes / t / 1e9 for t in times["plain"])
        c = sorted(n_bytes / t / 1e9 for t in times["compact"])
        print("compact over plain: median x%.2f; ranges %s" % (statistics.median(c) / statistics.median(p),
              "do not overlap (compact min %.2f > plain max %.2f)" % (c[0], p[-1]) if c[0] > p[-1] else "OVERLAP"), flush=True)
    eb.close()
    hbuf.close()


if __name__ == "__main__":
    main()
