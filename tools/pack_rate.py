"""Packed training rows of a device-resident batch (jtk_batch_pack, jtk_batch_pack_write) on the headline corpus (corpus.mixed,
cl100k_base, encodeOrdinary, <|endoftext|> after every document), and of one long document.

Per (seq_len, mode): the whole-document encode (jtk_batch_encode_device), the plan (the call's one wait included), the write of
rows, positions, cu_seqlens and seg_doc, and the two back to back, each timed with HIP events on its stream after warm-up.
"GB" is what the write must move: 4 B per token id read, 4 + 4 B per cell written (rows, positions), 12 B per segment; the
rate is that over the write's time, against the ~6.3 TB/s HBM achieves.  The counts and a seeded sample of rows are checked
against the restatement (tests/pack_ref.py) on the encode's own tokens.

  python tools/pack_rate.py [--docs 200000] [--sizes 2048,8192] [--iters 10] [--long-mb 40]
"""
import argparse
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

EOT_ID = 100257


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=200000)
    ap.add_argument("--sizes", default="2048,8192")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--long-mb", type=float, default=40.0, help="size of the one-document case (0: skip)")
    ap.add_argument("--sample", type=int, default=50)
    args = ap.parse_args()
    import torch
    import bench
    import jtokkit_amd
    import pack_ref

    enc = jtokkit_amd.get_encoding("cl100k_base")
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(dev)              # (a real stream: the library reads a NULL handle as the batch's own stream)
    sp = stream.cuda_stream

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        stream.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(args.iters):
            fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / args.iters

    def run_case(label, text, doc_off):
        n_docs = len(doc_off) - 1
        d_text, d_off = torch.from_numpy(text).to(dev), torch.from_numpy(doc_off).to(dev)
        torch.cuda.synchronize()
        b = enc.new_batch()
        t_enc = timed(lambda: b.encode_device(d_text.data_ptr(), d_off.data_ptr(), n_docs, len(text), True, stream=sp, sync=False))
        nt = b.encode_device(d_text.data_ptr(), d_off.data_ptr(), n_docs, len(text), True, stream=sp)
        res = b.fetch()
        lens = np.diff(res.tok_off) + 1
        U = res.tok_off[:-1] + np.arange(n_docs)
        S = np.insert(res.tokens, res.tok_off[1:], EOT_ID)
        print("%s: %d documents, %.1f MB, %d tokens; encode %.2f ms" % (label, n_docs, len(text) / 1e6, nt, t_enc), flush=True)
        rng = random.Random(5)
        for L in [int(x) for x in args.sizes.split(",")]:
            for whole in (False, True):
                t_plan = timed(lambda: b.pack(L, EOT_ID, whole, stream=sp))
                nr, ns, mx = b.pack(L, EOT_ID, whole, stream=sp)
                out = [torch.empty(nr * L, dtype=torch.int32, device=dev), torch.empty(nr * L, dtype=torch.int32, device=dev),
                       torch.empty(ns + 1, dtype=torch.int32, device=dev), torch.empty(max(ns, 1), dtype=torch.int64, device=dev)]
                ptrs = [t.data_ptr() for t in out]
                t_write = timed(lambda: b.pack_write(-1, *ptrs, stream=sp))

                def both():
                    b.pack(L, EOT_ID, whole, stream=sp)
                    b.pack_write(-1, *ptrs, stream=sp)
                t_both = timed(both)
                stream.synchronize()
                a = pack_ref.row_starts(lens.tolist(), L, whole)
                assert nr == len(a) - 1, (label, L, whole)
                cu, sd, exp_mx = pack_ref.segments(U, np.arange(n_docs), a, L)
                assert ns == len(sd) and mx == exp_mx, (label, L, whole)
                assert np.array_equal(out[2].cpu().numpy(), cu)
                rows = out[0].view(nr, L)
                for r in rng.sample(range(nr), min(args.sample, nr)):
                    ids, _ = pack_ref.row(S, U, a, r, L, -1)
                    assert np.array_equal(rows[r].cpu().numpy(), ids), (label, L, whole, r)
                gb = (4.0 * nt + 8.0 * nr * L + 12.0 * ns) / 1e9
                print("  L=%-5d %-6s rows=%-7d segments=%-8d max_seqlen=%-5d plan %7.3f ms  write %7.3f ms (%5.0f GB/s, %.2f GB)  "
                      "plan+write %7.3f ms" % (L, "whole" if whole else "concat", nr, ns, mx, t_plan, t_write, gb / t_write * 1e3, gb,
                                               t_both), flush=True)
                del out, rows
                torch.cuda.empty_cache()
        b.close()

    text, doc_off = bench.make_corpus("mixed", args.docs, 3, min(16, len(os.sched_getaffinity(0))))
    run_case("corpus.mixed (headline)", np.ascontiguousarray(text), np.ascontiguousarray(doc_off))
    if args.long_mb > 0:
        from jtokkit_amd import corpus
        n = int(args.long_mb * 1e6 / 4096)
        t1, _ = corpus.mixed(n, mean_bytes=4096, seed=44)
        t1 = np.ascontiguousarray(t1, dtype=np.uint8)
        run_case("one long document", t1, np.array([0, len(t1)], dtype=np.int64))


if __name__ == "__main__":
    main()
