"""Token-budget chunks of a device-resident batch (jtk_batch_chunk, jtk_batch_chunk_rows, jtk_batch_token_offsets) on the
headline corpus (corpus.mixed, cl100k_base, encodeOrdinary), and of one long document.

Per (N, overlap): the whole-document encode (jtk_batch_encode_device), the chunk plan (count, scan, byte scan, records; the
call's one wait included), the rows [n_chunks, N] and the token offsets, each timed with HIP events on its stream after
warm-up.  "GB/s" is the bytes a kernel must move (plan: 4 B per token id read + 41 B per chunk record; rows: the ids read
and the rows written; offsets: 4 B read + 8 B written per token) over its time, against the ~6.3 TB/s HBM achieves.  The output
is checked against the CPU restatement of the rule (tests/chunk_ref.py) on a seeded sample of documents.

  python tools/chunk_rate.py [--docs 200000] [--sizes 256,512,8192] [--overlaps 0,64] [--iters 10] [--long-mb 40]
"""
import argparse
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=200000)
    ap.add_argument("--sizes", default="256,512,8192")
    ap.add_argument("--overlaps", default="0,64")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--long-mb", type=float, default=40.0, help="size of the one-document case (0: skip)")
    ap.add_argument("--sample", type=int, default=300)
    args = ap.parse_args()
    import torch
    import bench
    import chunk_ref
    import jtokkit_amd
    import oracle_lib

    enc = jtokkit_amd.get_encoding("cl100k_base")
    o = oracle_lib.get("cl100k_base")
    tabs = chunk_ref.IdTables(o)
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
        tokens = b.fetch()
        pos = torch.empty(max(nt, 1), dtype=torch.int64, device=dev)
        print("%s: %d documents, %.1f MB, %d tokens; encode %.2f ms" % (label, n_docs, len(text) / 1e6, nt, t_enc), flush=True)
        rng = random.Random(5)
        sample = sorted(rng.sample(range(n_docs), min(args.sample, n_docs)))
        for N in [int(x) for x in args.sizes.split(",")]:
            for ov in [int(x) for x in args.overlaps.split(",")]:
                if ov >= N:
                    continue
                t_plan = timed(lambda: b.chunk(N, ov, sp))
                nc = b.chunk(N, ov, sp)
                rows = torch.empty((nc, N), dtype=torch.int32, device=dev)
                t_rows = timed(lambda: b.chunk_rows(-1, rows.data_ptr(), sp))
                t_off = timed(lambda: b.token_offsets(pos.data_ptr(), sp))
                f = b.chunk_fetch()
                in_rows = int(f["n_tok"].sum())
                # check against the CPU rule on the sample
                for d in sample:
                    toks = tokens.doc(d)
                    exp = chunk_ref.chunks(tabs.first[toks], N, ov)
                    got = [(int(f["tok_begin"][c] - tokens.tok_off[d]), int(f["tok_begin"][c] - tokens.tok_off[d] + f["n_tok"][c]),
                            bool(f["split"][c])) for c in range(f["chunk_off"][d], f["chunk_off"][d + 1])]
                    assert got == exp, (label, d, N, ov)
                    cum = np.concatenate([[0], np.cumsum(tabs.length[toks])])
                    for c, (s, e, _) in zip(range(f["chunk_off"][d], f["chunk_off"][d + 1]), exp):
                        assert f["byte_begin"][c] == doc_off[d] + cum[s] and f["byte_end"][c] == doc_off[d] + cum[e]
                gb_plan = (4.0 * nt + 41.0 * nc) / 1e9
                gb_rows = (4.0 * in_rows + 4.0 * nc * N) / 1e9
                gb_off = 12.0 * nt / 1e9
                print("  N=%-5d overlap=%-3d chunks=%-9d plan %7.3f ms (%5.0f GB/s)  rows %7.3f ms (%5.0f GB/s, %.2f GB)  "
                      "offsets %7.3f ms (%5.0f GB/s)  [checked %d docs]"
                      % (N, ov, nc, t_plan, gb_plan / t_plan * 1e3, t_rows, gb_rows / t_rows * 1e3, gb_rows, t_off,
                         gb_off / t_off * 1e3, len(sample)), flush=True)
                del rows
                torch.cuda.empty_cache()
        b.close()

    text, doc_off = bench.make_corpus("mixed", args.docs, 3, min(16, len(os.sched_getaffinity(0))))
    run_case("corpus.mixed (headline)", np.ascontiguousarray(text), np.ascontiguousarray(doc_off))
    if args.long_mb > 0:
        from jtokkit_amd import corpus
        n = int(args.long_mb * 1e6 / 4096)
        t1, off1 = corpus.mixed(n, mean_bytes=4096, seed=44)
        t1 = np.ascontiguousarray(t1, dtype=np.uint8)
        args.sample = 1
        run_case("one long document", t1, np.array([0, len(t1)], dtype=np.int64))


if __name__ == "__main__":
    main()
