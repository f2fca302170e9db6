"""Boundary-preferring chunks of a device-resident batch (jtk_batch_chunk_prefer) against the plain plan (jtk_batch_chunk) in
the same run, on the headline corpus (corpus.mixed, cl100k_base, encodeOrdinary) and on one long document.

Per (N, overlap), with prefer = 15 and min_tokens = N / 2: the plan of jtk_batch_chunk and the plan of
jtk_batch_chunk_prefer (level plane, count, scan, byte scan, records; the call's wait included), the level plane alone
(jtk_batch_token_cut_levels: cp_levels + cp_doc_heads) and, by difference, the rest of the new plan (walks, scan, byte scan,
records), each timed with HIP events on its stream after warm-up.  The output is checked against the CPU restatement of the
rule (tests/chunk_prefer_ref.py) on a seeded sample of documents.  Per-kernel times come from running this tool under
`rocprofv3 --kernel-trace --stats`.  Writes its lines to --out as well.

  python tools/chunk_prefer_rate.py [--docs 200000] [--sizes 256,512] [--overlaps 0,64] [--iters 10] [--long-mb 40]
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
    ap.add_argument("--sizes", default="256,512")
    ap.add_argument("--overlaps", default="0,64")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--long-mb", type=float, default=40.0, help="size of the one-document case (0: skip)")
    ap.add_argument("--sample", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chunk_prefer_rate.txt"))
    args = ap.parse_args()
    import torch
    import bench
    import chunk_prefer_ref as ref
    import jtokkit_amd
    import oracle_lib

    enc = jtokkit_amd.get_encoding("cl100k_base")
    o = oracle_lib.get("cl100k_base")
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(dev)              # (a real stream: the library reads a NULL handle as the batch's own stream)
    sp = stream.cuda_stream
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def timed(fn, iters):
        for _ in range(min(args.warmup, iters)):
            fn()
        stream.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(iters):
            fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / iters

    def run_case(label, text, doc_off, iters, n_sample):
        n_docs = len(doc_off) - 1
        d_text, d_off = torch.from_numpy(text).to(dev), torch.from_numpy(doc_off).to(dev)
        torch.cuda.synchronize()
        b = enc.new_batch()
        nt = b.encode_device(d_text.data_ptr(), d_off.data_ptr(), n_docs, len(text), True, stream=sp)
        tokens = b.fetch()
        plane = torch.empty(max(nt, 1), dtype=torch.uint8, device=dev)
        say("%s: %d documents, %.1f MB, %d tokens" % (label, n_docs, len(text) / 1e6, nt))
        t_plane = timed(lambda: b.token_cut_levels(15, plane.data_ptr(), sp), iters)
        say("  level plane alone (prefer=15): %.3f ms (%.0f GB/s at 4 B read + 1 B written per token)"
            % (t_plane, 5.0 * nt / 1e9 / t_plane * 1e3))
        rng = random.Random(5)
        sample = sorted(rng.sample(range(n_docs), min(n_sample, n_docs)))
        for N in [int(x) for x in args.sizes.split(",")]:
            for ov in [int(x) for x in args.overlaps.split(",")]:
                if ov >= N:
                    continue
                mt = max(N // 2, 1)
                t_old = timed(lambda: b.chunk(N, ov, sp), iters)
                nc_old = b.chunk(N, ov, sp)
                t_new = timed(lambda: b.chunk_prefer(N, ov, mt, 15, sp), iters)
                nc = b.chunk_prefer(N, ov, mt, 15, sp)
                f = b.chunk_fetch()
                lv = b.chunk_levels()[0]
                for d in sample:
                    toks = tokens.doc(d)
                    if len(toks) > 200000:                           # (the restatement is plain Python)
                        continue
                    tb = ref.token_bytes(o, toks.tolist())
                    exp = ref.chunks_fast(ref.levels(tb, 15), N, ov, mt)
                    t0 = tokens.tok_off[d]
                    got = [(int(f["tok_begin"][c] - t0), int(f["tok_begin"][c] - t0 + f["n_tok"][c]), bool(f["split"][c]), int(lv[c]))
                           for c in range(f["chunk_off"][d], f["chunk_off"][d + 1])]
                    assert got == exp, (label, d, N, ov)
                hist = np.bincount(lv, minlength=7).tolist()
                say("  N=%-5d overlap=%-3d min=%-4d plain plan %7.3f ms (%d chunks)  prefer plan %7.3f ms (%d chunks)  ratio %.2f  "
                    "rest of the new plan %7.3f ms  end levels 0..6 %s  [checked %d docs]"
                    % (N, ov, mt, t_old, nc_old, t_new, nc, t_new / t_old, t_new - t_plane, hist, len(sample)))
        b.close()

    text, doc_off = bench.make_corpus("mixed", args.docs, 3, min(16, len(os.sched_getaffinity(0))))
    run_case("corpus.mixed (headline)", np.ascontiguousarray(text), np.ascontiguousarray(doc_off), args.iters, args.sample)
    if args.long_mb > 0:
        from jtokkit_amd import corpus
        n = int(args.long_mb * 1e6 / 4096)
        t1, off1 = corpus.mixed(n, mean_bytes=4096, seed=44)
        t1 = np.ascontiguousarray(t1, dtype=np.uint8)
        # every step of the one workgroup's chain depends on the one before: slow by construction, so few iterations
        run_case("one long document", t1, np.array([0, len(t1)], dtype=np.int64), max(1, min(args.iters, 2)), 1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
