"""Best-fit-decreasing rows (jtk_batch_pack_best_fit) against next-fit of whole documents (JTK_PACK_WHOLE_DOCS, the yardstick)
in the same run, on the headline corpus (corpus.mixed, cl100k_base, encodeOrdinary, EOS separator) and on the driver's worst
case: rests that are all distinct and longer than L / 2.

Per L: rows and pad share of both placements, the lower bound ceil(cells / L), the driver's step count (from the CPU shim
tests/pack_fit_sim on the same token counts: the library exports no counter), and plan and write times of both, each timed with
HIP events on its stream after warm-up (the plan's one wait included).  The tool asserts that best fit gives no more rows than
next-fit.  Writes its lines to --out as well.

  python tools/pack_fit_rate.py [--docs 200000] [--lens 2048,8192] [--iters 10]
"""
import argparse
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
EOT_ID = 100257


def shim_steps(tok_off, L):
    """(rows, steps) of the rule header's driver on the CPU for documents of these token counts (EOS separator)."""
    out = os.path.join(tempfile.mkdtemp(), "libpack_fit_sim.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", out,
                           os.path.join(ROOT, "tests", "pack_fit_sim", "pack_fit_sim.cpp")])
    lib = C.CDLL(out)
    lib.sim_fit_counts.restype = None
    lib.sim_fit_counts.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int, C.c_void_p]
    n = len(tok_off) - 1
    status, counts = np.zeros(n + 1, dtype=np.int32), np.zeros(4, dtype=np.int64)
    lib.sim_fit_counts(None, tok_off.ctypes.data, status.ctypes.data, n, L, EOT_ID, 0, counts.ctypes.data)
    return int(counts[0]), int(counts[3])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=200000)
    ap.add_argument("--lens", default="2048,8192")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pack_fit_rate.txt"))
    args = ap.parse_args()
    import torch
    import bench
    import jtokkit_amd

    enc = jtokkit_amd.get_encoding("cl100k_base")
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

    def run_case(label, text, doc_off, Ls):
        n_docs = len(doc_off) - 1
        d_text, d_off = torch.from_numpy(text).to(dev), torch.from_numpy(doc_off).to(dev)
        torch.cuda.synchronize()
        b = enc.new_batch()
        nt = b.encode_device(d_text.data_ptr(), d_off.data_ptr(), n_docs, len(text), True, stream=sp)
        tok_off = np.ascontiguousarray(b.fetch().tok_off, dtype=np.int64)
        cells = nt + n_docs
        say("%s: %d documents, %.1f MB, %d tokens, longest unit %d" % (label, n_docs, len(text) / 1e6, nt, int(np.diff(tok_off).max()) + 1))
        for L in Ls:
            res = {}
            for fit in ("next", "best"):
                plan = lambda: b.pack(L, EOT_ID, whole_docs=True, stream=sp, fit=fit)
                t_plan = timed(plan, args.iters)
                nr, ns, _ = plan()
                rows = torch.empty((nr, L), dtype=torch.int32, device=dev)
                pos = torch.empty((nr, L), dtype=torch.int32, device=dev)
                cu = torch.empty(ns + 1, dtype=torch.int32, device=dev)
                sd = torch.empty(ns, dtype=torch.int64, device=dev)
                t_write = timed(lambda: b.pack_write(-1, rows.data_ptr(), pos.data_ptr(), cu.data_ptr(), sd.data_ptr(), sp), args.iters)
                assert int((rows >= 0).sum()) == cells                       # every token and separator is in a row, once
                res[fit] = (nr, 1.0 - cells / (nr * L), t_plan, t_write)
            sim_rows, steps = shim_steps(tok_off, L)
            assert sim_rows == res["best"][0] and res["best"][0] <= res["next"][0]
            say("  L=%-5d lower bound %d rows | next-fit %d rows, pad %.2f %%, plan %.3f ms, write %.3f ms | best fit %d rows, pad "
                "%.2f %%, plan %.3f ms, write %.3f ms, %d driver steps"
                % ((L, -(-cells // L)) + res["next"] [:1] + (100 * res["next"][1],) + res["next"][2:] + res["best"][:1]
                   + (100 * res["best"][1],) + res["best"][2:] + (steps,)))
        b.close()

    Ls = [int(x) for x in args.lens.split(",")]
    text, doc_off = bench.make_corpus("mixed", args.docs, 3, min(16, len(os.sched_getaffinity(0))))
    run_case("corpus.mixed (headline)", np.ascontiguousarray(text), np.ascontiguousarray(doc_off), Ls)
    # the worst case of the serial driver: units L / 2 + 1 .. L - 1, one document each ("a a a ..." is one token per word)
    L = Ls[-1]
    counts = np.arange(L // 2, L - 1, dtype=np.int64)                        # tokens; the separator makes the unit one longer
    doc_off = np.concatenate([[0], np.cumsum(2 * counts - 1)]).astype(np.int64)
    text = np.frombuffer(b"".join(b"a" + b" a" * int(k - 1) for k in counts), dtype=np.uint8).copy()
    run_case("worst case (all rests distinct, > L / 2)", text, doc_off, [L])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
