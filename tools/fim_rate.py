"""Fill-in-the-middle encodes (JTK_ENCODE_FIM) of a device-resident batch against the plain encodeOrdinary call on the same
bytes, cl100k_base, on the headline corpus (corpus.mixed, 200k documents):

  plain      the call without the flag
  fim 0.5    fim_rate 0.5, spm_rate 0.5
  fim 1.0    fim_rate 1.0, spm_rate 0.5
  special    for comparison, measured in the same session: JTK_ENCODE_ALLOW_SPECIAL with one <|endoftext|> per document
             (written over the first bytes of every document long enough)

Each timed with HIP events on a torch stream after warm-up (the call's waits included).  Then one profiled run of each: the
pipeline's stage times (on the documents, or on the 3 n sub-documents) and what is left of the call -- for FIM the cuts, the
stitch (count, scan, gather) and the launches.  The FIM results are checked on a sample against the restatement
tests/fim_ref.py.

  python tools/fim_rate.py [--docs 200000] [--iters 10]
"""
import argparse
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

EOT = b"<|endoftext|>"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=200000)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sample", type=int, default=100)
    args = ap.parse_args()
    import torch
    import bench
    import fim_ref
    import jtokkit_amd
    import oracle_lib

    enc = jtokkit_amd.get_encoding("cl100k_base")
    o = oracle_lib.get("cl100k_base")
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(dev)
    sp = stream.cuda_stream
    ids = enc.fim_ids(jtokkit_amd.FimParams(1.0))

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

    text, doc_off = bench.make_corpus("mixed", args.docs, 3, min(16, len(os.sched_getaffinity(0))))
    text, doc_off = np.ascontiguousarray(text, dtype=np.uint8), np.ascontiguousarray(doc_off, dtype=np.int64)
    n_docs = len(doc_off) - 1
    d_text, d_off = torch.from_numpy(text).to(dev), torch.from_numpy(doc_off).to(dev)
    with_lit = text.copy()
    lit = np.frombuffer(EOT, dtype=np.uint8)
    for d in np.flatnonzero(np.diff(doc_off) >= len(lit)):
        with_lit[doc_off[d]:doc_off[d] + len(lit)] = lit
    d_lit = torch.from_numpy(with_lit).to(dev)
    torch.cuda.synchronize()
    b = enc.new_batch()
    b.set_allowed_special([100257])

    def call(d_t, **kw):
        return lambda sync=False: b.encode_device(d_t.data_ptr(), d_off.data_ptr(), n_docs, len(text), True, stream=sp, sync=sync, **kw)

    def profiled(fn, total_ms):
        b.set_profiling(True)
        fn(sync=True)
        stages = b.kernel_times()
        b.set_profiling(False)
        inside = sum(stages.values())
        print("    pipeline stages: " + ", ".join("%s %.2f" % (k, ms) for k, ms in stages.items()))
        print("    pipeline %.2f ms, the rest of the call %.2f ms" % (inside, total_ms - inside), flush=True)

    print("%d documents, %.1f MB, %d timed calls each" % (n_docs, len(text) / 1e6, args.iters))
    t_plain = timed(call(d_text))
    print("plain     %8.2f ms" % t_plain)
    profiled(call(d_text), t_plain)
    for rate in (0.5, 1.0):
        fim = jtokkit_amd.FimParams(rate, 0.5, seed=1)
        b.set_fim(fim)
        t = timed(call(d_text, fim=True))
        nt = call(d_text, fim=True)(sync=True)
        res, (kind, cut, part_tok) = b.fetch(), b.fim_result()
        checked = 0
        for d in random.Random(5).sample(range(n_docs), min(args.sample, n_docs)):
            doc = text[doc_off[d]:doc_off[d + 1]].tobytes()
            if not fim_ref.well_formed(doc):
                continue
            k, a, c = fim_ref.transform(doc, 1, d, fim_ref.rate_u32(rate), fim_ref.rate_u32(0.5))
            st, exp, count = fim_ref.encode_doc(o.encode_ordinary, doc, k, a, c, ids)
            assert (kind[d], tuple(cut[d]), tuple(part_tok[d])) == (k, (a, c), count) and res.doc(d).tolist() == exp, (rate, d)
            checked += 1
        print("fim %.1f   %8.2f ms (%.2fx)  %d tokens, %d documents cut, %d of them SPM  [checked %d docs]"
              % (rate, t, t / t_plain, nt, int((kind != 0).sum()), int((kind == 2).sum()), checked))
        profiled(call(d_text, fim=True), t)
    t_plain_lit = timed(call(d_lit))
    t_sp = timed(call(d_lit, allow_special=True))
    print("special   %8.2f ms (%.2fx its own call without the flag, %.2f ms)" % (t_sp, t_sp / t_plain_lit, t_plain_lit))
    b.close()


if __name__ == "__main__":
    main()
