"""Allow-special encodes (JTK_ENCODE_ALLOW_SPECIAL, encodeOrdinary segments) of a device-resident batch against the same call
without the flag on the same bytes, cl100k_base:

  none     the headline corpus (corpus.mixed, 200k documents) with no literal
  sprinkle the same with <|endoftext|> written over the text about every 4 KB
  shard    the corpus joined by <|endoftext|> into a few large documents

Each timed with HIP events on a torch stream after warm-up (the call's waits included); results checked on a sample against
the restatement tests/special_ref.py.

  python tools/special_rate.py [--docs 200000] [--iters 10] [--shards 8]
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
    ap.add_argument("--shards", type=int, default=8)
    ap.add_argument("--sample", type=int, default=100)
    args = ap.parse_args()
    import torch
    import bench
    import jtokkit_amd
    import oracle_lib
    import special_ref

    enc = jtokkit_amd.get_encoding("cl100k_base")
    o = oracle_lib.get("cl100k_base")
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(dev)
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
        b.set_allowed_special([100257])
        t_plain = timed(lambda: b.encode_device(d_text.data_ptr(), d_off.data_ptr(), n_docs, len(text), True, stream=sp, sync=False))
        t_sp = timed(lambda: b.encode_device(d_text.data_ptr(), d_off.data_ptr(), n_docs, len(text), True, stream=sp, sync=False,
                                             allow_special=True))
        nt = b.encode_device(d_text.data_ptr(), d_off.data_ptr(), n_docs, len(text), True, stream=sp, allow_special=True)
        res = b.fetch()
        n_sp = int((res.tokens == 100257).sum())
        checked = 0
        for d in random.Random(5).sample(range(n_docs), min(args.sample, n_docs)):
            doc = text[doc_off[d]:doc_off[d + 1]].tobytes()
            if len(doc) > 2_000_000:
                continue
            try:
                exp = special_ref.encode(o, doc, {EOT: 100257}, ordinary=True)
            except oracle_lib.OracleError:                  # (a literal written over a character: a malformed segment)
                continue
            assert res.doc(d).tolist() == exp, (label, d)
            checked += 1
        print("%-9s %7d documents %7.1f MB %10d tokens %8d specials: without flag %7.2f ms, allow-special %7.2f ms (%.2fx)"
              "  [checked %d docs]" % (label, n_docs, len(text) / 1e6, nt, n_sp, t_plain, t_sp, t_sp / t_plain, checked), flush=True)
        b.close()

    text, doc_off = bench.make_corpus("mixed", args.docs, 3, min(16, len(os.sched_getaffinity(0))))
    text, doc_off = np.ascontiguousarray(text, dtype=np.uint8), np.ascontiguousarray(doc_off, dtype=np.int64)
    run_case("none", text, doc_off)
    sprinkled = text.copy()
    rng = np.random.default_rng(5)
    lit = np.frombuffer(EOT, dtype=np.uint8)
    for p in np.sort(rng.choice(len(text) - 64, size=len(text) // 4096, replace=False)):
        sprinkled[p:p + len(lit)] = lit
    run_case("sprinkle", sprinkled, doc_off)
    # shard: documents joined by <|endoftext|>, args.shards large documents
    per = (len(doc_off) - 1 + args.shards - 1) // args.shards
    parts, soff = [], [0]
    for k in range(args.shards):
        d0, d1 = k * per, min(len(doc_off) - 1, (k + 1) * per)
        docs = [text[doc_off[d]:doc_off[d + 1]].tobytes() for d in range(d0, d1)]
        parts.append(EOT.join(docs))
        soff.append(soff[-1] + len(parts[-1]))
    run_case("shard", np.frombuffer(b"".join(parts), dtype=np.uint8).copy(), np.array(soff, dtype=np.int64))


if __name__ == "__main__":
    main()
