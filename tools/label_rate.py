"""Training labels of a device-resident batch (jtk_batch_token_spans, jtk_batch_pack_labels) on the headline corpus
(corpus.mixed, cl100k_base, encodeOrdinary, <|endoftext|> after every document), one span per document over its second half (a
completion after a prompt), against the kernels they share their walk with, in the same process on the same encode and plan:

  k_lb_spans  against  k_ck_tokpos (jtk_batch_token_offsets): the same pass over the token tiles; writes 4 B per token where
              k_ck_tokpos writes 8, and reads the span arrays in addition.
  k_lb_pack   against  k_pk_write with rows and positions (jtk_batch_pack_write): the same cell walk; one store stream instead
              of two, one more int32 read per cell.

Each is timed with HIP events on its stream after warm-up, `--reps` times, the two alternating.  The margin of a comparison is
the run-to-run spread (max - min over the repetitions) of the baseline kernel in this same run.  tok_span and a seeded sample of
label rows are checked against the restatement (tests/label_ref.py, tests/pack_ref.py) on the encode's own tokens.

  python tools/label_rate.py [--docs 200000] [--sizes 2048,8192] [--iters 10] [--reps 3]
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
IGN = -100


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=200000)
    ap.add_argument("--sizes", default="2048,8192")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
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

    def compare(name, new, base_name, base):
        tn, tb = [], []
        for _ in range(args.reps):                # alternating: both see the same neighbours
            tb.append(timed(base))
            tn.append(timed(new))
        spread = max(tb) - min(tb)
        d = min(tn) - min(tb)
        print("    %-10s %s ms   %-11s %s ms   spread %.4f ms   difference %+.4f ms: %s"
              % (name, " ".join("%.4f" % t for t in tn), base_name, " ".join("%.4f" % t for t in tb), spread, d,
                 "slower than the baseline by more than its spread" if d > spread else "within the spread or faster"), flush=True)

    text, doc_off = bench.make_corpus("mixed", args.docs, 3, min(16, len(os.sched_getaffinity(0))))
    text, doc_off = np.ascontiguousarray(text), np.ascontiguousarray(doc_off)
    n_docs = len(doc_off) - 1
    d_text, d_off = torch.from_numpy(text).to(dev), torch.from_numpy(doc_off).to(dev)
    begin = (doc_off[:-1] + doc_off[1:]) // 2
    end = doc_off[1:].copy()
    d_b, d_e = torch.from_numpy(begin).to(dev), torch.from_numpy(end).to(dev)
    b = enc.new_batch()
    nt = b.encode_device(d_text.data_ptr(), d_off.data_ptr(), n_docs, len(text), True, stream=sp)
    res = b.fetch()
    print("corpus.mixed (headline): %d documents, %.1f MB, %d tokens, %d spans" % (n_docs, len(text) / 1e6, nt, n_docs), flush=True)
    d_pos = torch.empty(nt, dtype=torch.int64, device=dev)
    d_ts = torch.empty(nt, dtype=torch.int32, device=dev)
    b.token_offsets(d_pos.data_ptr(), stream=sp)   # (the byte scan: both passes reuse it from here on)
    print("  span pass (%.2f GB read and written by k_lb_spans, %.2f GB by k_ck_tokpos)" % ((8.0 * nt + 16.0 * n_docs) / 1e9, 12.0 * nt / 1e9))
    compare("k_lb_spans", lambda: b.token_spans(d_b.data_ptr(), d_e.data_ptr(), n_docs, "whole", d_ts.data_ptr(), stream=sp),
            "k_ck_tokpos", lambda: b.token_offsets(d_pos.data_ptr(), stream=sp))
    stream.synchronize()
    # tok_span against the restatement, from the positions of the tokens by a cumulative sum of their decoded lengths
    import oracle_lib
    o = oracle_lib.get("cl100k_base")
    tl = np.zeros(int(res.tokens.max()) + 1, dtype=np.int64)
    for t in np.unique(res.tokens):
        tl[t] = len(o.decode_bytes([int(t)]))
    lens = tl[res.tokens]
    q = np.cumsum(lens)
    doc_of = np.repeat(np.arange(n_docs), np.diff(res.tok_off))
    base = doc_off[:-1] - np.concatenate([[0], q])[res.tok_off[:-1]]
    p = q - lens + base[doc_of]
    exp_ts = np.where((begin[doc_of] <= p) & (p + lens <= end[doc_of]), doc_of, -1).astype(np.int32)
    ts = d_ts.cpu().numpy()
    assert np.array_equal(ts, exp_ts), "tok_span differs from the restatement"
    U = res.tok_off[:-1] + np.arange(n_docs)
    unit_lens = np.diff(res.tok_off) + 1
    S_lab = np.insert(np.where(ts >= 0, res.tokens, IGN), res.tok_off[1:], IGN)
    rng = random.Random(5)
    for L in [int(x) for x in args.sizes.split(",")]:
        for whole in (False, True):
            nr, ns, _ = b.pack(L, EOT_ID, whole, stream=sp)
            rows = torch.empty(nr * L, dtype=torch.int32, device=dev)
            pos = torch.empty(nr * L, dtype=torch.int32, device=dev)
            lab = torch.empty(nr * L, dtype=torch.int32, device=dev)
            print("  L=%-5d %-6s rows=%-7d (%.2f GB by k_lb_pack, %.2f GB by k_pk_write)"
                  % (L, "whole" if whole else "concat", nr, (8.0 * nt + 4.0 * nr * L) / 1e9, (4.0 * nt + 8.0 * nr * L) / 1e9), flush=True)
            compare("k_lb_pack", lambda: b.pack_labels(d_ts.data_ptr(), IGN, lab.data_ptr(), stream=sp),
                    "k_pk_write", lambda: b.pack_write(-1, rows.data_ptr(), pos.data_ptr(), stream=sp))
            stream.synchronize()
            a = pack_ref.row_starts(unit_lens.tolist(), L, whole)
            assert nr == len(a) - 1
            labels = lab.view(nr, L)
            for r in rng.sample(range(nr), min(args.sample, nr)):
                exp, _ = pack_ref.row(S_lab, U, a, r, L, IGN)
                assert np.array_equal(labels[r].cpu().numpy(), exp), (L, whole, r)
            del rows, pos, lab, labels
            torch.cuda.empty_cache()
    b.close()


if __name__ == "__main__":
    main()
