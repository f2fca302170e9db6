"""MinHash signatures of a device-resident batch (jtk_batch_minhash) beside the encode of the same batch, on the headline
corpus (corpus.mixed, cl100k_base, encodeOrdinary).

Per num_hashes K, with ngram = 5: the pass without band keys and with bands = K / 8, timed with HIP events on its stream
after warm-up (the call's one wait, for the token count, happens in the first call only); the shingle x hash evaluations per
second (every shingle takes K multiply-add-shift values and minima); and the bytes the pass writes (the preset and the rows:
2 x 4 K per document, plus 4 for n_shingles and 8 per band key).  The signatures of a seeded sample of documents are checked
against the CPU restatement (tests/minhash_ref.py).  Per-kernel times come from running this tool under
`rocprofv3 --kernel-trace --stats`.  Writes its lines to --out as well.

  python tools/minhash_rate.py [--docs 200000] [--hashes 64,128,256] [--ngram 5] [--iters 10]
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
    ap.add_argument("--hashes", default="64,128,256")
    ap.add_argument("--ngram", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sample", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "minhash_rate.txt"))
    args = ap.parse_args()
    import torch
    import bench
    import minhash_ref as ref
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

    text, doc_off = bench.make_corpus("mixed", args.docs, 3, min(16, len(os.sched_getaffinity(0))))
    text, doc_off = np.ascontiguousarray(text), np.ascontiguousarray(doc_off)
    n_docs = len(doc_off) - 1
    d_text, d_off = torch.from_numpy(text).to(dev), torch.from_numpy(doc_off).to(dev)
    torch.cuda.synchronize()
    b = enc.new_batch()
    t_enc = timed(lambda: b.encode_device(d_text.data_ptr(), d_off.data_ptr(), n_docs, len(text), True, stream=sp, sync=False), args.iters)
    nt = b.result()[0]
    tokens = b.fetch()
    lens = np.diff(tokens.tok_off)
    n = args.ngram
    shingles = int(np.where(lens > 0, lens - np.minimum(lens, n) + 1, 0).sum())
    say("corpus.mixed (headline): %d documents, %.1f MB, %d tokens, %d shingles of %d tokens; encode %.3f ms"
        % (n_docs, len(text) / 1e6, nt, shingles, n, t_enc))
    rng = random.Random(5)
    sample = sorted(rng.sample(range(n_docs), min(args.sample, n_docs)))
    for K in [int(x) for x in args.hashes.split(",")]:
        bands = K // 8
        sig = torch.empty((n_docs, K), dtype=torch.int32, device=dev)
        nsh = torch.empty(n_docs, dtype=torch.int32, device=dev)
        keys = torch.empty((n_docs, bands), dtype=torch.int64, device=dev)
        t_sig = timed(lambda: b.minhash(sig.data_ptr(), n, K, 0, args.seed, nsh.data_ptr(), None, sp), args.iters)
        t_all = timed(lambda: b.minhash(sig.data_ptr(), n, K, bands, args.seed, nsh.data_ptr(), keys.data_ptr(), sp), args.iters)
        stream.synchronize()
        got, got_n = sig[sample].cpu().numpy().view(np.uint32), nsh[sample].cpu().numpy()
        exp = ref.minhash([tokens.doc(d).tolist() for d in sample], args.seed, n, K, bands)
        assert np.array_equal(got, exp.sig) and np.array_equal(got_n, exp.n_shingles), K
        assert np.array_equal(keys[sample].cpu().numpy().view(np.uint64), exp.band_keys), K
        written = n_docs * (8 * K + 4)
        say("  K=%-3d signatures %7.3f ms (%.2f x the encode; %.1f G shingle x hash evaluations/s; %.1f MB written)  with %d band keys "
            "%7.3f ms (+%.1f MB)  [checked %d docs]"
            % (K, t_sig, t_sig / t_enc, shingles * K / 1e9 / t_sig * 1e3, written / 1e6, bands, t_all, n_docs * bands * 8 / 1e6, len(sample)))
    b.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
