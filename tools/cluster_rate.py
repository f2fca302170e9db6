"""Near-duplicate clusters of a device-resident batch (jtk_batch_minhash_cluster) on the headline corpus (corpus.mixed,
cl100k_base, encodeOrdinary), beside the path it stands next to (HipEncoding.near_duplicates: a sort per band, unique, and a
union-find on the host).

With ngram = 5, K = 128, B = 16, threshold 0.8, on the slice as it is and with a seeded share of its documents replaced by
edited copies of earlier ones: the signature pass and the cluster call -- with the default table budget and with one band per
group --, each timed with HIP events on its stream after warm-up; then one whole near_duplicate_clusters call and one whole
near_duplicates call on the same texts, by the host clock around calls that end in the copy of the labels.  The labels of the
whole batch are compared between the two budgets, and the labels and representatives of a seeded sample of rows, clustered on
their own, against the CPU restatement (tests/cluster_ref.py).  Per-kernel times come from running this tool under
`rocprofv3 --kernel-trace --stats`.  Writes its lines to --out as well.

  python tools/cluster_rate.py [--docs 200000] [--hashes 128] [--bands 16] [--threshold 0.8] [--iters 10]
"""
import argparse
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=200000)
    ap.add_argument("--hashes", type=int, default=128)
    ap.add_argument("--bands", type=int, default=16)
    ap.add_argument("--ngram", type=int, default=5)
    ap.add_argument("--threshold", type=float, default=0.8)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sample", type=int, default=5000)
    ap.add_argument("--dups", type=float, default=0.1, help="share of planted near-duplicates in the second run")
    ap.add_argument("--skip-old", action="store_true", help="do not time HipEncoding.near_duplicates")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cluster_rate.txt"))
    args = ap.parse_args()
    import torch
    import bench
    import cluster_ref as ref
    import jtokkit_amd
    N = jtokkit_amd._native

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

    def planted(text, doc_off, share):
        """The slice with a seeded share of its documents replaced by copies of earlier ones in which a few letters are changed."""
        rng = np.random.default_rng(11)
        n = len(doc_off) - 1
        docs = [text[doc_off[d]:doc_off[d + 1]] for d in range(n)]
        for d in np.sort(rng.choice(np.arange(1, n), int(share * n), replace=False)):
            copy = docs[int(rng.integers(0, d))].copy()
            at = rng.integers(0, max(1, len(copy)), size=4)
            at = at[(copy[at] >= 97) & (copy[at] <= 122)] if len(copy) else at[:0]
            copy[at] = 120
            docs[d] = copy
        off = np.zeros(n + 1, dtype=np.int64)
        np.cumsum([len(x) for x in docs], out=off[1:])
        return np.concatenate(docs), off

    def measure(tag, text, doc_off):
        n = len(doc_off) - 1
        K, B, m = args.hashes, args.bands, int(math.ceil(args.threshold * args.hashes))
        d_text, d_off = torch.from_numpy(text).to(dev), torch.from_numpy(doc_off).to(dev)
        torch.cuda.synchronize()
        b = enc.new_batch()
        b.encode_device(d_text.data_ptr(), d_off.data_ptr(), n, len(text), True, stream=sp, sync=False)
        sig = torch.empty((n, K), dtype=torch.int32, device=dev)
        nsh = torch.empty(n, dtype=torch.int32, device=dev)
        keys = torch.empty((n, B), dtype=torch.int64, device=dev)
        t_sig = timed(lambda: b.minhash(sig.data_ptr(), args.ngram, K, B, args.seed, nsh.data_ptr(), keys.data_ptr(), sp), args.iters)
        say("%s: %d documents, %.1f MB; K = %d, B = %d, min_agree = %d; signatures and band keys %.3f ms"
            % (tag, n, len(text) / 1e6, K, B, m, t_sig))

        cap = max(64, 1 << (2 * n - 1).bit_length())
        labels = {}
        for what, budget in (("default budget", 256 << 20), ("one band per group", cap * 16 + 8)):
            b.set_option(N.JTK_OPT_REPEAT_TABLE_BYTES, budget)
            groups = -(-B // max(1, min(B, budget // (cap * 16 + 8))))
            lab = torch.empty(n, dtype=torch.int64, device=dev)
            rep = torch.empty((n, B), dtype=torch.int64, device=dev)
            run = lambda: b.minhash_cluster(sig.data_ptr(), keys.data_ptr(), n, K, B, m, lab.data_ptr(), nsh.data_ptr(), rep.data_ptr(), sp)
            t = timed(run, args.iters)
            stream.synchronize()
            labels[what] = lab.cpu().numpy()
            cand = int(((rep >= 0) & (rep < torch.arange(n, device=dev)[:, None])).sum())
            say("  jtk_batch_minhash_cluster, %s (%d group%s of bands, table %.1f MB): %.3f ms for %d (document, band) keys, %d of them "
                "with an earlier representative" % (what, groups, "" if groups == 1 else "s", min(budget, B * (cap * 16 + 8)) / 1e6, t, n * B, cand))
        lab = labels["default budget"]
        assert np.array_equal(lab, labels["one band per group"])
        sizes = np.bincount(lab, minlength=n)
        say("  clusters: %d documents in %d clusters of 2 or more, the largest of %d; the two budgets give the same labels"
            % (int(sizes[sizes > 1].sum()), int((sizes > 1).sum()), int(sizes.max())))

        # a seeded sample of rows, clustered on its own on the device and by the restatement: members of the clusters found above, so
        # that the sample has pairs to verify, and random documents
        rng = np.random.default_rng(5)
        pick = np.union1d(np.flatnonzero(sizes[lab] > 1)[:args.sample // 2], rng.choice(n, min(args.sample, n), replace=False))
        idx = torch.from_numpy(pick).to(dev)
        s_sig, s_keys, s_nsh = sig[idx].contiguous(), keys[idx].contiguous(), nsh[idx].contiguous()
        torch.cuda.synchronize()                     # (the gathers ran on torch's stream)
        with torch.cuda.stream(stream):
            got_lab, got_rep = enc.minhash_cluster_device(s_sig, s_keys, args.threshold, s_nsh, return_rep=True)
        stream.synchronize()
        want_lab, want_rep = ref.cluster(s_sig.cpu().numpy().view(np.uint32), s_keys.cpu().numpy().view(np.uint64), m, s_nsh.cpu().numpy())
        assert np.array_equal(got_lab.cpu().numpy(), want_lab) and np.array_equal(got_rep.cpu().numpy(), want_rep)
        say("  checked against tests/cluster_ref.py: %d sampled rows, %d of them in clusters of 2 or more there"
            % (len(pick), int((np.bincount(want_lab, minlength=len(pick))[want_lab] > 1).sum())))
        b.close()

        texts = [text[doc_off[d]:doc_off[d + 1]].tobytes() for d in range(n)]
        kw = dict(threshold=args.threshold, ngram=args.ngram, num_hashes=K, bands=B, seed=args.seed)
        enc.near_duplicate_clusters(texts[:1000], **kw)                    # (warm-up)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        new = enc.near_duplicate_clusters(texts, **kw)
        t_new = time.perf_counter() - t0
        assert np.array_equal(new, lab)
        say("  near_duplicate_clusters(texts), whole call by the host clock (join, upload, encode, signatures, clusters, labels to the "
            "host): %.1f ms" % (t_new * 1e3))
        if not args.skip_old:
            enc.near_duplicates(texts[:1000], **kw)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            old = enc.near_duplicates(texts, **kw)
            t_old = time.perf_counter() - t0
            say("  near_duplicates(texts), the same: %.1f ms; %d documents labelled differently by the two rules"
                % (t_old * 1e3, int((old != new).sum())))

    measure("corpus.mixed (headline)", text, doc_off)
    measure("the same with %d%% of the documents replaced by edited copies of earlier ones" % round(100 * args.dups), *planted(text, doc_off, args.dups))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
