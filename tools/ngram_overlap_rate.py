"""n-gram sets and overlap of a device-resident batch (jtk_ngram_set_add_batch, jtk_batch_ngram_overlap) beside the encode of the
same batch, on the headline corpus (corpus.mixed, cl100k_base, encodeOrdinary), n = 13.

Per set -- the empty one, and sets built from a seeded sample of the documents (0.01 %: a 1 MB table, inside the 4 MB L2;
0.1 %: 8 MB, past L2 and inside the 256 MB Infinity Cache; 10 %: 1 GB, past both) --: the first insert of the sample's batch
into a fresh set (host clock around the call and a synchronise: it holds the count kernel, the call's waits, the table's
allocation and the rehash), the same insert repeated into a second set (HIP events, every key already present), and the
overlap with all four outputs and with the flags alone (HIP events over --iters calls after warm-up), each beside the encode
of the batch it reads, timed in the same session; for scale, jtk_batch_minhash with K = 64.
The set's size is checked against the distinct keys computed here with numpy, and the overlap of a seeded sample of documents
against the CPU restatement (tests/ngram_ref.py) in every row.  Per-kernel times come from running this tool under
`rocprofv3 --kernel-trace --stats`.  Writes its lines to --out as well.

  python tools/ngram_overlap_rate.py [--docs 200000] [--fractions 0,0.0001,0.001,0.1] [--ngram 13] [--iters 10]
"""
import argparse
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

G = np.uint64(0x9E3779B97F4A7C15)


def mix_array(x):
    x = x ^ (x >> np.uint64(30))
    x = x * np.uint64(0xBF58476D1CE4E5B9)
    x = x ^ (x >> np.uint64(27))
    x = x * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def batch_keys(tokens, tok_off, n, key):
    """k of every n-gram of a batch (uint64 array, document order), with numpy: the windows of the flat token array that lie
    inside one document."""
    t = (tokens.astype(np.int64) & 0xFFFFFFFF).astype(np.uint64) + np.uint64(1)
    count = len(t) - n + 1
    if count <= 0:
        return np.zeros(0, dtype=np.uint64)
    h = np.zeros(count, dtype=np.uint64)
    for j in range(n):
        h = h * G + t[j:j + count]
    k = mix_array(h ^ np.uint64(key))
    k[k == 0] = G
    doc = np.searchsorted(tok_off, np.arange(count), side="right") - 1
    return k[np.arange(count) + n <= tok_off[doc + 1]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=200000)
    ap.add_argument("--fractions", default="0,0.0001,0.001,0.1")
    ap.add_argument("--ngram", type=int, default=13)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sample", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ngram_overlap_rate.txt"))
    args = ap.parse_args()
    import torch
    import bench
    import ngram_ref as ref
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
    n = args.ngram
    key = ref.key_of(args.seed, n)
    sig = torch.empty((n_docs, 64), dtype=torch.int32, device=dev)
    t_mh = timed(lambda: b.minhash(sig.data_ptr(), 5, 64, 0, args.seed, None, None, sp), args.iters)
    lens = np.diff(tokens.tok_off)
    n_grams = int(np.maximum(lens - n + 1, 0).sum())
    say("corpus.mixed (headline): %d documents, %.1f MB, %d tokens, %d n-grams of %d tokens; encode %.3f ms; for scale, minhash K=64 ngram=5 %.3f ms"
        % (n_docs, len(text) / 1e6, nt, n_grams, n, t_enc, t_mh))
    one = tokens.doc(0).tolist()
    assert [int(x) for x in batch_keys(np.array(one, dtype=np.int32), np.array([0, len(one)]), n, key)] == ref.doc_keys([one], [0], args.seed, n)
    rng = random.Random(5)
    sample = sorted(rng.sample(range(n_docs), min(args.sample, n_docs)))
    flags = torch.empty(nt, dtype=torch.uint8, device=dev)
    n_hit = torch.empty(n_docs, dtype=torch.int32, device=dev)
    n_cov = torch.empty(n_docs, dtype=torch.int32, device=dev)
    first = torch.empty(n_docs, dtype=torch.int64, device=dev)
    sb = enc.new_batch()
    for frac in [float(x) for x in args.fractions.split(",")]:
        pick = sorted(random.Random(7).sample(range(n_docs), int(round(frac * n_docs))))
        s = enc.ngram_set(n, args.seed)
        t_senc = t_first = t_again = 0.0
        src_keys = np.zeros(0, dtype=np.uint64)
        src_tokens = n_src = 0
        if pick:
            parts = [text[doc_off[d]:doc_off[d + 1]] for d in pick]
            s_off = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
            s_text = np.concatenate(parts)
            ds_text = torch.zeros(len(s_text) + 32, dtype=torch.uint8, device=dev)
            ds_text[:len(s_text)].copy_(torch.from_numpy(s_text))
            ds_off = torch.from_numpy(s_off).to(dev)
            torch.cuda.synchronize()
            t_senc = timed(lambda: sb.encode_device(ds_text.data_ptr(), ds_off.data_ptr(), len(pick), len(s_text), True, stream=sp, sync=False), args.iters)
            src_tokens = sb.result()[0]
            stream.synchronize()
            t0 = time.perf_counter()
            s.add_last_encode(sb, sp)
            stream.synchronize()
            t_first = (time.perf_counter() - t0) * 1e3
            again = enc.ngram_set(n, args.seed)               # (a set of its own: inserting twice would double the measured table)
            t_again = timed(lambda: again.add_last_encode(sb, sp), args.iters)
            again.close()
            src = sb.fetch()
            n_src = int(np.maximum(np.diff(src.tok_off) - n + 1, 0).sum())
            src_keys = np.unique(batch_keys(src.tokens, src.tok_off, n, key))
        assert len(s) == len(src_keys), (frac, len(s), len(src_keys))
        cap = s.capacity
        assert cap == ref.capacity(0, n_src)
        t_ov = timed(lambda: b.ngram_overlap(s, flags.data_ptr(), n_hit.data_ptr(), n_cov.data_ptr(), first.data_ptr(), sp), args.iters)
        t_fl = timed(lambda: b.ngram_overlap(s, flags.data_ptr(), None, None, None, sp), args.iters)
        stream.synchronize()
        got_hit, got_cov, got_first, got_flags = n_hit.cpu().numpy(), n_cov.cpu().numpy(), first.cpu().numpy(), flags.cpu().numpy()
        for d in sample:
            ids = tokens.doc(d).tolist()
            mine = ref.Set(args.seed, n)
            ks = batch_keys(np.array(ids, dtype=np.int32), np.array([0, len(ids)]), n, key)
            at = np.minimum(np.searchsorted(src_keys, ks), max(len(src_keys) - 1, 0))
            mine.keys = set(int(k) for k in ks[src_keys[at] == ks]) if len(src_keys) else set()
            exp = ref.overlap([ids], [0], mine)
            lo, hi = tokens.tok_off[d], tokens.tok_off[d + 1]
            assert np.array_equal(got_flags[lo:hi], exp.flags) and got_hit[d] == exp.n_hit[0] and got_cov[d] == exp.n_covered[0] \
                and got_first[d] == exp.first_hit[0], (frac, d)
        say("  set from %5.2f %% of the documents: %d keys in %d slots (%.1f MB); source batch %d tokens, encode %.3f ms, first insert %.3f ms "
            "(host clock), insert again %.3f ms (%.2f x its encode)" % (100 * frac, len(s), cap, cap * 8 / 1e6, src_tokens, t_senc, t_first, t_again,
                                                                        t_again / t_senc if t_senc else 0.0))
        say("      overlap %7.3f ms (%.2f x the encode, %.2f x minhash K=64; %.1f G tokens/s); flags only %7.3f ms; %d starts flagged, %d tokens "
            "covered  [checked %d docs]" % (t_ov, t_ov / t_enc, t_ov / t_mh, nt / 1e9 / t_ov * 1e3, t_fl, int(got_hit.sum()), int(got_cov.sum()), len(sample)))
        s.close()
    sb.close()
    b.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
