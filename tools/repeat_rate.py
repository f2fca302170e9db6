"""Repeated n-grams inside a document (jtk_batch_ngram_repeats) on a device-resident batch, beside the encode of the same batch
and beside the yardstick of the same hashing: NgramSet.add_last_encode (one CAS per n-gram) + Batch.ngram_overlap (one probe
per n-gram) of the same batch.  cl100k_base, encodeOrdinary.

Two corpora: the headline one (corpus.mixed) and a repetitive one, in which every second document is replaced by one short
phrase repeated to the same length -- what the pass exists to find, and where every atomic of pass 1 goes to a handful of
slots.  Per corpus n = 3 and n = 10 at three table budgets: 4 MiB (the table of a group inside the L2), 64 MiB (inside the 256
MB Infinity Cache) and 16 GiB (the whole batch one group).  Times are HIP events over --iters calls after warm-up; the pass's
calls include its two host waits.  A seeded sample of documents is checked against the CPU restatement (tests/repeat_ref.py)
in every row.  Writes its lines to --out as well.

  python tools/repeat_rate.py [--docs 50000] [--ngrams 3,10] [--budgets 4,64,256,1024,16384] [--iters 10]
"""
import argparse
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PHRASES = [b"Click here ", b"Buy now and save! ", b"la ", b"Home | About | Contact | ", b"0 "]


def repetitive(text, doc_off):
    """Every second document replaced by one phrase repeated to the document's length."""
    out = text.copy()
    for d in range(0, len(doc_off) - 1, 2):
        lo, hi = int(doc_off[d]), int(doc_off[d + 1])
        ph = np.frombuffer(PHRASES[(d // 2) % len(PHRASES)], dtype=np.uint8)
        if hi > lo:
            out[lo:hi] = np.resize(ph, hi - lo)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=50000)
    ap.add_argument("--ngrams", default="3,10")
    ap.add_argument("--budgets", default="4,64,256,1024,16384", help="table budgets in MiB")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sample", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "repeat_rate.txt"))
    args = ap.parse_args()
    import torch
    import bench
    import repeat_ref as ref
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
    n_docs = len(doc_off) - 1
    rng = random.Random(5)
    sample = sorted(rng.sample(range(n_docs), min(args.sample, n_docs)))
    for name, tx in (("corpus.mixed (headline)", text), ("repetitive (every second document one phrase repeated)", repetitive(text, doc_off))):
        d_text = torch.zeros(len(tx) + 32, dtype=torch.uint8, device=dev)
        d_text[:len(tx)].copy_(torch.from_numpy(tx))
        d_off = torch.from_numpy(doc_off).to(dev)
        torch.cuda.synchronize()
        b = enc.new_batch()
        t_enc = timed(lambda: b.encode_device(d_text.data_ptr(), d_off.data_ptr(), n_docs, len(tx), True, stream=sp, sync=False), args.iters)
        nt = b.result()[0]
        tokens = b.fetch()
        say("%s: %d documents, %.1f MB, %d tokens; encode %.3f ms" % (name, n_docs, len(tx) / 1e6, nt, t_enc))
        flags = torch.empty(nt, dtype=torch.uint8, device=dev)
        rows = [torch.empty(n_docs, dtype=torch.int32, device=dev) for _ in range(3)] + [torch.empty(n_docs, dtype=torch.int64, device=dev)]
        ptrs = [flags.data_ptr()] + [t.data_ptr() for t in rows]
        expected = {}                                # the restatement's result per (document, n, mode): the budget does not enter
        for n in [int(x) for x in args.ngrams.split(",")]:
            n_grams = int(np.maximum(np.diff(tokens.tok_off) - n + 1, 0).sum())
            s = enc.ngram_set(n, args.seed)
            s.add_last_encode(b, sp)
            t_add = timed(lambda: s.add_last_encode(b, sp), args.iters)          # (every key present: the CAS walk, no growth)
            t_ov = timed(lambda: b.ngram_overlap(s, flags.data_ptr(), rows[0].data_ptr(), rows[1].data_ptr(), rows[3].data_ptr(), sp), args.iters)
            say("  n = %2d: %d n-grams; yardstick add_last_encode %.3f ms + ngram_overlap %.3f ms = %.3f ms (set of %d keys, %.1f MB)"
                % (n, n_grams, t_add, t_ov, t_add + t_ov, len(s), s.capacity * 8 / 1e6))
            s.close()
            for mib in [int(x) for x in args.budgets.split(",")]:
                b.set_option(N.JTK_OPT_REPEAT_TABLE_BYTES, mib << 20)
                for mark in (False, True):
                    t = timed(lambda: b.ngram_repeats(n, *ptrs, seed=args.seed, mark_first=mark, stream=sp), args.iters)
                    stream.synchronize()
                    got = [flags.cpu().numpy()] + [r.cpu().numpy() for r in rows]
                    for d in sample:
                        if (d, n, mark) not in expected:
                            expected[d, n, mark] = ref.repeats([tokens.doc(d).tolist()], [0], n, args.seed, d, mark)
                        exp = expected[d, n, mark]
                        lo, hi = tokens.tok_off[d], tokens.tok_off[d + 1]
                        assert np.array_equal(got[0][lo:hi], exp.flags) and all(g[d] == e[0] for g, e in zip(
                            got[1:], (exp.n_repeat, exp.n_covered, exp.top_count, exp.top_first))), (name, n, mib, mark, d)
                    say("      budget %5d MiB, %-10s %8.3f ms (%.2f x the yardstick, %.2f x the encode; %.2f G tokens/s); %d starts, %d tokens "
                        "covered, largest top_count %d  [checked %d docs]"
                        % (mib, "mark_first" if mark else "later only", t, t / (t_add + t_ov), t / t_enc, nt / 1e9 / t * 1e3, int(got[1].sum()),
                           int(got[2].sum()), int(got[3].max()), len(sample)))
        b.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
