"""Phrase hits (jtk_batch_phrase_hits) on a device-resident batch of the headline corpus (corpus.mixed), beside the yardstick of the
same text in the same run: the word pass (jtk_batch_word_stats, the nine word outputs, Gopher's stop list), which reads the same
bytes once and does more per byte.  cl100k_base, encodeOrdinary.

Two sets: C4_PHRASES with JTK_PHRASE_FOLD_ASCII (nine phrases: the edge table is staged in LDS) and 20,000 seeded random lowercase
phrases of 6..12 bytes (the table is probed in global memory).  Per set the four per-document outputs alone, and all six over a held
list of trimmed lines.  Times are HIP events over --iters calls after warm-up, the rows alternating --rounds times (the spread is
printed); the call does not wait on the host.  A seeded sample of documents is checked against the CPU restatement
(tests/phrase_ref.py) in every row.  Writes its lines to --out as well.

  python tools/phrase_hits_rate.py [--docs 50000] [--iters 10]
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
    ap.add_argument("--docs", type=int, default=50000)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sample", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "phrase_hits_rate.txt"))
    args = ap.parse_args()
    import torch
    import bench
    import phrase_ref as ref
    import jtokkit_amd
    from jtokkit_amd import _native as N

    enc = jtokkit_amd.get_encoding("cl100k_base")
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(dev)              # (a real stream: the library reads a NULL handle as the batch's own stream)
    sp = stream.cuda_stream
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

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
    text, doc_off = np.ascontiguousarray(text), np.ascontiguousarray(doc_off)
    n_docs = len(doc_off) - 1
    sample = sorted(random.Random(5).sample(range(n_docs), min(args.sample, n_docs)))
    rng = random.Random(11)
    many = [("".join(rng.choice("abcdefghijklmnopqrstuvwxyz") for _ in range(rng.randint(6, 12))).encode(), rng.randrange(32)) for _ in range(20000)]
    c4 = [(p.encode(), g) for p, g in jtokkit_amd.C4_PHRASES]
    d_text = torch.zeros(len(text) + 32, dtype=torch.uint8, device=dev)
    d_text[:len(text)].copy_(torch.from_numpy(text))
    d_off = torch.from_numpy(doc_off).to(dev)
    torch.cuda.synchronize()
    b = enc.new_batch()
    b.encode_device(d_text.data_ptr(), d_off.data_ptr(), n_docs, len(text), True, stream=sp, sync=False)
    b.result()
    n_units = b.line_units("line", True, 0, 0, sp)
    say("corpus.mixed (headline): %d documents, %.1f MB, %d trimmed lines held" % (n_docs, len(text) / 1e6, n_units))
    words = {k: torch.zeros(n_docs, dtype=torch.int64 if dt == "int64" else torch.int32, device=dev) for k, dt in N.WORDS_OUT_TYPES
             if k not in N.WORDS_LINE_FIELDS}
    gopher = tuple(w.encode() for w in jtokkit_amd.GOPHER_STOP_WORDS)
    rows = [("word_stats, nine word outputs (yardstick)", lambda: b.word_stats(gopher, False, 0, sp, **{k: t.data_ptr() for k, t in words.items()}), None)]
    for label, phrases, fold in (("C4_PHRASES folded, table in LDS", c4, True), ("20,000 random phrases, table in global", many, False)):
        ps = enc.phrase_set(phrases, fold_ascii=fold)
        out = {k: torch.zeros(n_units if k == "unit_mask" else n_docs, dtype=torch.int64 if dt == "int64" else torch.int32, device=dev)
               for k, dt in N.PHRASE_OUT_TYPES}
        doc_ptrs = {k: t.data_ptr() for k, t in out.items() if k not in N.PHRASE_UNIT_FIELDS}
        all_ptrs = {k: t.data_ptr() for k, t in out.items()}
        say("    set: %s: %d distinct phrases, %d states" % (label, len(ps), ps.n_states))
        rows.append(("phrase_hits, %s, per document" % label, lambda ps=ps, p=doc_ptrs: b.phrase_hits(ps, sp, **p), (phrases, fold, out, ps)))
        rows.append(("phrase_hits, %s, + units" % label, lambda ps=ps, p=all_ptrs: b.phrase_hits(ps, sp, **p), (phrases, fold, out, ps)))
    times = [[timed(fn) for _, fn, _ in rows] for _ in range(args.rounds)]               # (the rows alternate inside a round)
    t_words = min(t[0] for t in times)
    for i, (label, fn, chk) in enumerate(rows):
        ts = sorted(t[i] for t in times)
        if chk:
            phrases, fold, out, _ = chk
            fn()
            stream.synchronize()
            got = {k: v.cpu().numpy() for k, v in out.items()}
            for d in sample:
                exp = ref.hits([text[int(doc_off[d]):int(doc_off[d + 1])].tobytes()], [0], phrases, fold, False)
                for k in ("group_mask", "n_hits", "first_hit", "first_which"):
                    assert int(got[k][d]) & 0xFFFFFFFF == int(exp[k][0]) & 0xFFFFFFFF, (label, d, k, got[k][d], exp[k][0])
        say("    %-72s min %8.3f ms, median %8.3f, max %8.3f (%.2f x word_stats; %.1f GB/s)%s"
            % (label, ts[0], ts[len(ts) // 2], ts[-1], ts[0] / t_words, len(text) / 1e6 / ts[0], "  [checked %d docs]" % len(sample) if chk else ""))
    b.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
