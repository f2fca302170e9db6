"""Word-level quality signals (jtk_batch_word_stats) on a device-resident batch, beside the two yardsticks of
tools/line_repeat_rate.py measured in the same session: a device-to-device copy of the text, and the build of the character index
(jtk_batch_char_index) over the same text.  cl100k_base, encodeOrdinary.

Two corpora: the headline one (corpus.mixed) and the repetitive one of tools/line_repeat_rate.py.  Per corpus the nine word outputs
alone (Gopher's stop list, with and without JTK_WORDS_FOLD_ASCII; no stop list) and the five line outputs alone (over a held line
list).  Times are HIP events over --iters calls after warm-up; the call does not wait on the host.  A seeded sample of documents is
checked against the CPU restatement (tests/words_ref.py) in every row.  Writes its lines to --out as well.

  python tools/word_stats_rate.py [--docs 50000] [--iters 10]
"""
import argparse
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=50000)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sample", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "word_stats_rate.txt"))
    args = ap.parse_args()
    import torch
    import bench
    import words_ref as ref
    import jtokkit_amd
    from jtokkit_amd import _native as N
    from line_repeat_rate import repetitive

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
    gopher = tuple(w.encode() for w in jtokkit_amd.GOPHER_STOP_WORDS)
    for name, tx in (("corpus.mixed (headline)", text), ("repetitive (every second document one line repeated)", repetitive(text, doc_off))):
        d_text = torch.zeros(len(tx) + 32, dtype=torch.uint8, device=dev)
        d_text[:len(tx)].copy_(torch.from_numpy(tx))
        d_copy = torch.empty_like(d_text)
        d_off = torch.from_numpy(doc_off).to(dev)
        torch.cuda.synchronize()
        b = enc.new_batch()
        t_enc = timed(lambda: b.encode_device(d_text.data_ptr(), d_off.data_ptr(), n_docs, len(tx), True, stream=sp, sync=False))
        b.result()
        with torch.cuda.stream(stream):
            t_copy = timed(lambda: d_copy.copy_(d_text))
        turn = [0]

        def index():                             # (another unit every call: the index is rebuilt, never served from the batch)
            turn[0] ^= 1
            b.char_index(("utf16", "char")[turn[0]], None, sp)
        t_index = timed(index)
        say("%s: %d documents, %.1f MB; encode %.3f ms; yardsticks: device-to-device copy %.3f ms, char_index build %.3f ms"
            % (name, n_docs, len(tx) / 1e6, t_enc, t_copy, t_index))
        n_lines = b.line_units("line", True, 0, 0, sp)
        out = {k: torch.zeros(n_docs, dtype=torch.int64 if dt == "int64" else torch.int32, device=dev) for k, dt in N.WORDS_OUT_TYPES}
        word_ptrs = {k: t.data_ptr() for k, t in out.items() if k not in N.WORDS_LINE_FIELDS}
        line_ptrs = {k: t.data_ptr() for k, t in out.items() if k in N.WORDS_LINE_FIELDS}
        for label, stops, fold, ptrs in (("words, Gopher's stop list", gopher, False, word_ptrs), ("words, the list with FOLD_ASCII", gopher, True, word_ptrs),
                                         ("words, no stop list", (), False, word_ptrs), ("lines (%d held units)" % n_lines, gopher, False, line_ptrs)):
            t = timed(lambda: b.word_stats(stops, fold, 30, sp, **ptrs))
            stream.synchronize()
            got = {k: v.cpu().numpy() for k, v in out.items() if k in ptrs}
            for d in sample:
                exp = ref.stats([tx[int(doc_off[d]):int(doc_off[d + 1])].tobytes()], [0], stops, fold, 30)
                for k in got:
                    assert int(got[k][d]) & 0xFFFFFFFFFFFFFFFF == int(exp[k][0]) & (0xFFFFFFFF if k == "stop_mask" else 0xFFFFFFFFFFFFFFFF) or \
                        int(got[k][d]) & 0xFFFFFFFF == int(exp[k][0]), (name, label, d, k, got[k][d], exp[k][0])
            say("    %-34s %8.3f ms (%.2f x the copy, %.2f x char_index; %.1f GB/s)  [checked %d docs]"
                % (label, t, t / t_copy, t / t_index, len(tx) / 1e6 / t, len(sample)))
        b.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
