"""Duplicate lines and paragraphs inside a document (jtk_batch_line_units, jtk_batch_line_repeats) on a device-resident batch,
beside two yardsticks measured in the same session: a device-to-device copy of the text, and the build of the character index
(jtk_batch_char_index) over the same text -- the closest existing streaming pass over the bytes.  cl100k_base, encodeOrdinary.

Two corpora: the headline one (corpus.mixed) and a repetitive one, in which every second document is replaced by one short line
repeated to the same length (the pair tools/repeat_rate.py uses, with a line break behind every phrase).  Per corpus both units,
line_units and line_repeats apart.  Times are HIP events over --iters calls after warm-up; line_units includes its one host
wait, line_repeats its one.  A seeded sample of documents is checked against the CPU restatement (tests/lines_ref.py) in every
row.  Writes its lines to --out as well.

  python tools/line_repeat_rate.py [--docs 50000] [--iters 10] [--trim]
"""
import argparse
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PHRASES = [b"Click here\n", b"Buy now and save!\n", b"la\n", b"Home | About | Contact\n", b"0\n"]


def repetitive(text, doc_off):
    """Every second document replaced by one line repeated to the document's length."""
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
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sample", type=int, default=16)
    ap.add_argument("--trim", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "line_repeat_rate.txt"))
    args = ap.parse_args()
    import torch
    import bench
    import lines_ref as ref
    import jtokkit_amd

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
    rng = random.Random(5)
    sample = sorted(rng.sample(range(n_docs), min(args.sample, n_docs)))
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
        for unit in ("line", "paragraph"):
            t_units = timed(lambda: b.line_units(unit, args.trim, args.seed, 0, sp))
            nu = b.line_units(unit, args.trim, args.seed, 0, sp)
            out = {"unit_begin": torch.empty(nu, dtype=torch.int64, device=dev), "unit_end": torch.empty(nu, dtype=torch.int64, device=dev),
                   "unit_flags": torch.empty(nu, dtype=torch.uint8, device=dev), "unit_off": torch.empty(n_docs + 1, dtype=torch.int64, device=dev)}
            for k, dt in (("n_dup", torch.int32), ("dup_bytes", torch.int64), ("dup_chars", torch.int64), ("unit_bytes", torch.int64),
                          ("unit_chars", torch.int64), ("doc_chars", torch.int64), ("top_count", torch.int32), ("top_first", torch.int64)):
                out[k] = torch.empty(n_docs, dtype=dt, device=dev)
            ptrs = {k: t.data_ptr() for k, t in out.items() if t.numel()}
            for mark in (False, True):
                t_rep = timed(lambda: b.line_repeats(unit, args.trim, mark, args.seed, 0, sp, **ptrs))
                stream.synchronize()
                got = {k: t.cpu().numpy() for k, t in out.items()}
                for d in sample:
                    lo, hi = int(doc_off[d]), int(doc_off[d + 1])
                    exp = ref.repeats([tx[lo:hi].tobytes()], [0], ref.LINE if unit == "line" else ref.PARAGRAPH, args.trim, mark, args.seed, d)
                    u0, u1 = int(got["unit_off"][d]), int(got["unit_off"][d + 1])
                    assert u1 - u0 == len(exp.unit_begin), (name, unit, mark, d)
                    assert np.array_equal(got["unit_begin"][u0:u1] - lo, exp.unit_begin) and np.array_equal(got["unit_end"][u0:u1] - lo, exp.unit_end)
                    assert np.array_equal(got["unit_flags"][u0:u1], exp.unit_flags), (name, unit, mark, d)
                    for k in ("n_dup", "dup_bytes", "dup_chars", "unit_bytes", "unit_chars", "doc_chars", "top_count", "top_first"):
                        assert got[k][d] == getattr(exp, k)[0], (name, unit, mark, d, k)
                say("    %-9s %-10s line_units %8.3f ms (%.2f x the copy, %.2f x char_index; %.1f GB/s), line_repeats %8.3f ms (%.2f x the copy, "
                    "%.2f x char_index); %d units, %d flagged, largest top_count %d  [checked %d docs]"
                    % (unit, "mark_first" if mark else "later only", t_units, t_units / t_copy, t_units / t_index, len(tx) / 1e6 / t_units,
                       t_rep, t_rep / t_copy, t_rep / t_index, nu, int(got["unit_flags"].sum()), int(got["top_count"].max()), len(sample)))
        b.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
