"""Exact duplicates across documents (jtk_batch_seen_mark, ADD | QUERY, unit LINE) on a device-resident batch, beside the
per-document pass over the same units measured in the same session: jtk_batch_line_units + jtk_batch_line_repeats on the same
batch.  cl100k_base, encodeOrdinary.  Two corpora (corpus.mixed and corpus.english), then a batch that is one line repeated, with
and without the merge of equal keys inside a workgroup (JTK_SEEN_NO_COMBINE).

Times are HIP events over --iters calls after warm-up, the two passes alternating inside every iteration; every call includes its
host waits.  seen_mark is timed twice: into a fresh set, created and destroyed inside the timed call, so that the time holds the
growth of the table from 64 slots to the batch's size and every claim; and into a set that holds the batch already, which neither
claims nor grows.  Every call takes another doc_index_base, so no pass is served from units the batch still holds.  The flags of
a mark into an empty set are checked against a Python set over the units' bytes.
Writes its lines to --out as well.

  python tools/seen_rate.py [--docs 50000] [--iters 10] [--repeats 1000000]
"""
import argparse
import os
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
    ap.add_argument("--repeats", type=int, default=1000000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seen_rate.txt"))
    args = ap.parse_args()
    import torch
    import bench
    import jtokkit_amd

    enc = jtokkit_amd.get_encoding("cl100k_base")
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(dev)              # (a real stream: the library reads a NULL handle as the batch's own stream)
    sp = stream.cuda_stream
    out_lines = []

    def say(s):
        print(s, flush=True)
        out_lines.append(s)

    def timed(fns):
        """ms per call of each of fns, alternating inside every iteration."""
        for _ in range(args.warmup):
            for fn in fns:
                fn()
        stream.synchronize()
        ms = [0.0] * len(fns)
        for _ in range(args.iters):
            for i, fn in enumerate(fns):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                fn()
                e1.record(stream)
                e1.synchronize()
                ms[i] += e0.elapsed_time(e1) / args.iters
        return ms

    def on_device(tx, doc_off):
        d_text = torch.zeros(len(tx) + 32, dtype=torch.uint8, device=dev)
        d_text[:len(tx)].copy_(torch.from_numpy(tx))
        d_off = torch.from_numpy(doc_off).to(dev)
        torch.cuda.synchronize()
        b = enc.new_batch()
        b.encode_device(d_text.data_ptr(), d_off.data_ptr(), len(doc_off) - 1, len(tx), True, stream=sp, sync=False)
        b.result()
        return b, (d_text, d_off)

    def seen_outs(nu, nd):
        o = {k: torch.empty(nu, dtype=torch.int64, device=dev) for k in ("unit_begin", "unit_end", "unit_first", "unit_count")}
        o["unit_flags"] = torch.empty(nu, dtype=torch.uint8, device=dev)
        o["unit_off"] = torch.empty(nd + 1, dtype=torch.int64, device=dev)
        o["n_dup"] = torch.empty(nd, dtype=torch.int32, device=dev)
        o.update({k: torch.empty(nd, dtype=torch.int64, device=dev) for k in ("dup_bytes", "dup_chars", "unit_bytes", "unit_chars")})
        return o

    for kind in ("mixed", "english"):
        text, doc_off = bench.make_corpus(kind, args.docs, 3, min(16, len(os.sched_getaffinity(0))))
        text, doc_off = np.ascontiguousarray(text), np.ascontiguousarray(doc_off)
        nd = len(doc_off) - 1
        b, keep = on_device(text, doc_off)
        nu = b.line_units("line", False, 0, 0, sp)
        lo = {k: torch.empty(nu, dtype=torch.int64, device=dev) for k in ("unit_begin", "unit_end")}
        lo.update(unit_flags=torch.empty(nu, dtype=torch.uint8, device=dev), unit_off=torch.empty(nd + 1, dtype=torch.int64, device=dev),
                  n_dup=torch.empty(nd, dtype=torch.int32, device=dev))
        lo.update({k: torch.empty(nd, dtype=torch.int64, device=dev) for k in ("dup_bytes", "dup_chars", "unit_bytes", "unit_chars")})
        so = seen_outs(nu, nd)
        lptr, sptr = ({k: t.data_ptr() for k, t in o.items() if t.numel()} for o in (lo, so))
        base = [0]
        warm_set = enc.seen_set("line")
        b.seen_mark(warm_set, True, False, 0, stream=sp)

        def lines_pass():                         # (another doc_index_base every call: the list is rebuilt, never served from the batch)
            base[0] += 1
            b.line_units("line", False, 0, base[0], sp)
            b.line_repeats("line", False, False, 0, base[0], sp, **lptr)

        def seen_fresh():
            base[0] += 1
            s = enc.seen_set("line")
            b.seen_mark(s, True, True, base[0], stream=sp, **sptr)
            s.close()

        def seen_warm():
            base[0] += 1
            b.seen_mark(warm_set, True, True, base[0], stream=sp, **sptr)

        t_lines, t_fresh, t_warm = timed([lines_pass, seen_fresh, seen_warm])
        # the check: first occurrence wins, by a dict over the units' bytes
        s = enc.seen_set("line")
        b.seen_mark(s, True, True, 0, stream=sp, **sptr)
        stream.synchronize()
        ub, ue, fl = (so[k].cpu().numpy() for k in ("unit_begin", "unit_end", "unit_flags"))
        seen, want = set(), np.zeros(nu, dtype=np.uint8)
        raw = text.tobytes()
        for i in range(nu):
            u = raw[ub[i]:ue[i]]
            want[i] = u in seen
            seen.add(u)
        assert np.array_equal(fl, want) and len(s) == len(seen), kind
        say("corpus.%s: %d documents, %.1f MB, %d lines, %d distinct, %d flagged; line_units + line_repeats %.3f ms; seen_mark ADD|QUERY into a "
            "fresh set %.3f ms (%.2f x), into a set that holds the batch %.3f ms (%.2f x)  [flags checked against a dict]"
            % (kind, nd, len(text) / 1e6, nu, len(seen), int(fl.sum()), t_lines, t_fresh, t_fresh / t_lines, t_warm, t_warm / t_lines))
        s.close(), warm_set.close(), b.close()
    # one line, repeated: the add with and without the merge inside the workgroup
    tx = np.frombuffer(b"Click here to subscribe\n" * args.repeats, dtype=np.uint8).copy()
    b, keep = on_device(tx, np.array([0, len(tx)], dtype=np.int64))
    s = enc.seen_set("line")
    assert b.seen_mark(s, True, False, 0, stream=sp) == args.repeats
    t_comb, t_plain = timed([lambda: b.seen_mark(s, True, False, 0, stream=sp), lambda: b.seen_mark(s, True, False, 0, stream=sp, combine=False)])
    k, f, c = s.entries()
    assert len(k) == 1 and f[0] == 0 and c[0] == args.repeats * (1 + 2 * (args.warmup + args.iters))
    say("one line x %d in one document (the units are found once and reused, so this is the add and its two host waits): merged in LDS %.3f ms, "
        "one triple of atomics per unit %.3f ms (%.2f x)" % (args.repeats, t_comb, t_plain, t_plain / t_comb))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(out_lines) + "\n")


if __name__ == "__main__":
    main()
