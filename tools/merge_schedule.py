"""Schedule model of the lean merge bins (k_bpe_merge), on the CPU: how many wave-steps the queues of a text cost
when a wave takes 64 consecutive entries, and when it takes a window of W consecutive entries in stable order of length
(jtokkit_amd/csrc/jtk_merge_order_rules.h), 64 per round.

The model.  Pieces are the oracle's split, cut further wherever two neighbouring bytes occur together in no table entry (the
split kernel makes those cuts in blocks with non-ASCII bytes or few pieces; the model makes them everywhere, exact either way).
A piece that is no table entry is queued by (bin of its length, tile % 64) in tile order; it takes length - tokens merge steps.
A wave steps until its slowest piece is done: 64 entries cost max(steps) wave-steps; sum(steps) / 64 is what they would cost if
no lane ever idled -- the bound a refill of finished lanes would be measured against.

    python tools/merge_schedule.py [--docs 1000] [--seed 3] [--encoding cl100k_base]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, Q_SHARDS = 2048, 64
BINS = ((4, 8), (9, 12), (13, 16), (17, 32), (33, 64))      # lean bins 0..4, piece bytes
WINDOWS = (128, 256, 512, 1024)


def queues(name, text, doc_off):
    """{(bin, shard): (lengths, steps)} in queue order (tiles of a shard in text order, pieces of a tile in text order)"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import merge_ref
    import oracle_lib
    o = oracle_lib.get(name)
    ranks = merge_ref.load_ranks(name)
    pair_ok = np.zeros(65536, dtype=bool)
    for k in ranks:
        a = np.frombuffer(k, dtype=np.uint8).astype(np.int64)
        pair_ok[(a[:-1] << 8) | a[1:]] = True
    raw = text.tobytes()
    steps_of = {}
    q = {}
    for d in range(len(doc_off) - 1):
        pos = int(doc_off[d])
        for p in o.split(raw[pos:int(doc_off[d + 1])]):
            start = pos
            pos += len(p)
            if len(p) < 4 or p in ranks:
                continue
            a = np.frombuffer(p, dtype=np.uint8).astype(np.int64)
            cuts = [0] + (np.nonzero(~pair_ok[(a[:-1] << 8) | a[1:]])[0] + 1).tolist() + [len(p)]
            for i in range(len(cuts) - 1):
                s = p[cuts[i]:cuts[i + 1]] if len(cuts) > 2 else p
                if len(s) < 4 or len(s) > 64 or s in ranks:
                    continue
                if s not in steps_of:
                    steps_of[s] = len(s) - len(o.merge_piece(s))
                b = next(k for k, (lo, hi) in enumerate(BINS) if lo <= len(s) <= hi)
                q.setdefault((b, (start + cuts[i]) // T % Q_SHARDS), []).append((len(s), steps_of[s]))
    return {k: (np.array([x[0] for x in v]), np.array([x[1] for x in v])) for k, v in q.items()}


def wave_steps(steps):
    """64 consecutive entries per wave"""
    n = len(steps)
    pad = np.zeros((n + 63) // 64 * 64, dtype=np.int64)
    pad[:n] = steps
    return int(pad.reshape(-1, 64).max(axis=1).sum())


def wave_steps_ordered(lengths, steps, window):
    total = 0
    for at in range(0, len(steps), window):
        order = np.argsort(lengths[at:at + window], kind="stable")
        total += wave_steps(steps[at:at + window][order])
    return total


def table(q):
    """per bin: entries, mean steps, wave-steps today, if no lane idled, and ordered per window size"""
    rows = []
    for b in range(len(BINS)):
        mine = [v for (bb, _), v in sorted(q.items()) if bb == b]
        n = sum(len(s) for _, s in mine)
        if not n:
            continue
        row = {"bin": b, "entries": n, "mean_steps": sum(int(s.sum()) for _, s in mine) / n,
               "today": sum(wave_steps(s) for _, s in mine), "no_idle": sum(int(s.sum()) for _, s in mine) / 64.0}
        for w in WINDOWS:
            row[w] = sum(wave_steps_ordered(l, s, w) for l, s in mine)
        rows.append(row)
    return rows


def render(rows):
    out = ["bin  bytes    entries  mean steps  wave-steps today  no lane idle  busy  " + "  ".join("W=%-4d" % w for w in WINDOWS)]
    for r in rows:
        out.append("%-3d  %2d..%-2d  %8d  %10.2f  %16d  %12.0f  %4.2f  " % (
            r["bin"], BINS[r["bin"]][0], BINS[r["bin"]][1], r["entries"], r["mean_steps"], r["today"], r["no_idle"],
            r["no_idle"] / r["today"]) + "  ".join("x%5.3f" % (r[w] / r["today"]) for w in WINDOWS))
    return "\n".join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1000)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--encoding", default="cl100k_base")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    from jtokkit_amd import corpus
    text, doc_off = corpus.mixed(args.docs, seed=args.seed)
    print("corpus.mixed(%d, seed=%d): %.1f MB" % (args.docs, args.seed, len(text) / 1e6))
    print(render(table(queues(args.encoding, text, doc_off))))


if __name__ == "__main__":
    main()
