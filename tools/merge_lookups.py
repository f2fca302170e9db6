"""Which pair lookups of the lean merge bins (lean_steps in k_bpe_merge) any lane wants, counted on the CPU: an
extension of the schedule model of tools/merge_schedule.py -- same pieces, same cuts, same queue order -- that replays every
piece's merge with want1 / want2 formed as lean_steps forms them (tests/merge_exit_cases.py: replay) and steps the lanes of a
wave together.

Waves.  The 4..8-byte bin is taken in windows of --window (256) consecutive entries in stable order of length, 64 per round,
whatever the queue's length (the kernel does so once a shard's queue gives each of its waves a full window);
the other bins 64 consecutive entries per wave.  A wave-step is one trip of the step loop with a lane still merging; it issues
two gather instructions, one per side.

Columns
    wave-steps          trips with a lane still merging (and per wave)
    no lane wants       trips in which no lane wants either lookup -- what the early exit of lean_steps spares -- and the share
                        of the waves that have one; `last` says how many of them were their wave's last trip (all, by the lane
                        rule: a lane that merges and wants nothing is done after this step)
    gathers unwanted    of the 2 x wave-steps gather instructions, those whose side no lane wants
    one side            trips in which exactly one side is wanted by some lane               (counted, not built)
    never both          trips in which some lane wants a lookup but no lane wants both sides (counted, not built)

    python tools/merge_lookups.py [--docs 1000] [--seed 3] [--encoding cl100k_base] [--window 256]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import merge_schedule as ms                                                    # noqa: E402


def queues(name, text, doc_off):
    """{(bin, shard): [(length, want profile)]} in queue order, the pieces and cuts of merge_schedule.queues"""
    import merge_exit_cases as mx
    import merge_ref
    import oracle_lib
    o = oracle_lib.get(name)
    ranks = merge_ref.load_ranks(name)
    pair_ok = np.zeros(65536, dtype=bool)
    for k in ranks:
        a = np.frombuffer(k, dtype=np.uint8).astype(np.int64)
        pair_ok[(a[:-1] << 8) | a[1:]] = True
    raw = text.tobytes()
    prof_of, q = {}, {}
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
                if s not in prof_of:
                    prof_of[s] = mx.replay(s, ranks, len(s) <= 16)[0]         # SKIP_WHOLE in the bins of up to 16 bytes
                b = next(k for k, (lo, hi) in enumerate(ms.BINS) if lo <= len(s) <= hi)
                q.setdefault((b, (start + cuts[i]) // ms.T % ms.Q_SHARDS), []).append((len(s), prof_of[s]))
    return q


def waves_of(entries, window):
    """lists of up to 64 want profiles: consecutive entries, or per window in stable order of length"""
    if not window:
        return [[e[1] for e in entries[at:at + 64]] for at in range(0, len(entries), 64)]
    out = []
    for at in range(0, len(entries), window):
        w = sorted(entries[at:at + window], key=lambda e: e[0])                 # (stable)
        out += [[e[1] for e in w[r:r + 64]] for r in range(0, len(w), 64)]
    return out


def count(waves):
    c = dict(waves=len(waves), steps=0, none=0, none_last=0, waves_none=0, unwanted=0, one_side=0, never_both=0)
    for lanes in waves:
        n = max(len(st) for st in lanes)
        c["steps"] += n
        had = False
        for k in range(n):
            live = [st[k] for st in lanes if len(st) > k]
            any1, any2 = any(w1 for w1, _ in live), any(w2 for _, w2 in live)
            both = any(w1 and w2 for w1, w2 in live)
            c["unwanted"] += (not any1) + (not any2)
            if not any1 and not any2:
                c["none"] += 1
                c["none_last"] += k == n - 1
                had = True
            elif any1 != any2:
                c["one_side"] += 1
            if (any1 or any2) and not both:
                c["never_both"] += 1
        c["waves_none"] += had
    return c


def table(q, window):
    rows = []
    for b in range(len(ms.BINS)):
        mine = [v for (bb, _), v in sorted(q.items()) if bb == b]
        if not mine:
            continue
        waves = [w for v in mine for w in waves_of(v, window if b == 0 else 0)]
        row = count(waves)
        row.update(bin=b, entries=sum(len(v) for v in mine))
        rows.append(row)
    return rows


def render(rows):
    pct = lambda a, b: 100.0 * a / b if b else 0.0
    out = ["bin  bytes    entries  waves  wave-steps (per wave)  no lane wants (last)  in waves  gathers unwanted  one side  never both"]
    tot = dict(steps=0, none=0, unwanted=0)
    for r in rows:
        lo, hi = ms.BINS[r["bin"]]
        out.append("%-3d  %2d..%-2d  %8d  %5d  %10d (%5.2f)  %6d = %4.1f %% (%d)  %5.1f %%  %8d = %4.1f %%  %5.1f %%  %7.1f %%" % (
            r["bin"], lo, hi, r["entries"], r["waves"], r["steps"], r["steps"] / r["waves"], r["none"], pct(r["none"], r["steps"]),
            r["none_last"], pct(r["waves_none"], r["waves"]), r["unwanted"], pct(r["unwanted"], 2 * r["steps"]),
            pct(r["one_side"], r["steps"]), pct(r["never_both"], r["steps"])))
        for k in tot:
            tot[k] += r[k]
    out.append("all lean bins: %d wave-steps; in %d of them no lane wants a lookup: the exit spares %.1f %% of the wave-steps' %d gather "
               "instructions.\n               In all %.1f %% of them are wanted by no lane (the rest: the idle side of a step that stays)." % (
                   tot["steps"], tot["none"], pct(tot["none"], tot["steps"]), 2 * tot["steps"], pct(tot["unwanted"], 2 * tot["steps"])))
    return "\n".join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1000)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--encoding", default="cl100k_base")
    ap.add_argument("--window", type=int, default=256, help="entries per ordered window of the 4..8-byte bin (0: none)")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    from jtokkit_amd import corpus
    text, doc_off = corpus.mixed(args.docs, seed=args.seed)
    print("corpus.mixed(%d, seed=%d): %.1f MB, %s, windows of %d" % (args.docs, args.seed, len(text) / 1e6, args.encoding, args.window))
    print(render(table(queues(args.encoding, text, doc_off), args.window)))


if __name__ == "__main__":
    main()
