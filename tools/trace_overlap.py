#!/usr/bin/env python3
"""How much of each kernel's span other kernels ran beside it, from a rocprofv3 --kernel-trace CSV:

    python tools/trace_overlap.py <dir>/kt_kernel_trace.csv [kernel-name substring, default k_bpe_merge]

Per kernel name: launches, mean duration, and the mean share of a launch's span during which at least one kernel of another
queue (another chunk's stream) was running.  Then for the named kernel the same share split by which kernel ran beside it,
and the whole trace's busy time (union of all spans) against the sum of the spans."""
import csv
import sys
from collections import defaultdict


def short(name):
    for k in ("k_piece_resolve", "k_pretok_split", "k_bpe_merge", "k_pack_tokens", "k_tile_scan", "k_doc_offsets", "k_mark_docs"):
        if k in name:
            return k
    return name.split("(")[0][-40:]


def union_len(spans):
    total, end = 0, None
    for a, b in sorted(spans):
        if end is None or a > end:
            total += b - a
            end = b
        elif b > end:
            total += b - end
            end = b
    return total


def clipped(spans, a, b):
    return [(max(a, x), min(b, y)) for x, y in spans if y > a and x < b]


def main():
    path = sys.argv[1]
    focus = sys.argv[2] if len(sys.argv) > 2 else "k_bpe_merge"
    rows = []
    for r in csv.DictReader(open(path)):
        rows.append((short(r["Kernel_Name"]), int(r["Queue_Id"]), int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    by_name = defaultdict(list)
    for i, r in enumerate(rows):
        by_name[r[0]].append(i)
    print("%-28s %8s %12s %22s" % ("kernel", "launches", "mean ms", "span shared with others"))
    for name, idx in sorted(by_name.items(), key=lambda kv: -sum(rows[i][3] - rows[i][2] for i in kv[1])):
        dur = shared = 0
        for i in idx:
            _, q, a, b = rows[i]
            others = clipped([(x, y) for (_, q2, x, y) in rows if q2 != q], a, b)
            dur += b - a
            shared += union_len(others)
        print("%-28s %8d %12.4f %21.1f%%" % (name, len(idx), dur / len(idx) / 1e6, 100.0 * shared / max(1, dur)))
    print()
    print("beside %s, by kernel (share of its span; they may overlap each other):" % focus)
    tot = sum(rows[i][3] - rows[i][2] for i in by_name.get(focus, []))
    for name in by_name:
        s = 0
        for i in by_name.get(focus, []):
            _, q, a, b = rows[i]
            s += union_len(clipped([(x, y) for (n2, q2, x, y) in rows if q2 != q and n2 == name], a, b))
        if s:
            print("  %-26s %6.1f%%" % (name, 100.0 * s / max(1, tot)))
    spans = [(a, b) for (_, _, a, b) in rows]
    print()
    print("sum of spans %.3f ms, busy (union) %.3f ms, first start to last end %.3f ms" % (
        sum(b - a for a, b in spans) / 1e6, union_len(spans) / 1e6, (max(b for _, b in spans) - min(a for a, _ in spans)) / 1e6))


if __name__ == "__main__":
    main()
