#!/usr/bin/env python3
"""Cost of the stop-string search (jtk_batch_decode_find_stops) beside the rows decode it follows, on the workload of
tools/decode_rows_rate.py: the ids of 100k English documents, resident in HBM, as the dense int32 [n / 2048, 2048] matrix and as
int64 [n_docs, max_len] rows right-filled with an EOS id (one stop id, the pad skipped).  For each matrix four runs, alternated
in one process, medians of the repeated steps:
  plain    the rows decode alone, as tools/decode_rows_rate.py runs it (unchanged code: the yardstick)
  decode   the same decode writing cell_byte too, which stop_col needs (unchanged code)
  never    decode + find_stops with 4 strings that never occur (their first bytes do: the compare loop runs)
  often    decode + find_stops with 4 strings of which "\\n\\n" occurs often
and the search alone over the decode that is there (never / often), which is the cost of the post-pass without the noise of the
difference.  Every run ends in a device synchronise.
usage: python tools/stop_strings_rate.py [--steps 15] [--warmup 3]"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import jtokkit_amd
from jtokkit_amd import corpus

NEVER = ["\n\n\x00", "User:\x01", " the\x02", "</s>"]
OFTEN = ["\n\n", "User:", "<|im_end|>", "###"]

def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--docs", type=int, default=100000)
    a = ap.parse_args()
    text, doc_off = corpus.english(a.docs, seed=2)
    enc = jtokkit_amd.get_encoding("cl100k_base")
    b = enc.new_batch()
    b.encode_host(text, doc_off, ordinary=True)
    res = b.fetch()
    ids, tok_off = res.tokens, res.tok_off
    nt, nd = len(ids), len(doc_off) - 1
    eos = enc.special_ids(["<|endoftext|>"])[0]
    d_ids = torch.from_numpy(ids).cuda()
    n_dense = nt // 2048
    lens = torch.from_numpy(np.diff(tok_off)).cuda()
    max_len = int(lens.max())
    padded = torch.full((nd, max_len), eos, dtype=torch.int64, device="cuda")
    padded[torch.arange(max_len, device="cuda")[None, :] < lens[:, None]] = d_ids.to(torch.int64)
    cells = {"dense": torch.empty((n_dense, 2048), dtype=torch.int64, device="cuda"),
             "padded": torch.empty((nd, max_len), dtype=torch.int64, device="cuda")}
    torch.cuda.synchronize()
    decode = {
        "dense": lambda: b.decode_rows_device(d_ids.data_ptr(), 4, n_dense, 2048, d_cell_byte_ptr=cells["dense"].data_ptr()),
        "padded": lambda: b.decode_rows_device(padded.data_ptr(), 8, nd, max_len, pad_id=eos, stop_ids=[eos], skip_pad=True,
                                               d_cell_byte_ptr=cells["padded"].data_ptr()),
    }
    plain = {
        "dense": lambda: b.decode_rows_device(d_ids.data_ptr(), 4, n_dense, 2048),
        "padded": lambda: b.decode_rows_device(padded.data_ptr(), 8, nd, max_len, pad_id=eos, stop_ids=[eos], skip_pad=True),
    }
    width = {"dense": 2048, "padded": max_len}

    def find(m, strings):
        b.decode_find_stops(strings, None, cells[m].data_ptr(), width[m])
        torch.cuda.synchronize()

    # results first: every stop of the padded rows against bytes.find on the documents
    raw = text.tobytes()
    nb = {m: decode[m]() for m in decode}
    find("padded", OFTEN)
    pos, which, hold, col = b.decode_stops_fetch()
    ok, hits = True, 0
    bo = [s.encode() for s in OFTEN]
    for q in range(0, nd, max(1, nd // 5000)):
        doc = raw[doc_off[q]:doc_off[q + 1]]
        found = min([(p, i) for i, s in enumerate(bo) for p in [doc.find(s)] if p >= 0], default=None)
        hits += found is not None
        exp = (doc_off[q] + found[0], found[1]) if found else (doc_off[q + 1], -1)
        ok = ok and (int(pos[q]), int(which[q])) == (int(exp[0]), exp[1]) and (col[q] >= 0) == (found is not None)
    share_often = float((which >= 0).mean())
    find("padded", NEVER)
    ok = ok and bool((b.decode_stops_fetch()[1] == -1).all())

    runs = {}
    for m in decode:
        runs[m + "_plain"] = plain[m]
        runs[m + "_decode"] = decode[m]
        runs[m + "_never"] = lambda m=m: (decode[m](), find(m, NEVER))
        runs[m + "_often"] = lambda m=m: (decode[m](), find(m, OFTEN))
        runs[m + "_find_never_alone"] = lambda m=m: find(m, NEVER)
        runs[m + "_find_often_alone"] = lambda m=m: find(m, OFTEN)
    times = {k: [] for k in runs}
    for step in range(a.warmup + a.steps):
        for k, f in runs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            if step >= a.warmup:
                times[k].append(time.perf_counter() - t0)
    ms = {k: float(np.median(v)) * 1e3 for k, v in times.items()}
    out = {"tokens": nt, "docs": nd, "results_ok": bool(ok), "sampled_docs_with_a_stop": hits, "rows_with_a_stop_often": round(share_often, 4),
           "steps": a.steps, "warmup": a.warmup, "ms": {k: round(v, 3) for k, v in ms.items()},
           "min_max_ms": {k: [round(min(v) * 1e3, 3), round(max(v) * 1e3, 3)] for k, v in times.items()}}
    for m in decode:
        n_cells = (n_dense * 2048) if m == "dense" else nd * max_len
        out[m] = {"shape": [n_dense, 2048] if m == "dense" else [nd, max_len], "cells": n_cells, "out_bytes": int(nb[m])}
        for kind in ("never", "often"):
            alone = ms["%s_find_%s_alone" % (m, kind)]
            out[m][kind] = {"post_pass_ms_by_difference": round(ms["%s_%s" % (m, kind)] - ms[m + "_decode"], 3),
                            "post_pass_ms_alone": round(alone, 3), "post_pass_GB_per_s_over_out": round(nb[m] / alone / 1e6, 1),
                            "post_pass_over_plain_decode": round(alone / ms[m + "_plain"], 4),
                            "post_pass_over_decode_with_cell_byte": round(alone / ms[m + "_decode"], 4)}
    print(json.dumps(out))

if __name__ == "__main__":
    main()
