#!/usr/bin/env python3
"""Rate of the id-matrix decode (jtk_batch_decode_rows_device) beside the flat decode, on the workload of tools/decode_rate.py:
the ids of 100k English documents, resident in HBM.  Three runs, alternated in one process, medians of the repeated steps:
  flat    jtk_batch_decode_device on the ids and their offsets (unchanged code: the yardstick)
  dense   the same ids as an int32 [n / 2048, 2048] matrix without options (reads and writes what the flat decode does)
  padded  the ids as int64 [n_docs, max_len] rows right-filled with an EOS id; one stop id and the pad skipped
usage: python tools/decode_rows_rate.py [--steps 15] [--warmup 3]"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import jtokkit_amd
from jtokkit_amd import corpus

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
    d_off = torch.from_numpy(tok_off).cuda()
    n_dense = nt // 2048
    lens = torch.from_numpy(np.diff(tok_off)).cuda()
    max_len = int(lens.max())
    padded = torch.full((nd, max_len), eos, dtype=torch.int64, device="cuda")
    padded[torch.arange(max_len, device="cuda")[None, :] < lens[:, None]] = d_ids.to(torch.int64)
    torch.cuda.synchronize()
    runs = {
        "flat": lambda: b.decode_device(d_ids.data_ptr(), d_off.data_ptr(), nd, nt),
        "dense": lambda: b.decode_rows_device(d_ids.data_ptr(), 4, n_dense, 2048),
        "padded": lambda: b.decode_rows_device(padded.data_ptr(), 8, nd, max_len, pad_id=eos, stop_ids=[eos], skip_pad=True),
    }
    # results first: the dense matrix gives the text of its ids, the padded rows give every document
    nb_flat = runs["flat"]()
    flat_out = b.decode_fetch()[0].copy()
    ok = bool(np.array_equal(flat_out, text))
    nb_dense = runs["dense"]()
    ok = ok and bool(np.array_equal(b.decode_fetch()[0], flat_out[:nb_dense]))
    nb_padded = runs["padded"]()
    out, byte_off, status = b.decode_fetch()
    ok = ok and bool(np.array_equal(out, text) and np.array_equal(byte_off, doc_off) and (status == 0).all())
    times = {k: [] for k in runs}
    for step in range(a.warmup + a.steps):
        for k, f in runs.items():                                           # (every call ends in a stream synchronise)
            t0 = time.perf_counter()
            f()
            if step >= a.warmup:
                times[k].append(time.perf_counter() - t0)
    ms = {k: float(np.median(v)) * 1e3 for k, v in times.items()}
    spread = {k: [round(min(v) * 1e3, 3), round(max(v) * 1e3, 3)] for k, v in times.items()}
    cells = nd * max_len
    print(json.dumps({
        "tokens": nt, "docs": nd, "bytes": int(nb_flat), "results_ok": ok, "steps": a.steps, "warmup": a.warmup,
        "flat_ms": round(ms["flat"], 3), "dense_ms": round(ms["dense"], 3), "padded_ms": round(ms["padded"], 3), "min_max_ms": spread,
        "dense_cells": n_dense * 2048, "dense_over_flat": round(ms["dense"] / ms["flat"] * nt / (n_dense * 2048), 3),
        "padded_shape": [nd, max_len], "padded_cells": cells, "pad_share": round(1 - nt / cells, 4),
        "padded_ns_per_cell": round(ms["padded"] * 1e6 / cells, 4), "padded_ns_per_output_byte": round(ms["padded"] * 1e6 / nb_padded, 4),
        "padded_over_flat": round(ms["padded"] / ms["flat"], 3)}))

if __name__ == "__main__":
    main()
