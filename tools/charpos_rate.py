#!/usr/bin/env python3
"""Rate of the character-position passes (jtk_batch_char_index, jtk_batch_token_char_offsets) beside two yardsticks that are
older code, on 100k English documents and on the headline mix, resident in HBM.  Runs alternated in one process, medians of the
repeated steps, every step timed up to a device synchronise:
  copy      hipMemcpyAsync, device to device, of the text's n_bytes (moves 2 n; the build reads n and writes about 0.03 n)
  build     jtk_batch_char_index: the index over the text, rebuilt every step (for the unit that the cached index is not for)
  offsets   jtk_batch_token_offsets on the encode (byte positions, one int64 per token; the byte scan is there already)
  chars     jtk_batch_token_char_offsets on the same encode, begin and end, index already built (two int64 per token)
usage: python tools/charpos_rate.py [--steps 15] [--warmup 3] [--docs 100000] [--mixed-docs 50000]"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import jtokkit_amd
from jtokkit_amd import corpus
from jtokkit_amd.encoding import _copy_d2d

def measure(name, text, doc_off, steps, warmup):
    enc = jtokkit_amd.get_encoding("cl100k_base")
    b = enc.new_batch()
    n, nd = len(text), len(doc_off) - 1
    buf = torch.zeros((n + 15) // 16 * 16 + 16, dtype=torch.uint8, device="cuda")
    buf[:n].copy_(torch.from_numpy(np.ascontiguousarray(text)))
    d_off = torch.from_numpy(doc_off).cuda()
    dst = torch.empty_like(buf)
    torch.cuda.synchronize()
    stream = b.stream()
    nt = b.encode_device(buf.data_ptr(), d_off.data_ptr(), nd, n, ordinary=True)
    pos = torch.empty(nt, dtype=torch.int64, device="cuda")
    begin, end = torch.empty(nt, dtype=torch.int64, device="cuda"), torch.empty(nt, dtype=torch.int64, device="cuda")
    units = torch.empty(nd, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    b.token_offsets(pos.data_ptr())                                        # (the byte scan: shared by both token passes)
    b.char_index("utf16", units.data_ptr())
    torch.cuda.synchronize()
    # results first: the document lengths and the last token's end against the host's own count over the text
    cont = (text & 0xC0) == 0x80
    lead4 = text >= 0xF0
    cs = np.concatenate([[0], np.cumsum(~cont, dtype=np.int64) + np.cumsum(lead4, dtype=np.int64)])
    ok = bool(np.array_equal(units.cpu().numpy(), cs[doc_off[1:]] - cs[doc_off[:-1]]))
    b.token_char_offsets("utf16", begin.data_ptr(), end.data_ptr())
    torch.cuda.synchronize()
    p = pos.cpu().numpy()
    doc = np.searchsorted(doc_off, p, side="right") - 1
    at_char = ~cont[p]
    ok = ok and bool(np.array_equal(begin.cpu().numpy()[at_char], (cs[p] - cs[doc_off[doc]])[at_char])) and bool((end > begin).all())
    runs = {
        "copy": lambda: _copy_d2d(dst.data_ptr(), buf.data_ptr(), n, stream),
        "build": lambda: b.char_index("char"),                               # (the index at hand is the "chars" run's, for utf16)
        "offsets": lambda: b.token_offsets(pos.data_ptr()),
        "chars": None,
    }
    times = {k: [] for k in runs}
    for step in range(warmup + steps):
        for k, f in runs.items():
            if k == "chars":
                b.char_index("utf16")                                        # (outside the clock: the index for the pass)
                torch.cuda.synchronize()
                f = lambda: b.token_char_offsets("utf16", begin.data_ptr(), end.data_ptr())
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            if step >= warmup:
                times[k].append(time.perf_counter() - t0)
    ms = {k: float(np.median(v)) * 1e3 for k, v in times.items()}
    b.close()
    return {"workload": name, "docs": nd, "bytes": n, "tokens": int(nt), "results_ok": ok, "steps": steps, "warmup": warmup,
            "copy_ms": round(ms["copy"], 3), "build_ms": round(ms["build"], 3), "offsets_ms": round(ms["offsets"], 3),
            "chars_ms": round(ms["chars"], 3), "min_max_ms": {k: [round(min(v) * 1e3, 3), round(max(v) * 1e3, 3)] for k, v in times.items()},
            "build_gb_per_s": round(n / ms["build"] / 1e6, 1), "copy_gb_per_s_moved": round(2 * n / ms["copy"] / 1e6, 1),
            "build_over_copy": round(ms["build"] / ms["copy"], 3), "chars_over_offsets": round(ms["chars"] / ms["offsets"], 3),
            "chars_ns_per_token": round(ms["chars"] * 1e6 / max(nt, 1), 4)}

def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--docs", type=int, default=100000)
    ap.add_argument("--mixed-docs", type=int, default=50000)
    a = ap.parse_args()
    for name, (text, doc_off) in (("english", corpus.english(a.docs, seed=2)), ("mixed", corpus.mixed(a.mixed_docs))):
        print(json.dumps(measure(name, text, doc_off, a.steps, a.warmup)), flush=True)

if __name__ == "__main__":
    main()
