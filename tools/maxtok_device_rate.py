"""Encoding.encode(text, maxTokens) for a device-resident batch, three routes, on the headline corpus (200k documents of
corpus.mixed, cl100k_base):

  device_max_tokens   jtk_batch_encode_device_max_tokens (HipEncoding.encode_batch_max_tokens_device): the early exit as
                      kernels, rows [n_docs, max_tokens]
  whole_truncate      jtk_batch_encode_device of every whole document + jtk_batch_truncate (ragged result)
  host_max_tokens     jtk_batch_encode_max_tokens from host buffers (the early exit on host threads)

Device routes are timed with HIP events on their stream after warm-up, the host route by the wall clock.  The new route's
output is checked against the host route at every size.  With --trace one more call per size prints its rounds
(JTK_MAXTOK_TRACE) to stderr; run under `rocprofv3 --kernel-trace --stats` for per-kernel times.

  python tools/maxtok_device_rate.py [--docs 200000] [--limits 10,128,2048] [--iters 10] [--trace]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=200000)
    ap.add_argument("--limits", default="10,128,2048")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()
    import torch
    import bench
    import jtokkit_amd
    from jtokkit_amd import _native as N

    text, doc_off = bench.make_corpus("mixed", args.docs, 3, min(16, len(os.sched_getaffinity(0))))
    n_docs = len(doc_off) - 1
    dev = torch.device("cuda:0")
    d_text, d_off = torch.from_numpy(text).to(dev), torch.from_numpy(doc_off).to(dev)
    enc = jtokkit_amd.get_encoding("cl100k_base")
    print("corpus: %d documents, %.1f MB, device-resident" % (n_docs, len(text) / 1e6), flush=True)

    def device_ms(fn, stream):
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

    results = []
    for mx in [int(x) for x in args.limits.split(",")]:
        out = torch.empty((n_docs, mx), dtype=torch.int32, device=dev)
        for ordinary in (True, False):
            cur = torch.cuda.current_stream(dev)
            ms_new = device_ms(lambda: enc.encode_batch_max_tokens_device(d_text, d_off, mx, ordinary=ordinary, out=out), cur)
            rows, kept, tr, st = enc.encode_batch_max_tokens_device(d_text, d_off, mx, ordinary=ordinary, out=out)
            b = enc.new_batch()
            bstream = torch.cuda.ExternalStream(b.stream(), device=dev)

            def whole():
                b.encode_device(d_text.data_ptr(), d_off.data_ptr(), n_docs, len(text), ordinary=ordinary, sync=False)
                rc = N.lib().jtk_batch_truncate(b._h, mx)
                assert rc == 0
            ms_whole = device_ms(whole, bstream)
            hb = enc.new_batch()
            hb.encode_max_tokens(text, doc_off, mx, ordinary)
            t0 = time.perf_counter()
            for _ in range(max(1, args.iters // 2)):
                h_rows, h_kept, h_tr, h_st = hb.encode_max_tokens(text, doc_off, mx, ordinary)
            ms_host = (time.perf_counter() - t0) * 1e3 / max(1, args.iters // 2)
            kept_n, st_n, tr_n = kept.cpu().numpy(), st.cpu().numpy(), tr.cpu().numpy()
            ok = np.array_equal(kept_n, h_kept) and np.array_equal(st_n, h_st) and np.array_equal(tr_n.astype(np.uint8), h_tr)
            rows_n = rows.cpu().numpy()
            live = np.arange(mx)[None, :] < kept_n[:, None]
            ok = ok and np.array_equal(np.where(live, rows_n, 0), np.where(live, h_rows, 0)) and (rows_n[~live] == -1).all()
            r = {"max_tokens": mx, "ordinary": ordinary, "device_max_tokens_ms": round(ms_new, 3),
                 "whole_truncate_ms": round(ms_whole, 3), "host_max_tokens_ms": round(ms_host, 3),
                 "speedup_vs_whole": round(ms_whole / ms_new, 2), "equals_host_call": bool(ok)}
            print(json.dumps(r), flush=True)
            results.append(r)
            if args.trace:
                os.environ["JTK_MAXTOK_TRACE"] = "1"
                enc.encode_batch_max_tokens_device(d_text, d_off, mx, ordinary=ordinary, out=out)
                torch.cuda.synchronize()
                del os.environ["JTK_MAXTOK_TRACE"]
            b.close()
            hb.close()
            assert ok, "device rows differ from the host call at max_tokens=%d ordinary=%s" % (mx, ordinary)
        del out
    return results


if __name__ == "__main__":
    main()
