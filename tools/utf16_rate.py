#!/usr/bin/env python3
"""Rate of the UTF-16 passes (jtk_batch_transcode_utf16_device, jtk_batch_encode_utf16_device, jtk_batch_decode_utf16) beside
yardsticks that are older code, on 100k English documents and on the headline mix, resident in HBM.  Runs alternated in one
process, medians of the repeated steps, every step timed up to a device synchronise:
  transcode      E: units -> UTF-8 text and doc_off (reads 2 bytes per unit twice -- count and write --, writes the text)
  copy           hipMemcpyAsync, device to device, of (input + output) / 2 bytes of E: it moves what E reads once plus writes
  encode_utf16   jtk_batch_encode_utf16_device: the transcode and the encode of the owned text
  encode         jtk_batch_encode_device on the already transcoded text: what there was once a host had transcoded
  decode_utf16   D over the decode of the batch's tokens: bytes -> units and unit_off
  decode_copy    the copy of (input + output) / 2 bytes of D
  cpu_*          the CPython codecs on one core for the same text, for scale
The results are checked first: the corpora are well-formed, so E of their UTF-16 form must give back their bytes and offsets, D
of the decoded tokens their units; the first documents also go through the plain reference tests/utf16_ref.py.
usage: python tools/utf16_rate.py [--steps 15] [--warmup 3] [--docs 100000] [--mixed-docs 50000]"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import jtokkit_amd
from jtokkit_amd import corpus
from jtokkit_amd.encoding import _copy_d2d
import utf16_ref

def measure(name, text, doc_off, steps, warmup):
    enc = jtokkit_amd.get_encoding("cl100k_base")
    b = enc.new_batch()
    n, nd = len(text), len(doc_off) - 1
    raw = text.tobytes()
    t0 = time.perf_counter()
    as_str = raw.decode("utf-8")
    as_u16 = as_str.encode("utf-16-le")
    cpu_d = time.perf_counter() - t0
    t0 = time.perf_counter()
    back = as_u16.decode("utf-16-le").encode("utf-8")
    cpu_e = time.perf_counter() - t0
    assert back == raw
    units = np.frombuffer(as_u16, dtype=np.uint16)
    cont, lead4 = (text & 0xC0) == 0x80, text >= 0xF0
    cs = np.concatenate([[0], np.cumsum(~cont, dtype=np.int64) + np.cumsum(lead4, dtype=np.int64)])
    unit_off = cs[doc_off]
    nu = len(units)
    assert unit_off[-1] == nu
    d_units, d_uoff = torch.from_numpy(units.copy()).cuda(), torch.from_numpy(unit_off).cuda()
    torch.cuda.synchronize()
    stream = b.stream()
    # results first
    ok = b.transcode_utf16_device(d_units.data_ptr(), d_uoff.data_ptr(), nd, nu) == n
    utf8, d_off = enc.transcode_utf16_device(d_units, d_uoff)
    torch.cuda.synchronize()
    ok = ok and bool(np.array_equal(utf8.cpu().numpy(), text)) and bool(np.array_equal(d_off.cpu().numpy(), doc_off))
    k = min(nd, 200)
    ref_text, ref_off = utf16_ref.encode(units[:unit_off[k]], unit_off[:k + 1])
    ok = ok and bool(np.array_equal(ref_text, text[:doc_off[k]])) and bool(np.array_equal(ref_off, doc_off[:k + 1]))
    buf = torch.zeros((n + 15) // 16 * 16 + 16, dtype=torch.uint8, device="cuda")
    buf[:n].copy_(utf8)
    d_doff = torch.from_numpy(doc_off).cuda()
    torch.cuda.synchronize()
    nt = b.encode_device(buf.data_ptr(), d_doff.data_ptr(), nd, n, ordinary=True)
    ok = ok and b.encode_utf16_device(d_units.data_ptr(), d_uoff.data_ptr(), nd, nu, ordinary=True) == nt
    p_tok, p_toff, _ = b.device_result()
    ok = ok and b.decode_device(p_tok, p_toff, nd, nt) == n
    ok = ok and b.decode_utf16() == nu
    got_units, got_off, _ = b.decode_utf16_fetch()
    ok = ok and bool(np.array_equal(got_units, units)) and bool(np.array_equal(got_off, unit_off))
    ref_units, ref_uoff = utf16_ref.decode(text[:doc_off[k]], doc_off[:k + 1])
    ok = ok and bool(np.array_equal(ref_units, units[:unit_off[k]])) and bool(np.array_equal(ref_uoff, unit_off[:k + 1]))
    moved = 2 * nu + n                                                      # input + output bytes, the same for E and D
    src, dst = torch.empty(moved // 2, dtype=torch.uint8, device="cuda"), torch.empty(moved // 2, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    runs = {
        "copy": lambda: _copy_d2d(dst.data_ptr(), src.data_ptr(), moved // 2, stream),
        "transcode": lambda: b.transcode_utf16_device(d_units.data_ptr(), d_uoff.data_ptr(), nd, nu),
        "encode": lambda: b.encode_device(buf.data_ptr(), d_doff.data_ptr(), nd, n, ordinary=True),
        "encode_utf16": lambda: b.encode_utf16_device(d_units.data_ptr(), d_uoff.data_ptr(), nd, nu, ordinary=True),
        "decode_utf16": lambda: b.decode_utf16(),
    }
    times = {k_: [] for k_ in runs}
    for step in range(warmup + steps):
        for k_, f in runs.items():
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            if step >= warmup:
                times[k_].append(time.perf_counter() - t0)
    ms = {k_: float(np.median(v)) * 1e3 for k_, v in times.items()}
    b.close()
    return {"workload": name, "docs": nd, "bytes": n, "units": nu, "tokens": int(nt), "results_ok": ok, "steps": steps, "warmup": warmup,
            "transcode_ms": round(ms["transcode"], 3), "copy_ms": round(ms["copy"], 3),
            "transcode_over_copy": round(ms["transcode"] / ms["copy"], 3),
            "encode_utf16_ms": round(ms["encode_utf16"], 3), "encode_ms": round(ms["encode"], 3),
            "encode_utf16_over_encode": round(ms["encode_utf16"] / ms["encode"], 3),
            "decode_utf16_ms": round(ms["decode_utf16"], 3), "decode_copy_ms": round(ms["copy"], 3),
            "decode_utf16_over_copy": round(ms["decode_utf16"] / ms["copy"], 3),
            "transcode_gb_per_s_moved": round(moved / ms["transcode"] / 1e6, 1), "copy_gb_per_s_moved": round(moved / ms["copy"] / 1e6, 1),
            "cpu_encode_utf8_ms": round(cpu_e * 1e3, 1), "cpu_decode_utf8_ms": round(cpu_d * 1e3, 1),
            "min_max_ms": {k_: [round(min(v) * 1e3, 3), round(max(v) * 1e3, 3)] for k_, v in times.items()}}

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
