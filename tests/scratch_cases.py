"""Worst-case texts for the queue bounds of jtk_scratch_rules.h, shared by test_scratch_bounds.py (CPU) and
test_chunks_in_flight_gpu.py: text made of one hard piece (no table entry, so it is queued for bytePairMerge) back to back.

The rules come from the stand-alone program tests/scratch_bounds/scratch_bounds.cpp (built once per session into a temporary
directory); the pieces from merge_cases.Pieces, checked against the oracle's split: a piece is used only if the oracle cuts
the repeated text into exactly that piece, and only if it encodes to two or more tokens."""
import functools
import json
import os
import subprocess
import tempfile

import merge_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "cl100k_base"
GIB = 1 << 30


@functools.lru_cache(maxsize=None)
def rules(*n_bytes):
    """what the header says (for the byte counts given: tiles, shard capacities, bytes of a set)"""
    d = tempfile.mkdtemp(prefix="jtk_scratch_bounds_")
    exe = os.path.join(d, "scratch_bounds")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I" + os.path.join(rocm, "include"), "-D__HIP_PLATFORM_AMD__", "-o", exe,
                           os.path.join(ROOT, "tests", "scratch_bounds", "scratch_bounds.cpp")])
    return json.loads(subprocess.check_output([exe] + [str(n) for n in n_bytes]))


@functools.lru_cache(maxsize=None)
def pieces():
    return merge_cases.Pieces(NAME)


@functools.lru_cache(maxsize=None)
def hard_piece(length, seed=1):
    """a piece of `length` bytes that is no table entry and that the oracle cuts out of its own repetition"""
    P = pieces()
    ok = lambda p: p is not None and len(p) == length and P.count(p) >= 2 and P.o.split(p * 3) == [p] * 3
    for kind in ("words", "sym", "rare", "multi"):
        try:
            p = P.pick(kind, length, seed)
        except (KeyError, IndexError, ValueError):
            p = None
        if ok(p):
            return p
    if length <= 3:                                    # a blank and one or two bytes that are neither letters, digits nor blanks
        for c in list(range(1, 9)) + list(range(14, 32)) + [127]:
            p = b" " + bytes([c]) * (length - 1)
            if ok(p):
                return p
    raise AssertionError("no hard piece of %d bytes" % length)


def bin_lengths(r, b):
    lens = [int(k) for k, v in r["bin_of_len"].items() if v == b]
    return min(lens), max(lens)


def back_to_back(piece, n_bytes, shift=0):
    """`shift` filler bytes (newlines: pieces of their own kind, resolved), then whole pieces up to at least n_bytes"""
    n = (n_bytes - shift + len(piece) - 1) // len(piece)
    return b"\n" * shift + piece * n


def queued(r, text):
    """{(bin, tile): entries} by the oracle's split and the header's binning"""
    P = pieces()
    out, pos, hard = {}, 0, {}
    for p in P.o.split(text):
        if 2 <= len(p) <= r["maxlen"]:
            if p not in hard:
                hard[p] = P.count(p) >= 2
            if hard[p]:
                key = (r["bin_of_len"][str(len(p))], pos // r["tile"])
                out[key] = out.get(key, 0) + 1
        pos += len(p)
    assert pos == len(text)
    return out
