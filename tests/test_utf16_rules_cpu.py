"""CPU tier of UTF-16 in and out: the rule header jtokkit_amd/csrc/jtk_utf16_rules.h -- run serially through the shim
tests/utf16_sim the way the kernels partition the work -- against the plain restatement tests/utf16_ref.py, and that restatement
against the CPython codecs, which stand for String.getBytes(UTF_8) and new String(bytes, UTF_8) here:
  E   units.decode("utf-16-le", "surrogatepass").encode("utf-8", "replace")   (an unpaired surrogate becomes '?')
  D   bytes.decode("utf-8", "replace").encode("utf-16-le")                    (one U+FFFD per maximal ill-formed subpart)
Every output byte and unit and every offset is compared, on every case of tests/utf16_cases.py, on seeded fuzz and exhaustively
over short strings of representative values; the case set must reach its edges, so that the GPU tier cannot pass by missing
one; and a stand-alone sanitizer build of the shim runs every case in buffers of exactly the documented readable size.  No GPU."""
import ctypes as C
import itertools
import os
import random
import struct
import subprocess

import numpy as np
import pytest

import charpos_ref as cr
import utf16_cases as uc
import utf16_ref as ur

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIM_DIR = os.path.join(ROOT, "tests", "utf16_sim")
E_CASES, D_CASES = uc.e_cases(), uc.d_cases()


def codec_encode_doc(units):
    return np.array(units, dtype=np.uint16).tobytes().decode("utf-16-le", "surrogatepass").encode("utf-8", "replace")


def codec_decode_seq(seq):
    return np.frombuffer(bytes(seq).decode("utf-8", "replace").encode("utf-16-le"), dtype=np.uint16).tolist()


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("utf16_sim") / "libutf16_sim.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas", "-o", out,
                           os.path.join(SIM_DIR, "utf16_sim.cpp")])
    L = C.CDLL(out)
    L.sim_u16_encode.restype = C.c_int64
    L.sim_u16_encode.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_void_p, C.c_int64, C.c_void_p]
    L.sim_u16_decode.restype = C.c_int64
    L.sim_u16_decode.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p]
    L.sim_u16_e_unit.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]
    L.sim_u16_d_byte.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]
    return L


def _padded(a, fill):
    """A 16-byte aligned copy of `a`, filled with `fill` up to the next multiple of 16 bytes."""
    n = (a.nbytes + 15) // 16 * 16 + 16
    raw = np.full(n + 16, fill, dtype=np.uint8)
    start = (-raw.ctypes.data) % 16
    view = raw[start:start + n]
    view[:a.nbytes] = a.view(np.uint8)
    return raw, view


def sim_encode(sim, units, unit_off, aligned=True):
    keep, view = _padded(units, 0xDC)                                        # (units past the end: low surrogates)
    ptr = view.ctypes.data
    if not aligned:
        keep = np.concatenate([np.zeros(1, np.uint16), units])
        ptr = keep.ctypes.data + 2
    nd = len(unit_off) - 1
    total = sim.sim_u16_encode(ptr, unit_off.ctypes.data, nd, len(units), int(aligned), None, 0, None)
    if total < 0:
        return None, None
    out = np.full(total + 1, 0xEE, dtype=np.uint8)
    doc_off = np.full(nd + 1, -7, dtype=np.int64)
    assert sim.sim_u16_encode(ptr, unit_off.ctypes.data, nd, len(units), int(aligned), out.ctypes.data, total, doc_off.ctypes.data) == total
    assert out[-1] == 0xEE
    return out[:-1], doc_off


def sim_decode(sim, text, byte_off):
    keep, view = _padded(text, 0xBF)                                         # (bytes past the end: continuation bytes)
    ns = len(byte_off) - 1
    total = sim.sim_u16_decode(view.ctypes.data, byte_off.ctypes.data, ns, len(text), None, 0, None)
    out = np.full(total + 1, 0xEEEE, dtype=np.uint16)
    unit_off = np.full(ns + 1, -7, dtype=np.int64)
    assert sim.sim_u16_decode(view.ctypes.data, byte_off.ctypes.data, ns, len(text), out.ctypes.data, total, unit_off.ctypes.data) == total
    assert out[-1] == 0xEEEE
    return out[:-1], unit_off


# ---- (a) the restatement against the codecs
def _surrogate_dense(rng):
    pool = [0xD800, 0xDBFF, 0xDC00, 0xDFFF, 0xD83D, 0xDE00, 0x41, 0x7F, 0x80, 0x7FF, 0x800, 0xD7FF, 0xE000, 0xFFFF, 0, 0xFEFF, 0x20AC]
    return [rng.choice(pool) if rng.random() < 0.9 else rng.randrange(0x10000) for _ in range(rng.randrange(0, 12))]


def _malformed_dense(rng):
    pool = [0x41, 0x7F, 0x80, 0x8F, 0x90, 0x9F, 0xA0, 0xBF, 0xC0, 0xC1, 0xC2, 0xDF, 0xE0, 0xE1, 0xEC, 0xED, 0xEE, 0xEF, 0xF0, 0xF1, 0xF3, 0xF4,
            0xF5, 0xFF]
    return bytes(rng.choice(pool) if rng.random() < 0.9 else rng.randrange(256) for _ in range(rng.randrange(0, 12)))


def test_reference_equals_the_codecs_on_cases_and_fuzz():
    for name, docs in E_CASES:
        for d in docs:
            assert ur.encode_doc(d) == codec_encode_doc(d), name
    for name, seqs in D_CASES:
        for s in seqs:
            assert ur.decode_seq(s) == codec_decode_seq(s), (name, s)
    rng = random.Random(7)
    for _ in range(4000):
        d = _surrogate_dense(rng)
        assert ur.encode_doc(d) == codec_encode_doc(d), d
        s = _malformed_dense(rng)
        assert ur.decode_seq(s) == codec_decode_seq(s), s


# ---- (b) exhaustive over short strings of representative values: reference, codec and the header's per-position functions
D_VALUES = [0x00, 0x41, 0x7F, 0x80, 0x8F, 0x90, 0x9F, 0xA0, 0xBF, 0xC0, 0xC1, 0xC2, 0xDF, 0xE0, 0xE1, 0xED, 0xEE, 0xF0, 0xF1, 0xF4, 0xF5, 0xFF]
E_VALUES = [0x0000, 0x007F, 0x0080, 0x07FF, 0x0800, 0xD7FF, 0xD800, 0xDBFF, 0xDC00, 0xDFFF, 0xE000, 0xFFFF]


def test_exhaustive_decode_of_all_4_byte_strings(sim):
    out2 = np.zeros(2, dtype=np.uint16)
    n = 0
    for tup in itertools.product(D_VALUES, repeat=4):
        s = bytes(tup)
        exp = codec_decode_seq(s)
        assert ur.decode_seq(s) == exp, s
        buf = np.frombuffer(s, dtype=np.uint8)
        got = []
        for i in range(4):
            m = sim.sim_u16_d_byte(buf.ctypes.data, 4, i, out2.ctypes.data)
            got += out2[:m].tolist()
        assert got == exp, s
        n += 1
    assert n == len(D_VALUES) ** 4


def test_exhaustive_encode_of_all_3_unit_strings(sim):
    out4 = np.zeros(4, dtype=np.uint8)
    for tup in itertools.product(E_VALUES, repeat=3):
        exp = codec_encode_doc(tup)
        assert ur.encode_doc(tup) == exp, tup
        buf = np.array(tup, dtype=np.uint16)
        got = b""
        for i in range(3):
            m = sim.sim_u16_e_unit(buf.ctypes.data, 3, i, out4.ctypes.data)
            got += out4[:m].tobytes()
        assert got == exp, tup


# ---- (c) the shim against the reference
@pytest.mark.parametrize("name", [n for n, _ in E_CASES])
def test_rule_header_encodes_as_the_reference(sim, name):
    units, unit_off = ur.batch_units(dict(E_CASES)[name])
    exp, exp_off = ur.encode(units, unit_off)
    for aligned in (True, False):
        got, doc_off = sim_encode(sim, units, unit_off, aligned)
        assert np.array_equal(doc_off, exp_off), (name, aligned, np.flatnonzero(doc_off != exp_off)[:10])
        assert np.array_equal(got, exp), (name, aligned, np.flatnonzero(got != exp)[:10] if len(got) == len(exp) else (len(got), len(exp)))


def test_rule_header_encodes_documents_inside_a_longer_array(sim):
    """unit_off[0] > 0 and unit_off[n_docs] < n_units: the units outside belong to no document, and a surrogate next to them
    pairs with nothing."""
    units = np.array([uc.HI, uc.LO, 0x61, uc.HI, uc.LO, uc.HI, uc.LO, 0x62], dtype=np.uint16)
    unit_off = np.array([1, 4, 6], dtype=np.int64)
    got, doc_off = sim_encode(sim, units, unit_off)
    assert got.tobytes() == b"?a???" and doc_off.tolist() == [0, 3, 5]
    exp, exp_off = ur.encode(units, unit_off)
    assert np.array_equal(got, exp) and np.array_equal(doc_off, exp_off)


def test_rule_header_refuses_bad_offsets(sim):
    units = np.arange(0x41, 0x49, dtype=np.uint16)
    for off in ([-1, 4, 8], [0, 5, 4, 8], [0, 4, 9], [2, 1]):
        assert sim_encode(sim, units, np.array(off, dtype=np.int64))[0] is None, off


@pytest.mark.parametrize("name", [n for n, _ in D_CASES])
def test_rule_header_decodes_as_the_reference(sim, name):
    text, byte_off = ur.batch_bytes(dict(D_CASES)[name])
    exp, exp_off = ur.decode(text, byte_off)
    got, unit_off = sim_decode(sim, text, byte_off)
    assert np.array_equal(unit_off, exp_off), (name, np.flatnonzero(unit_off != exp_off)[:10])
    assert np.array_equal(got, exp), (name, np.flatnonzero(got != exp)[:10] if len(got) == len(exp) else (len(got), len(exp)))


def test_rule_header_on_fuzzed_batches(sim):
    """Many short documents and sequences back to back: every edge lands somewhere in a lane."""
    rng = random.Random(21)
    docs = [_surrogate_dense(rng) for _ in range(3000)]
    units, unit_off = ur.batch_units(docs)
    exp, exp_off = ur.encode(units, unit_off)
    got, doc_off = sim_encode(sim, units, unit_off)
    assert np.array_equal(doc_off, exp_off) and np.array_equal(got, exp)
    seqs = [_malformed_dense(rng) for _ in range(3000)]
    text, byte_off = ur.batch_bytes(seqs)
    exp, exp_off = ur.decode(text, byte_off)
    got, unit_off = sim_decode(sim, text, byte_off)
    assert np.array_equal(unit_off, exp_off) and np.array_equal(got, exp)


# ---- (d) the edges the case set must reach
def test_case_set_reaches_the_edges():
    assert uc.e_edges_reached(dict(E_CASES)["all"]) == uc.E_ALL_EDGES
    assert uc.d_edges_reached(dict(D_CASES)["all"]) == uc.D_ALL_EDGES
    assert uc.E_TILE == uc.LANES * uc.E_LANE and uc.D_TILE == uc.LANES * uc.D_LANE and uc.E_LANE * 2 == 16 and uc.D_LANE == 16
    assert len(set(n for n, _ in E_CASES)) == len(E_CASES) and len(set(n for n, _ in D_CASES)) == len(D_CASES)


# ---- (e) UTF-16 positions of the transcoded text index the original units
def test_utf16_length_of_the_transcoded_text_is_the_unit_count():
    rng = random.Random(3)
    docs = dict(E_CASES)["all"] + [_surrogate_dense(rng) for _ in range(500)]
    r = cr.Ref([ur.encode_doc(d) for d in docs])
    assert np.array_equal(r.doc_units(cr.UTF16), [len(d) for d in docs])


# ---- the stand-alone sanitizer run
def test_sanitizer_build_runs_every_case_in_exact_buffers(tmp_path):
    exe = str(tmp_path / "utf16_sim_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, os.path.join(SIM_DIR, "utf16_sim_main.cpp")])
    rng = random.Random(5)
    jobs = [(0, ur.batch_units(docs)) for _, docs in E_CASES] + [(1, ur.batch_bytes(seqs)) for _, seqs in D_CASES]
    for n in (1, 7, 8, 9, 15, 16, 17):                                       # ragged ends around the granule
        jobs.append((0, ur.batch_units([([uc.LO] + [uc.HI, uc.LO] * 9)[:n]])))
        jobs.append((1, ur.batch_bytes([(b"\x80" + uc.G4 * 5)[:n]])))
    jobs.append((0, ur.batch_units([_surrogate_dense(rng) for _ in range(600)])))
    jobs.append((1, ur.batch_bytes([_malformed_dense(rng) for _ in range(600)])))
    cases, results = str(tmp_path / "cases.bin"), str(tmp_path / "results.bin")
    with open(cases, "wb") as f:
        for kind, (items, off) in jobs:
            f.write(struct.pack("<3q", kind, len(off) - 1, len(items)))
            f.write(off.astype("<i8").tobytes())
            f.write(items.tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe, cases, results], env=env, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-4000:]
    assert p.stdout.strip() == "%d cases" % len(jobs)
    raw = open(results, "rb").read()
    pos = 0
    for kind, (items, off) in jobs:
        total = struct.unpack_from("<q", raw, pos)[0]
        pos += 8
        got_off = np.frombuffer(raw, dtype="<i8", count=len(off), offset=pos)
        pos += 8 * len(off)
        width = 1 if kind == 0 else 2
        got = np.frombuffer(raw, dtype=np.uint8 if kind == 0 else np.uint16, count=total, offset=pos)
        pos += total * width
        exp, exp_off = ur.encode(items, off) if kind == 0 else ur.decode(items, off)
        assert np.array_equal(got_off, exp_off) and np.array_equal(got, exp), kind
    assert pos == len(raw)
