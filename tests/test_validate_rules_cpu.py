"""CPU tier of JTK_ENCODE_VALIDATE_UTF8: the rule header jtokkit_amd/csrc/jtk_validate_rules.h -- run serially through the shim
tests/validate_sim the way k_validate_utf8 runs it over the chunks of a job -- against CPython's strict decoder (the reference of
record, tests/validate_ref.py), an independent automaton over Unicode Table 3-7 and the CPU oracle, on every document of every
batch of tests/validate_cases.py.  The case set must reach its edges, so that the GPU tier cannot pass by missing one, and must
tell every wrong version of the automaton -- a constant moved by one, boundaries ignored, empty documents flagged -- from the
right one, so that it covers the rule; and a stand-alone sanitizer build of the shim runs the batches in buffers of exactly
their size.  No GPU."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import oracle_lib
import validate_cases as vc
import validate_ref as vr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIM_DIR = os.path.join(ROOT, "tests", "validate_sim")
BATCHES = vc.batches()
BIG = [n for n, _ in BATCHES if not n.startswith("small_")]
SMALL = [b for n, b in BATCHES if n.startswith("small_")]


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("validate_sim") / "libvalidate_sim.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas", "-o", out,
                           os.path.join(SIM_DIR, "validate_sim.cpp")])
    L = C.CDLL(out)
    L.sim_validate_chunk.restype = C.c_int
    L.sim_validate_chunk.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p]
    return L


def sim_statuses(sim, docs, chunks=None):
    """The shim over the batch, one call per chunk (chunks: pairs of first document and end; default: the batch as one)."""
    text, doc_off = vc.pack(docs)
    text = text.copy()                                                       # (exactly n_bytes readable)
    status = np.zeros(max(len(docs), 1), dtype=np.int32)
    for d0, d1 in ([(0, len(docs))] if chunks is None else chunks):
        assert sim.sim_validate_chunk(text.ctypes.data if len(text) else None, doc_off.ctypes.data, d0, d1, vc.TILE, status.ctypes.data) == 0
    return status[:len(docs)].tolist()


# ---- (a) the references against each other and against the oracle
def test_class_product_is_the_set_the_issue_counts():
    docs = vc.class_product()
    assert len(docs) == vc.N_PRODUCT == 346200 and sum(len(d) for d in docs) == 1369752 and len(set(docs)) == len(docs)
    assert len(vc.CLASS_VALUES) == 24 and vr.statuses(docs).count(0) == vc.N_PRODUCT_GOOD == 1926
    assert sum(len(d) for d in docs) > vc.SMALL_JOB and sum(len(d) for d in vc.class_product_slice()) <= vc.TINY_JOB


@pytest.mark.parametrize("name", BIG + ["small"])
def test_automaton_equals_the_strict_decoder(name):
    for docs in ([dict(BATCHES)[name]] if name != "small" else SMALL):
        assert vr.automaton_statuses(docs) == vr.statuses(docs)


def test_oracle_refuses_exactly_the_malformed_documents():
    """encode_ordinary of the CPU oracle: JTK_ERR_BAD_UTF8 for every malformed document of every batch, tokens for every other."""
    o = oracle_lib.get("cl100k_base")
    L = oracle_lib.lib()
    docs = sorted({d for _, b in BATCHES for d in b})
    out = np.empty(max(len(d) for d in docs) + 1, dtype=np.int32)
    trunc = C.c_int(0)
    wrong = []
    for d in docs:
        n = L.jtko_encode(o._h, d, len(d), 1, -1, out.ctypes.data, len(out), C.byref(trunc))
        if (0 if n >= 0 else n) != (0 if vr.well_formed(d) else vr.BAD_UTF8):
            wrong.append((d, n))
    assert not wrong, wrong[:5]


# ---- (b) the rule header against the reference
@pytest.mark.parametrize("name", BIG)
def test_rule_header_equals_the_strict_decoder(sim, name):
    docs = dict(BATCHES)[name]
    exp = vr.statuses(docs)
    got = sim_statuses(sim, docs)
    assert got == exp, [(i, docs[i], got[i], exp[i]) for i in range(len(docs)) if got[i] != exp[i]][:5]


def test_rule_header_on_the_small_batches(sim):
    for docs in SMALL + [[], [b""], [b"", b""]]:
        assert sim_statuses(sim, docs) == vr.statuses(docs), docs


@pytest.mark.parametrize("plan", ["host", "device"])
def test_rule_header_chunk_by_chunk(sim, plan):
    """The chunks batch cut by the chunk plan: the look-back stops at the chunk's first document, the look-ahead at its end, and
    a byte in front of the chunk flags nothing."""
    docs = vc.chunk_layout()
    starts = (vc.host_chunk_starts if plan == "host" else vc.device_chunk_starts)(vc.pack(docs)[1], vc.MIN_CHUNK)
    assert len(starts) == 4
    chunks = list(zip(starts, starts[1:] + [len(docs)]))
    exp = vr.statuses(docs)
    assert exp.count(vr.BAD_UTF8) == 3                                       # E4 B8 | AD ..., and the stray 80
    assert sim_statuses(sim, docs, chunks) == exp
    for d0, d1 in chunks:                                                    # a chunk alone flags its own documents only
        assert sim_statuses(sim, docs, [(d0, d1)]) == [exp[i] if d0 <= i < d1 else 0 for i in range(len(docs))]


# ---- (c) the edges the case set must reach
def test_case_set_reaches_the_edges():
    reached = set()
    for _, docs in BATCHES:
        reached |= vc.edges_reached(docs)
    assert reached == vc.ALL_EDGES, (sorted(vc.ALL_EDGES - reached), sorted(reached - vc.ALL_EDGES))
    assert len(set(n for n, _ in BATCHES)) == len(BATCHES)
    # the partition constants are the sources'
    src = lambda f: open(os.path.join(ROOT, "jtokkit_amd", "csrc", f)).read()
    assert int(re.search(r"^#define\s+JTK_TILE\s+(\d+)", src("jtk_kernels.h"), re.M).group(1)) == vc.TILE
    abi = src("jtk_abi.cpp")
    assert "TINY_JOB_BYTES = 128 << 10" in abi and "SMALL_JOB_BYTES = 1 << 20" in abi and "value < (1 << 16)" in abi
    k = src("jtk_kernels.hip")
    assert "__launch_bounds__(256) k_validate_utf8" in k and "k_validate_utf8, dim3((unsigned)((w.n_bytes + 255) / 256)), dim3(256)" in k
    assert (vc.WAVE, vc.WORKGROUP, vc.DOCMASK_WORD, vc.MIN_CHUNK, vc.TINY_JOB, vc.SMALL_JOB) == (64, 256, 64, 1 << 16, 128 << 10, 1 << 20)


# ---- (d) the case set covers the rule: every wrong version of the automaton is told from the right one
R = vr.TABLE_3_7_RULE
MUTANTS = [("lead floor C2 -> C1", R._replace(lead_min=0xC1)), ("lead floor C2 -> C3", R._replace(lead_min=0xC3)),
           ("lead ceiling F4 -> F3", R._replace(lead_max=0xF3)), ("lead ceiling F4 -> F5", R._replace(lead_max=0xF5)),
           ("E0 second byte A0 -> 9F", R._replace(e0_min=0x9F)), ("E0 second byte A0 -> A1", R._replace(e0_min=0xA1)),
           ("ED second byte 9F -> 9E", R._replace(ed_max=0x9E)), ("ED second byte 9F -> A0", R._replace(ed_max=0xA0)),
           ("F0 second byte 90 -> 8F", R._replace(f0_min=0x8F)), ("F0 second byte 90 -> 91", R._replace(f0_min=0x91)),
           ("F4 second byte 8F -> 8E", R._replace(f4_max=0x8E)), ("F4 second byte 8F -> 90", R._replace(f4_max=0x90)),
           ("look-back 3 -> 2: no fourth byte", R._replace(max_len=3)),
           ("document boundaries ignored", R._replace(ignore_boundaries=True)),
           ("empty documents take the flag", R._replace(empties_take_flag=True))]


@pytest.mark.parametrize("name", [n for n, _ in MUTANTS])
def test_case_set_tells_a_wrong_rule_from_the_right_one(name):
    rule = dict(MUTANTS)[name]
    if rule.ignore_boundaries or rule.empties_take_flag:
        docs = vc.table_cuts() + vc.bad_kinds()
        assert vr.automaton_statuses(docs, rule) != vr.statuses(docs)
        return
    for d in vc.table_cuts() + vc.bad_kinds() + vc.class_product():
        if vr.automaton_well_formed(d, rule) != vr.well_formed(d):
            return
    pytest.fail("no document of class_product + table_cuts + bad_kinds changes its status under: " + name)


# ---- the stand-alone sanitizer run
def test_sanitizer_build_runs_the_batches_in_exact_buffers(tmp_path):
    exe = str(tmp_path / "validate_sim_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, os.path.join(SIM_DIR, "validate_sim_main.cpp")])
    jobs = [(docs, [0]) for n, docs in BATCHES if n != "class_product"] + [(vc.edge_layout(), [0]), (vc.table_cuts(), [0]), ([], [0]), ([b""], [0])]
    chunks = vc.chunk_layout()
    jobs.append((chunks, vc.host_chunk_starts(vc.pack(chunks)[1], vc.MIN_CHUNK)))
    for n in range(1, 8):                                                    # ragged ends: every cut of two characters
        jobs.append(([(vc.G4 + vc.G3)[:n]], [0]))
        jobs.append(([(b"\x80\x80\x80" + vc.G4)[-n:]], [0]))
    cases, results = str(tmp_path / "cases.bin"), str(tmp_path / "results.bin")
    with open(cases, "wb") as f:
        for docs, starts in jobs:
            text, off = vc.pack(docs)
            f.write(struct.pack("<4q", len(docs), len(text), len(starts), vc.TILE))
            f.write(off.astype("<i8").tobytes())
            f.write(np.array(list(starts) + [len(docs)], dtype="<i8").tobytes())
            f.write(text.tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe, cases, results], env=env, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-4000:]
    assert p.stdout.strip() == "%d cases" % len(jobs)
    raw = open(results, "rb").read()
    pos = 0
    for docs, _ in jobs:
        got = np.frombuffer(raw, dtype="<i4", count=len(docs), offset=pos).tolist()
        pos += 4 * len(docs)
        assert got == vr.statuses(docs)
    assert pos == len(raw)
