"""CPU tier: the boundary-preferring chunking rule of jtk_batch_chunk_prefer (jtokkit_amd/csrc/jtk_chunk_prefer_rules.h), run on
the CPU through the shim tests/chunk_prefer_sim, against a plain restatement (tests/chunk_prefer_ref.py) on oracle token lists
-- golden prompts of the four encodings, seeded fuzz, the probe document --, for every prefer mask 0..15 and the (N, overlap)
grid of test_chunk_rules_cpu.py crossed with min_tokens in {1, (N + 1) // 2, N}; and the rule's invariants."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import chunk_prefer_ref as ref
import chunk_ref
import golden_util
import oracle_lib
import regex_crosscheck as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRID_N = (1, 2, 3, 4, 7, 64, 512)


def _grid():
    for N in GRID_N:
        for ov in sorted({0, 1, N - 1}):
            if ov < N:
                for mt in sorted({1, (N + 1) // 2, N}):
                    yield N, ov, mt


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("chunk_prefer_sim") / "libchunk_prefer_sim.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-o", out,
                           os.path.join(ROOT, "tests", "chunk_prefer_sim", "chunk_prefer_sim.cpp")])
    L = C.CDLL(out)
    L.sim_cut_levels.restype = None
    L.sim_cut_levels.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_uint32, C.c_void_p]
    L.sim_chunk_prefer.restype = C.c_int64
    L.sim_chunk_prefer.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_int64]
    return L


def _sim_levels(sim, tb, prefer):
    D = np.frombuffer(b"".join(tb) + b"\0", dtype=np.uint8)
    pos = np.zeros(len(tb) + 1, dtype=np.int64)
    np.cumsum([len(x) for x in tb], out=pos[1:])
    lv = np.zeros(len(tb) + 1, dtype=np.uint8)
    sim.sim_cut_levels(D.ctypes.data, pos.ctypes.data, len(tb), prefer, lv.ctypes.data)
    return lv[:len(tb)]


def _sim_chunks(sim, lv, N, ov, mt):
    lv = np.ascontiguousarray(lv, dtype=np.uint8)
    cap = len(lv) + 1
    s, e = np.zeros(cap, dtype=np.int64), np.zeros(cap, dtype=np.int64)
    sp, el = np.zeros(cap, dtype=np.uint8), np.zeros(cap, dtype=np.uint8)
    k = sim.sim_chunk_prefer(lv.ctypes.data, len(lv), N, ov, mt, s.ctypes.data, e.ctypes.data, sp.ctypes.data, el.ctypes.data, cap)
    return [(int(s[i]), int(e[i]), bool(sp[i]), int(el[i])) for i in range(k)]


def _tokens(o, doc):
    try:
        return o.encode_ordinary(doc)
    except oracle_lib.OracleError:                         # malformed UTF-8: the bytes merged as one piece
        return o.merge_piece(doc)


def _check_doc(sim, o, doc, seen, inv_masks=range(16)):
    """Shim against restatement for every mask and the whole grid; the invariants for the masks in inv_masks."""
    toks = _tokens(o, doc)
    tb = ref.token_bytes(o, toks)
    D = b"".join(tb)
    cum = np.concatenate([[0], np.cumsum([len(x) for x in tb])]).astype(np.int64)
    fb = chunk_ref.first_bytes(o, toks)
    n = len(toks)
    for prefer in range(16):
        lv = ref.levels(tb, prefer)
        assert _sim_levels(sim, tb, prefer).tolist() == lv, (doc[:60], prefer)
        for i in range(1, n):
            assert (lv[i] != 0) == ((fb[i] & 0xC0) != 0x80)                        # B(i) of jtk_chunk_rules.h
            assert 1 <= lv[i] <= 5 or lv[i] == 0
            if lv[i] >= ref.LINE_:
                assert D[cum[i] - 1] == 0x0A
        for N, ov, mt in _grid():
            got = _sim_chunks(sim, lv, N, ov, mt)
            assert got == ref.chunks(lv, N, ov, mt), (doc[:60], prefer, N, ov, mt)
            assert got == ref.chunks_fast(lv, N, ov, mt), (doc[:60], prefer, N, ov, mt)
            seen.update(c[3] for c in got)
            if prefer not in inv_masks:
                continue
            if not toks:
                assert got == []
                continue
            assert got[0][0] == 0 and got[-1][1] == n and got[-1][3] == ref.DOC_END_
            for (s, e, split, el) in got:
                assert 0 < e - s <= N                                              # at most N tokens, progress
                assert el == (ref.DOC_END_ if e == n else lv[e])
                assert split == (not ((s == 0 or lv[s] != 0) and (e == n or lv[e] != 0)))
                if 4 <= el <= 5:
                    assert D[cum[e] - 1] == 0x0A                                   # ends right after \n
                if e < n and e - s < mt:
                    assert all(lv[i] == 0 for i in range(s + mt, s + N + 1))       # below min_tokens only by the back-off
            for (s0, e0, _, _), (s1, _, _, _) in zip(got, got[1:]):
                assert s0 < s1 <= e0 and e0 - s1 <= ov
            if ov == 0:
                assert [t for (s, e, _, _) in got for t in toks[s:e]] == toks      # concatenation
            if prefer == 0 and mt == 1:
                assert [c[:3] for c in got] == chunk_ref.chunks(fb, N, ov)


@pytest.mark.parametrize("name", golden_util.ENCODING_NAMES)
def test_golden_prompts(sim, name):
    o = oracle_lib.get(name)
    seen = set()
    for inp, _, _ in golden_util.load_rows(name):
        _check_doc(sim, o, inp.encode("utf-8"), seen, inv_masks=(0, 15))
    assert {1, 2, 6} <= seen


def test_fuzz(sim):
    o = oracle_lib.get("cl100k_base")
    seen = set()
    rng = random.Random(43)
    for _ in range(40):
        _check_doc(sim, o, rc.random_text(rng, 80).encode("utf-8"), seen)
    for doc in (b"", b"a", b"\n\n", b"a\n\nb", b"\x80\x80abc\n\n\x80", "x。y！z？w".encode(), b"a.\r\n\r\nb. c"):
        _check_doc(sim, o, doc, seen)


def test_probe_document_reaches_every_level(sim):
    """Condition of the feature: over the grid on the probe document, every end level 0..6 occurs."""
    o = oracle_lib.get("cl100k_base")
    doc = ref.PROBE.encode("utf-8")
    assert len(o.encode_ordinary(doc)) == 1046
    seen = set()
    _check_doc(sim, o, doc, seen)
    assert seen == set(range(7)), seen


def test_paragraph_never_looks_into_the_previous_document(sim):
    """The lookback stops at the document's start: with "\\n" as the last byte of the document before, a document that starts
    with "\\n" has LINE, not PARAGRAPH, at its first cut; the same bytes inside one document give PARAGRAPH."""
    o = oracle_lib.get("cl100k_base")
    one = lambda s: [o.decode_bytes([t]) for t in o.merge_piece(s)]
    nl = one(b"\n")
    assert nl == [b"\n"]
    tb = nl + one(b"abc")
    assert ref.levels(tb, 15)[1] == ref.LINE_ and _sim_levels(sim, tb, 15)[1] == ref.LINE_
    tb2 = nl + tb
    assert ref.levels(tb2, 15)[2] == ref.PARAGRAPH_ and _sim_levels(sim, tb2, 15)[2] == ref.PARAGRAPH_
    tb3 = [b"\r", b"\n"] + one(b"abc")                                              # x(3) is none: \r\n alone is a LINE
    assert ref.levels(tb3, 15)[2] == ref.LINE_ and _sim_levels(sim, tb3, 15)[2] == ref.LINE_
