"""CPU tier: the token-budget chunking rule of jtk_batch_chunk (jtokkit_amd/csrc/jtk_chunk_rules.h), run on the CPU through
the shim tests/chunk_sim, against a plain restatement of the rule (tests/chunk_ref.py) on oracle token lists -- golden prompts
of the four encodings, seeded corpus fuzz, emoji / CJK / Indic runs, lone continuation bytes -- and the rule's invariants:
at most N tokens per chunk, concatenation to encode(doc) without overlap, unflagged chunks are whole characters equal to their
byte span, chunk 0 equals encode(doc, N) where that cut is a byte boundary."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

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
                yield N, ov


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("chunk_sim") / "libchunk_sim.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-o", out,
                           os.path.join(ROOT, "tests", "chunk_sim", "chunk_sim.cpp")])
    L = C.CDLL(out)
    L.sim_chunk.restype = C.c_int64
    L.sim_chunk.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]
    return L


def _sim_chunks(sim, fb, N, ov):
    fb = np.ascontiguousarray(fb, dtype=np.uint8)
    cap = len(fb) + 1
    s = np.zeros(cap, dtype=np.int64)
    e = np.zeros(cap, dtype=np.int64)
    sp = np.zeros(cap, dtype=np.uint8)
    k = sim.sim_chunk(fb.ctypes.data, len(fb), N, ov, s.ctypes.data, e.ctypes.data, sp.ctypes.data, cap)
    return [(int(s[i]), int(e[i]), bool(sp[i])) for i in range(k)]


def _check_doc(sim, o, doc, stats):
    try:
        toks = o.encode_ordinary(doc)
    except oracle_lib.OracleError:                         # malformed UTF-8: the bytes merged as one piece
        toks = o.merge_piece(doc)
    fb = chunk_ref.first_bytes(o, toks)
    lens = [len(o.decode_bytes([t])) for t in toks]
    cum = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    assert cum[-1] == len(doc)
    valid = True
    try:
        doc.decode("utf-8")
    except UnicodeDecodeError:
        valid = False
    for N, ov in _grid():
        got = _sim_chunks(sim, fb, N, ov)
        assert got == chunk_ref.chunks(fb, N, ov), (doc[:60], N, ov)
        if not toks:
            assert got == []
            continue
        assert got[0][0] == 0 and got[-1][1] == len(toks)
        for (s, e, split) in got:
            assert 0 < e - s <= N
            if split:
                stats["split"] += 1
                stats.setdefault("split_N", set()).add(N)
            elif valid:
                piece = o.decode_bytes(toks[s:e])
                assert piece == doc[cum[s]:cum[e]]
                piece.decode("utf-8")                      # whole characters
        for (s0, e0, _), (s1, _, _) in zip(got, got[1:]):
            assert s0 < s1 <= e0 and e0 - s1 <= ov
        if ov == 0:
            assert [t for (s, e, _) in got for t in toks[s:e]] == toks
        try:
            ref, _ = o.encode_ordinary(doc, N)
        except oracle_lib.OracleError:                     # (the oracle's maxTokens path takes well-formed text only)
            continue
        if ref and (cum[len(ref)] == len(doc) or (doc[cum[len(ref)]] & 0xC0) != 0x80):
            assert toks[:got[0][1]] == ref, (doc[:60], N)
            stats["chunk0"] += 1


@pytest.mark.parametrize("name", golden_util.ENCODING_NAMES)
def test_golden_prompts(sim, name):
    o = oracle_lib.get(name)
    stats = {"split": 0, "chunk0": 0}
    for inp, _, _ in golden_util.load_rows(name):
        _check_doc(sim, o, inp.encode("utf-8"), stats)
    assert stats["chunk0"] > 100


def test_corpus_fuzz(sim):
    from jtokkit_amd import corpus
    o = oracle_lib.get("cl100k_base")
    stats = {"split": 0, "chunk0": 0}
    rng = random.Random(41)
    for text, off in (corpus.mixed(12, mean_bytes=1500, lo=64, hi=4000, seed=9), corpus.english(12, seed=8)):
        for d in range(len(off) - 1):
            doc = bytes(text[off[d]:off[d + 1]])
            a = rng.randrange(0, max(1, len(doc) - 600))
            while a < len(doc) and (doc[a] & 0xC0) == 0x80:
                a += 1
            _check_doc(sim, o, doc[a:a + 600].decode("utf-8", "ignore").encode("utf-8"), stats)
    for _ in range(40):
        _check_doc(sim, o, rc.random_text(rng, 80).encode("utf-8"), stats)
    assert stats["chunk0"] > 100


@pytest.mark.parametrize("name", ["cl100k_base", "r50k_base"])
def test_scripts_and_continuation_bytes(sim, name):
    """Emoji, CJK and Indic runs split into byte-level tokens, and lone continuation bytes: the flagged path is taken."""
    o = oracle_lib.get(name)
    stats = {"split": 0, "chunk0": 0}
    docs = ["\U0001F355" * 9, "I love \U0001F355\U0001F680\U0001F9E0 ok", "\U0001F468‍\U0001F469‍\U0001F467" * 3,
            "日本語のテキストを分割する" * 3, "漢字龘靐齉" * 4, "हिन्दी भाषा में पाठ " * 3, "தமிழ் உரை " * 3,
            "한국어 텍스트 " * 4, "a��b�"]
    bdocs = [d.encode("utf-8") for d in docs] + [b"\x80\x80abc", b"ab\x80", b"\xbf", b"x\xe6\x97y\x80\x80\x80z" * 3]
    for doc in bdocs:
        _check_doc(sim, o, doc, stats)
    assert stats["split"] > 0 and min(stats["split_N"]) <= 3
