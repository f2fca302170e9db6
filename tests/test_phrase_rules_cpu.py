"""CPU tier of phrase sets (jtk_phrase_set_*, jtk_batch_phrase_hits): the host table build and the walk of the rule header
jtokkit_amd/csrc/jtk_phrase_rules.h through the shim tests/phrase_sim against the plain restatement and on the cases of
tests/phrase_ref.py (the per-document outputs: units are the device tier's), and the refusals of the build.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import phrase_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PER_DOC = pr.OUTS[:4]


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("phrase_sim") / "libphrase_sim.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas", "-o", out,
                           os.path.join(ROOT, "tests", "phrase_sim", "phrase_sim.cpp")])
    L = C.CDLL(out)
    p = C.c_void_p
    L.sim_ph_build.restype, L.sim_ph_build.argtypes = p, [p, p, p, C.c_int64, C.c_uint32, C.POINTER(C.c_char_p)]
    L.sim_ph_free.restype, L.sim_ph_free.argtypes = None, [p]
    L.sim_ph_hits.restype, L.sim_ph_hits.argtypes = None, [p, p, C.c_int64, p, p, C.c_int64, p, p, p, p]
    return L


def build(sim, phrases, flags, groups=None):
    """(set or None, the refusal or None); the call copies what it reads"""
    blob, off = pr.pack(phrases)
    off = off.astype(np.uint32)
    grp = np.array(list(groups if groups is not None else [0] * len(phrases)) + [0], dtype=np.uint8)
    what = C.c_char_p()
    return sim.sim_ph_build(blob.ctypes.data, off.ctypes.data, grp.ctypes.data, len(phrases), flags, C.byref(what)), what.value


@pytest.mark.parametrize("word_bounds", [False, True])
@pytest.mark.parametrize("fold", [False, True])
@pytest.mark.parametrize("name", list(pr.CASES))
def test_build_and_walk_equal_restatement(sim, name, fold, word_bounds):
    c = pr.CASES[name]
    s, what = build(sim, [ph for ph, _ in c.phrases], (1 if fold else 0) | (2 if word_bounds else 0), [g for _, g in c.phrases])
    assert s and what is None
    exp = pr.hits(c.docs, c.status, c.phrases, fold, word_bounds)
    text, doc_off = pr.pack(c.docs)
    status = np.array(c.status, dtype=np.int32)
    got = {k: np.full(len(c.docs), -1 if k.startswith("first") else 0, dtype=dt) for k, dt in PER_DOC}
    sim.sim_ph_hits(s, text.ctypes.data, len(text), doc_off.ctypes.data, status.ctypes.data, len(c.docs), *[got[k].ctypes.data for k, _ in PER_DOC])
    sim.sim_ph_free(s)
    for k in got:
        assert np.array_equal(got[k], exp[k]), (k, got[k], exp[k])
    assert name != "dense_one_document" or word_bounds or got["n_hits"][0] == 19999


def test_refusals_make_no_set(sim):
    ok = [b"ab", b"c"]
    for phrases, flags, groups in (([b""], 0, None), ([b"x" * 65], 0, None), (ok, 4, None), (ok, 0, [0, 32]), ([b"ab%d" % i for i in range(65537)], 0, None),
                                   ([b"%063d" % i for i in range(16645)], 0, None)):          # (16,645 x 63 bytes: 1 MiB + 59)
        s, what = build(sim, phrases, flags, groups)
        assert not s and what, (phrases[:2], flags, groups)
    for phrases, flags, groups in (([], 3, None), ([b"x" * 64, b"y"], 3, [31, 0]), ([b"ab%d" % i for i in range(65536)], 0, None)):
        s, what = build(sim, phrases, flags, groups)
        assert s and what is None
        sim.sim_ph_free(s)
