"""CPU tier of the character positions: the rule header jtokkit_amd/csrc/jtk_charpos_rules.h -- the index as k_cp_build's lanes
count it, and the header's own rank, forward and inverse walks --, run serially through the shim tests/charpos_sim, against the
plain reference tests/charpos_ref.py on every case of tests/charpos_cases.py: every position of every case, both rounds, all
three units, with the document named and searched; every (d, k) from -1 to doc_units + 2; doc_units; the round trip over the
boundaries of the well-formed documents; and the edges that the case set must reach, so that the GPU tier cannot pass by missing
one.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import charpos_cases as cc
import charpos_ref as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = cc.cases()
NAMES = [n for n, _ in CASES]


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("charpos_sim") / "libcharpos_sim.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-o", out,
                           os.path.join(ROOT, "tests", "charpos_sim", "charpos_sim.cpp")])
    L = C.CDLL(out)
    L.sim_cp_open.restype = C.c_void_p
    L.sim_cp_open.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int]
    L.sim_cp_close.argtypes = [C.c_void_p]
    L.sim_cp_doc_units.argtypes = [C.c_void_p, C.c_void_p]
    L.sim_cp_char_positions.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    L.sim_cp_byte_positions.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    L.sim_cp_word_mismatches.restype = C.c_int64
    L.sim_cp_word_mismatches.argtypes = [C.c_void_p, C.c_int64]
    return L


_refs = {}


def ref(name):
    if name not in _refs:
        _refs[name] = cr.Ref(dict(CASES)[name])
    return _refs[name]


class Opened:
    def __init__(self, sim, r, unit):
        self.sim, self.r = sim, r
        text = np.ascontiguousarray(r.text)
        self.h = sim.sim_cp_open(text.ctypes.data if len(text) else None, r.n_bytes, r.doc_off.ctypes.data, len(r.docs), unit)

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.sim.sim_cp_close(self.h)

    def doc_units(self):
        out = np.full(max(len(self.r.docs), 1), -7, dtype=np.int64)
        self.sim.sim_cp_doc_units(self.h, out.ctypes.data)
        return out[:len(self.r.docs)]

    def char_positions(self, rnd, pos, doc=None):
        out = np.full(len(pos), -7, dtype=np.int64)
        self.sim.sim_cp_char_positions(self.h, rnd, None if doc is None else doc.ctypes.data, pos.ctypes.data, len(pos), out.ctypes.data)
        return out

    def byte_positions(self, doc, k):
        out = np.full(len(doc), -7, dtype=np.int64)
        self.sim.sim_cp_byte_positions(self.h, doc.ctypes.data, k.ctypes.data, len(doc), out.ctypes.data)
        return out


def test_word_count_equals_the_byte_weights(sim):
    """jtk_cp_word_units on every pair of byte values in every pair of lanes of a word, and on random words, for 0..4 valid
    bytes: the sum of jtk_cp_weight over those bytes."""
    vals = np.arange(256, dtype=np.uint32)
    words = [(vals[:, None] << (8 * i) | vals[None, :] << (8 * j)).reshape(-1) for i in range(4) for j in range(i + 1, 4)]
    words.append(np.random.default_rng(3).integers(0, 1 << 32, 200000, dtype=np.uint64).astype(np.uint32))
    w = np.ascontiguousarray(np.concatenate(words), dtype=np.uint32)
    assert sim.sim_cp_word_mismatches(w.ctypes.data, len(w)) == 0


@pytest.mark.parametrize("unit", cr.UNITS)
@pytest.mark.parametrize("name", NAMES)
def test_rule_header_equals_reference_on_every_case(sim, name, unit):
    r = ref(name)
    with Opened(sim, r, unit) as s:
        assert np.array_equal(s.doc_units(), r.doc_units(unit)), (name, unit)
        pos, doc = r.all_positions()
        free = r.free_positions()
        for rnd in cr.ROUNDS:
            got, exp = s.char_positions(rnd, pos, doc), r.expected_char_positions(unit, rnd, pos, doc)
            assert np.array_equal(got, exp), (name, unit, rnd, "named", np.flatnonzero(got != exp)[:10])
            got, exp = s.char_positions(rnd, free), r.expected_char_positions(unit, rnd, free)
            assert np.array_equal(got, exp), (name, unit, rnd, "searched", np.flatnonzero(got != exp)[:10])
        qd, qk = r.all_char_queries(unit)
        got, exp = s.byte_positions(qd, qk), r.expected_byte_positions(unit, qd, qk)
        assert np.array_equal(got, exp), (name, unit, "inverse", np.flatnonzero(got != exp)[:10])


@pytest.mark.parametrize("unit", (cr.UTF16, cr.CODEPOINT))
def test_round_trip_over_the_boundaries_of_well_formed_documents(sim, unit):
    """byte_pos(d, char_index(q)) == q for every boundary q of every well-formed document, either round; and the indices are
    those of Python's own str (code points) and of its UTF-16 form."""
    n_bounds = 0
    for name in NAMES:
        r = ref(name)
        with Opened(sim, r, unit) as s:
            for d, doc in enumerate(r.docs):
                if not cr.well_formed(doc):
                    continue
                a = int(r.doc_off[d])
                text = doc.decode("utf-8")
                starts = np.cumsum([0] + [len(ch.encode("utf-8")) for ch in text]).astype(np.int64)
                pos, dd = a + starts, np.full(len(starts), d, dtype=np.int64)
                idx = s.char_positions(cr.FLOOR, pos, dd)
                assert np.array_equal(idx, s.char_positions(cr.CEIL, pos, dd))
                if unit == cr.CODEPOINT:
                    assert np.array_equal(idx, np.arange(len(text) + 1)), (name, d)
                else:
                    assert np.array_equal(idx, [len(text[:i].encode("utf-16-le")) // 2 for i in range(len(text) + 1)]), (name, d)
                assert np.array_equal(s.byte_positions(dd, idx), pos), (name, d)
                n_bounds += len(pos)
    assert n_bounds > 10000


def test_case_set_reaches_the_edges():
    """Conditions on the inputs, so that a change to the builder cannot quietly lose an edge."""
    assert cc.edges_reached(dict(CASES)["all"]) == cc.ALL_EDGES
    assert cc.edges_reached(dict(CASES)["edges"]) >= {"4-byte character across a block edge", "4-byte character across a superblock edge",
                                                      "document from block edge to block edge",
                                                      "document from superblock edge to superblock edge", "n_bytes % 16 != 0",
                                                      "more than 4 superblocks and a ragged tail"}
    r = ref("all")
    assert not all(cr.well_formed(d) for d in r.docs) and r.n_bytes % 16 != 0
    # a UTF-16 index that points at a low surrogate floors to its character's first byte
    e = cr.Ref(["a\U0001F600b".encode("utf-8")])
    assert [e.byte_pos(0, k, cr.UTF16) for k in range(5)] == [0, 1, 1, 5, 6]
    assert [e.char_index(0, p, cr.UTF16, cr.FLOOR) for p in range(7)] == [0, 1, 1, 1, 1, 3, 4]
    assert [e.char_index(0, p, cr.UTF16, cr.CEIL) for p in range(7)] == [0, 1, 3, 3, 3, 3, 4]
    assert len(set(NAMES)) == len(NAMES)
