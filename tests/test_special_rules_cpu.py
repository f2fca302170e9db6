"""CPU tier: the match selection of the allow-special encode (JTK_ENCODE_ALLOW_SPECIAL; jtokkit_amd/csrc/jtk_special_rules.h),
run on the CPU through the shim tests/special_sim, against the plain restatement tests/special_ref.py -- the shipped encodings'
literals, custom overlapping sets, seeded random text dense in literal fragments -- and the restatement itself on hand-checked
vectors of the oracle."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import golden_util
import oracle_lib
import special_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("special_sim") / "libspecial_sim.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-o", out,
                           os.path.join(ROOT, "tests", "special_sim", "special_sim.cpp")])
    L = C.CDLL(out)
    L.sim_special.restype = C.c_int64
    L.sim_special.argtypes = [C.c_char_p, C.c_int64, C.c_int, C.c_void_p, C.c_char_p, C.c_void_p,
                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int32)]
    return L


def _sim(sim, doc, lits, allowed):
    """lits: [bytes]; allowed: set of literals -> ([(s, e, literal)], disallowed present)."""
    off = np.zeros(len(lits) + 1, dtype=np.uint32)
    off[1:] = np.cumsum([len(x) for x in lits])
    al = np.array([1 if x in allowed else 0 for x in lits] + [0], dtype=np.uint8)
    cap = len(doc) + 1
    s, e = np.zeros(cap, dtype=np.int64), np.zeros(cap, dtype=np.int64)
    li = np.zeros(cap, dtype=np.int32)
    dis = C.c_int32(0)
    k = sim.sim_special(doc, len(doc), len(lits), off.ctypes.data, b"".join(lits), al.ctypes.data, s.ctypes.data, e.ctypes.data,
                        li.ctypes.data, cap, C.byref(dis))
    return [(int(s[i]), int(e[i]), lits[int(li[i])]) for i in range(k)], bool(dis.value)


def _check(sim, doc, lits, allowed):
    got, dis = _sim(sim, doc, lits, allowed)
    amap = {x: x for x in lits if x in allowed}
    exp = special_ref.matches(doc, amap)
    assert got == [(s, e, x) for (s, e, x) in exp], (doc[:80], allowed)
    assert dis == special_ref.disallowed_in(doc, lits, amap)
    return len(got)


def test_restatement_hand_checked():
    o = oracle_lib.get("cl100k_base")
    eot = {b"<|endoftext|>": 100257}
    assert o.encode_ordinary(b"<|endoftext|>") == [27, 91, 8862, 728, 428, 91, 29]
    assert special_ref.encode(o, b"foo  <|endoftext|>", eot) == [8134, 256, 100257]
    assert o.encode_ordinary(b"foo  <|endoftext|>")[:2] == [8134, 220]          # (the whole text's split differs)
    assert special_ref.encode(o, b"it<|endoftext|>'s", eot) == [275, 100257, 596]
    assert special_ref.encode(o, b"a<|fim_prefix|>b", eot, [b"<|fim_prefix|>"]) is None
    assert special_ref.encode(o, b"a<|fim_prefix|>b", eot, [b"<|fim_prefix|>"], ordinary=True) == o.encode_ordinary(b"a<|fim_prefix|>b")


@pytest.mark.parametrize("name", golden_util.ENCODING_NAMES)
def test_shipped_literals(sim, name):
    lits = [k.encode() for k in oracle_lib.ENCODINGS[name]["specials"]]
    rng = random.Random(len(lits))
    n = 0
    for inp, _, _ in golden_util.load_rows(name)[:60]:
        b = inp.encode("utf-8")
        for _ in range(3):
            parts = [b[:rng.randint(0, len(b))]]
            for _ in range(rng.randint(0, 4)):
                parts.append(rng.choice(lits) + (b"" if rng.random() < 0.3 else rng.choice([b" ", b"12", b"\xe6\x97\xa5", b"<|", b"x"])))
            doc = b"".join(parts)
            for allowed in (set(lits), set(lits[:1]), set(lits[1:]), set()):
                n += _check(sim, doc, lits, allowed)
    assert n > 100


CUSTOM = [
    [b"aa", b"aaa", b"a"],
    [b"<a>", b"<a>b"],
    [b"\xe6\x97\xa5\xe6\x9c\xac", b"\xe6\x97\xa5"],
    [b"xyx", b"yxy", b"x"],
    [b"abab", b"bab", b"ba"],
]


@pytest.mark.parametrize("k", range(len(CUSTOM)))
def test_custom_overlapping_sets(sim, k):
    lits = CUSTOM[k]
    alphabet = sorted({bytes([c]) for x in lits for c in x}) + [b" ", b"<", b"z"]
    rng = random.Random(100 + k)
    chains = 0
    for _ in range(400):
        doc = b"".join(rng.choice(alphabet + lits) for _ in range(rng.randint(0, 40)))
        for allowed in (set(lits), {lits[0]}, set(lits[1:])):
            _check(sim, doc, lits, allowed)
        cands = [p for p in range(len(doc)) if any(doc.startswith(x, p) for x in lits)]
        chains += any(b - a < max(len(x) for x in lits) for a, b in zip(cands, cands[1:]))
    assert chains > 50


def test_random_dense_fragments(sim):
    lits = [b"<|endoftext|>", b"<|end|>", b"<|e", b"|>", b"<<|"]
    frags = [b"<", b"|", b"<|", b"|>", b"end", b"oftext", b"e", b" ", b"\n", b"7"] + lits
    rng = random.Random(7)
    for _ in range(800):
        doc = b"".join(rng.choice(frags) for _ in range(rng.randint(0, 50)))
        allowed = {x for x in lits if rng.random() < 0.6}
        _check(sim, doc, lits, allowed)
