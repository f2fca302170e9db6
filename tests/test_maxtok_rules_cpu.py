"""CPU tier: the maxTokens early-exit rules that jtk_batch_encode_max_tokens (host) and jtk_batch_encode_device_max_tokens
(device) share -- jtokkit_amd/csrc/jtk_maxtok_rules.h: the last safe piece start, the decision, the back-off -- run on the
CPU through the shim tests/maxtok_sim, fed with piece starts from the split-rule shim (libjtk_hostsim.so, sim_split) and
token lists from the oracle.  Whenever the rules decide on a prefix, the result equals the oracle's encode(text, max) of
the whole text.  The case tier beside it, tests/test_maxtok_cases_cpu.py, runs the header's last safe start at a nonzero
`base` with the neighbours' bits in the mask, against the plain model tests/maxtok_ref.py on the batches of
tests/maxtok_cases.py, and asserts that those batches reach the kernels' edges; tests/test_maxtok_edges_gpu.py runs them
on the device."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import oracle_lib
import regex_crosscheck as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sims(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("maxtok_sim") / "libmaxtok_sim.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-o", out,
                           os.path.join(ROOT, "tests", "maxtok_sim", "maxtok_sim.cpp")])
    mt = C.CDLL(out)
    mt.sim_maxtok_decide.restype = C.c_int64
    mt.sim_maxtok_decide.argtypes = [C.c_char_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64,
                                     C.POINTER(C.c_int)]
    mt.sim_maxtok_prefixes.argtypes = [C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_void_p]
    d = os.path.join(ROOT, "tests", "hostsim")
    if not os.path.exists(os.path.join(d, "libjtk_hostsim.so")):
        subprocess.check_call(["make", "-C", d])
    hs = C.CDLL(os.path.join(d, "libjtk_hostsim.so"))
    hs.sim_split.argtypes = [C.c_int, C.c_char_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p]
    return mt, hs


class _Lens:
    """Byte length of every token id (from the oracle's decoder), cached."""
    def __init__(self, o):
        self.o, self.cache = o, {}

    def __call__(self, ids):
        for t in ids:
            if t not in self.cache:
                self.cache[t] = len(self.o.decode_bytes([t]))
        return np.array([self.cache[t] for t in ids] or [0], dtype=np.int32)


def _decide(sims, o, lens, kind, doc, p, mx):
    mt, hs = sims
    pre = doc[:p]
    starts = np.zeros(p + 1, dtype=np.uint8)
    off = np.array([0, p], dtype=np.int64)
    hs.sim_split(kind, pre, p, off.ctypes.data, 1, starts.ctypes.data)
    cuts = np.nonzero(starts)[0].tolist()                   # (the prefix may end inside a character: merged piece by piece)
    toks = [t for a, b in zip(cuts, cuts[1:]) for t in o.merge_piece(pre[a:b])]
    tl = lens(toks)
    tr = C.c_int(0)
    k = mt.sim_maxtok_decide(doc, len(doc), p, starts.ctypes.data, tl.ctypes.data, len(toks), mx, C.byref(tr))
    return k, bool(tr.value), toks


@pytest.mark.parametrize("name,kind", [("cl100k_base", 1), ("r50k_base", 0)])
def test_decisions_equal_the_oracle_for_every_prefix(sims, name, kind):
    """Fuzz texts (mixed scripts, white-space runs, U+FFFD, cut characters) and every prefix length 1..300: a decision is
    always the oracle's encode(text, max) of the whole text."""
    o = oracle_lib.get(name)
    lens = _Lens(o)
    rng = random.Random(31)
    ws = [" ", "  ", "\n", " \n", "\n\n ", "\t", "\r\n", " ", " ", "　", "   "]
    docs = []
    for _ in range(14):
        t = rc.random_text(rng, 120) + "".join(rng.choice(ws) for _ in range(rng.randint(1, 12))) + rc.random_text(rng, 200)
        docs.append(t.encode("utf-8"))
    docs += ["they'll we've 1234567 �� é日本語 " .encode() * 12, ("x" + " \n" * 40 + "y" * 30).encode() * 3]
    n_decided = 0
    for doc in docs:
        for mx in (1, 3, 10):
            exp = o.encode_ordinary(doc, mx)
            for p in range(1, min(300, len(doc)) + 1):
                k, tr, toks = _decide(sims, o, lens, kind, doc, p, mx)
                if k < 0:
                    continue
                n_decided += 1
                assert (toks[:k], tr) == exp, (doc[:60], mx, p)
    assert n_decided > 2000


def test_prose_decides_soon_after_the_tokens(sims):
    """On plain prose the rules decide once the prefix holds max + 16 bytes past the bytes of the first max tokens (plus
    the rest of the word they end in)."""
    from jtokkit_amd import corpus
    o = oracle_lib.get("cl100k_base")
    lens = _Lens(o)
    text, off = corpus.english(30, seed=5, plain=True)
    for d in range(len(off) - 1):
        doc = text[off[d]:off[d + 1]].tobytes()
        for mx in (1, 5, 20):
            full = o.encode_ordinary(doc)
            if len(full) <= mx + 8:
                continue
            nb = int(lens(full[:mx]).sum())
            word_end = nb
            while word_end < len(doc) and doc[word_end:word_end + 1] not in (b" ", b"\n"):
                word_end += 1
            p = word_end + mx + 16
            if p >= len(doc):
                continue
            k, tr, toks = _decide(sims, o, lens, 1, doc, p, mx)
            assert k >= 0, (doc[:80], mx, p)
            assert (toks[:k], tr) == o.encode_ordinary(doc, mx)


def test_prefix_sizes_of_the_rounds(sims):
    mt, _ = sims
    out = np.zeros(4, dtype=np.int64)
    mt.sim_maxtok_prefixes(100000, 10, 1 << 25, 4, out.ctypes.data)
    assert out.tolist() == [144, 576, 2304, 9216]
    mt.sim_maxtok_prefixes(1000, 10, 1 << 25, 4, out.ctypes.data)
    assert out.tolist() == [144, 576, 1000, 1000]
    mt.sim_maxtok_prefixes(1 << 20, 100000, 1 << 20, 2, out.ctypes.data)      # past one chunk: the whole document
    assert out.tolist()[:2] == [800064, 1 << 20]
