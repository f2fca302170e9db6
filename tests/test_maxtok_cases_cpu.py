"""CPU tier of the device maxTokens case set (tests/maxtok_cases.py, run on the GPU by tests/test_maxtok_edges_gpu.py): the set
reaches every edge it names, so that the GPU tier cannot pass by missing one; the plain model tests/maxtok_ref.py returns the
oracle's answer on the whole document for every document of every batch, and the oracle refuses none outside the special-token
references, so that the GPU tier skips nothing; the rule header's last safe start (jtokkit_amd/csrc/jtk_maxtok_rules.h through
the shim tests/maxtok_sim), on a mask built at the model's nonzero `base` with the neighbours' bits around it, is the model's q
for every scan of the scan batches and traps; and the set tells every wrong version of the rules (maxtok_ref.MUTANTS) from the
right one.  No GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import maxtok_cases as mc
import maxtok_ref as ref
import oracle_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = mc.cases()
NAMES = [c.name for c in CASES]
BY_NAME = {c.name: c for c in CASES}


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("maxtok_sim") / "libmaxtok_sim.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-o", out,
                           os.path.join(ROOT, "tests", "maxtok_sim", "maxtok_sim.cpp")])
    L = C.CDLL(out)
    L.sim_maxtok_last_safe_start.restype = C.c_int64
    L.sim_maxtok_last_safe_start.argtypes = [C.c_void_p, C.c_int64, C.c_char_p, C.c_int64]
    return L


def _answers(results):
    return [(r.ids, r.kept, r.truncated, r.status) for r in results]


def _wrong(c, ordinary=True, mutant=None):
    """The documents on which the model (with a mutant) and the oracle on the whole document disagree."""
    got = _answers(mc.model(c.name, ordinary, 0, mutant)[0])
    exp = ref.expected(mc.oracle(c.enc), c.docs, c.max_tokens, ordinary, mc.literals(c.enc))
    return [d for d in range(len(c.docs)) if got[d] != exp[d]]


# ---- (a) the edges
def test_case_set_reaches_every_edge():
    assert len(set(NAMES)) == len(NAMES)
    scan, summ, rnd = set(), set(), set()
    for c in CASES:
        if c.kind in ("scan", "trap"):
            scan |= mc.edges_reached(c)
        elif c.kind == "sum":
            summ |= mc.edges_reached(c)
        elif c.kind == "round":
            rnd |= mc.edges_reached(c)
        elif c.kind == "gather":
            assert c.offsets == mc.GATHER_OFFSETS and c.modes == (True, False)
            for off in c.offsets:
                for ordinary in c.modes:                                     # (under encode() the literal documents are not gathered)
                    got = mc.edges_reached(c, ordinary, off)
                    assert got == mc.GATHER_EDGES, (off, ordinary, sorted(mc.GATHER_EDGES - got)[:5])
        else:
            assert c.kind == "special" and c.offsets == mc.SPECIAL_OFFSETS and c.modes == (False, True)
            got = set().union(*(mc.edges_reached(c, False, off) for off in c.offsets))
            req = mc.special_edges_required(c.enc)
            assert got == req, (c.name, sorted(req - got), sorted(got - req))
    assert scan == mc.SCAN_EDGES, (sorted(mc.SCAN_EDGES - scan), sorted(scan - mc.SCAN_EDGES))
    assert summ == mc.SUM_EDGES, (sorted(mc.SUM_EDGES - summ), sorted(summ - mc.SUM_EDGES))
    assert rnd == mc.ROUND_EDGES, (sorted(mc.ROUND_EDGES - rnd), sorted(rnd - mc.ROUND_EDGES))
    assert {c.enc for c in CASES if c.kind == "special"} == {"p50k_edit", "cl100k_base", mc.CUSTOM["name"]}
    assert {c.enc for c in CASES if c.kind == "trap"} == {"cl100k_base", "r50k_base"}
    assert all(sum(len(d) for d in c.docs) < (512 << 10) for c in CASES)


def test_partition_constants_are_the_sources():
    src = lambda f: open(os.path.join(ROOT, "jtokkit_amd", "csrc", f)).read()
    k = src("jtk_maxtok.hip")
    assert "constexpr int MT_ITEMS = %d;" % mc.PLAN_ITEMS in k and "constexpr int MT_BLOCK = 256;" in k
    assert mc.PLAN_BLOCK == mc.PLAN_ITEMS * 256 and "(n_in + 1023) / 1024" in src("jtk_abi.cpp")
    assert "__launch_bounds__(256) k_mt_special" in k and "16 * i" in k and mc.SPECIAL_WG == 256 * mc.BLOCK
    assert "wh -= 64" in k and "w.piecemask[wi]" in k and (mc.MASK_WORD, mc.STEP_WORDS) == (64, 64)
    rules = src("jtk_maxtok_rules.h")
    assert int(re.search(r"^#define\s+JTK_MAXTOK_MARGIN\s+(\d+)", rules, re.M).group(1)) == mc.MARGIN == ref.MARGIN
    assert "8 * max_tokens + 64" in rules and "P * 4" in rules
    assert int(re.search(r"^#define\s+JTK_TILE\s+(\d+)", src("jtk_kernels.h"), re.M).group(1)) == mc.TILE
    assert "value < (1 << 16)" in src("jtk_abi.cpp") and mc.MIN_CHUNK == 1 << 16
    assert [ref.first_prefix(1) * 4 ** r for r in range(5)] == [72, 288, 1152, 4608, 18432] == mc.prefixes(1, 5)
    assert ref.first_prefix(8) == 128 and mc.prefixes(24, 3) == [256, 1024, 4096]


# ---- (b) the model against the oracle on the whole document
@pytest.mark.parametrize("name", NAMES)
def test_model_equals_the_oracle_on_every_document(name):
    c = BY_NAME[name]
    for ordinary in c.modes:
        assert _wrong(c, ordinary) == []
    for off in c.offsets[1:]:                                                # (where the text lies changes no answer)
        assert _answers(mc.model(name, c.modes[0], off)[0]) == _answers(mc.model(name, c.modes[0], 0)[0])
    if c.kind == "special":
        flagged = sum(ref.special_docs(c.docs, mc.literals(c.enc)))
        assert 25 <= flagged < len(c.docs) - 100
        assert all(r.status == 0 for r in mc.model(name, True, 0)[0])        # encodeOrdinary flags nothing


@pytest.mark.parametrize("name", NAMES)
def test_oracle_refuses_only_the_special_references(name):
    """encode() and encodeOrdinary() of the oracle itself on every whole document: an error only where the special-token
    reference says -2, and no batch but the special ones and the gather batch holds such a document."""
    c = BY_NAME[name]
    o = mc.oracle(c.enc).o
    sp = ref.special_docs(c.docs, mc.literals(c.enc))
    assert not any(sp) or c.kind in ("special", "gather")
    for doc in set(c.docs):
        o.encode_ordinary(doc, c.max_tokens)
        try:
            o.encode(doc, c.max_tokens)
            raised = None
        except oracle_lib.OracleError as e:
            raised = e.code
        assert raised == (ref.UNSUPPORTED_SPECIAL if any(l in doc for l in mc.literals(c.enc)) else None), doc[:60]


# ---- (c) the rule header at the model's base
@pytest.mark.parametrize("name", [c.name for c in CASES if c.kind in ("scan", "trap")])
def test_rule_header_finds_the_models_q_at_a_nonzero_base(sim, name):
    c = BY_NAME[name]
    o = mc.oracle(c.enc)
    n_scans, bases = 0, set()
    for doc, r in zip(c.docs, mc.model(name, True, 0)[0]):
        for sc in r.scans:
            assert _header_q(sim, o, doc, sc) == sc.q, (doc[:40], sc)
            n_scans += 1
            bases.add(sc.base & 63)
    assert n_scans >= 3 and len(bases) > 1
    assert max(sc.base for r in mc.model(name, True, 0)[0] for sc in r.scans) > 0


def _header_q(sim, o, doc, sc):
    """jtk_maxtok_last_safe_start on a mask that holds the prefix's piece starts from bit `base` on, every bit up to and at
    `base` (the documents before it, and its own first byte) and every bit from base + p on (the documents behind it)."""
    n_words = (sc.base + sc.p) // 64 + 3
    bits = np.zeros(n_words * 64, dtype=bool)
    bits[:sc.base + 1] = True
    bits[sc.base + sc.p:] = True
    bits[[sc.base + x for x in o.starts(doc[:sc.p])]] = True
    mask = np.packbits(bits, bitorder="little").view("<u8").copy()
    return sim.sim_maxtok_last_safe_start(mask.ctypes.data, sc.base, doc + b"\0\0", sc.p)


# ---- (d) the case set tells every wrong rule from the right one
def _top_bits_of(c, docs):
    res = mc.model(c.name, True, 0)[0]
    return {res[d].scans[0].top & 63 for d in docs}


@pytest.mark.parametrize("enc", ["cl100k_base", "r50k_base"])
def test_margin_mutant_is_killed_at_every_top_bit(enc):
    c = BY_NAME["traps_" + enc]
    assert set(mc.EDGE_BITS) <= _top_bits_of(c, _wrong(c, mutant="M_margin"))


def test_safe_start_mutant_is_killed_under_cl100k_at_every_top_bit():
    c = BY_NAME["traps_cl100k_base"]
    wrong = _wrong(c, mutant="M_unsafe")
    assert set(mc.EDGE_BITS) <= _top_bits_of(c, wrong) and len(wrong) >= 8   # 16 and 24 spaces, four bits each
    d = b"ab\n" + b" " * 16 + b"\n\xe3\x80\x801 tail"                       # the documented sample
    o = mc.oracle("cl100k_base")
    assert o.tokens(d[:19])[:2] == [370, 198] and o.whole(d, 2)[0] == [370, 35235]


def test_safe_start_trap_search_finds_none_under_r50k():
    """A slice of the search recorded in maxtok_cases (30,000 samples: 8 traps under cl100k_base, none under r50k_base): under the
    r50k pattern neither the search nor the trap batch tells M_unsafe from the rule, which is why it need not be."""
    assert mc.search_safe_start_trap("r50k_base", 600, seed=1) == []
    assert _wrong(BY_NAME["traps_r50k_base"], mutant="M_unsafe") == []


def test_top_plus_one_mutant_is_killed_by_q_at_every_top_bit(sim):
    """No text tells M_top1 by its tokens (the margin has slack: see maxtok_cases), so it is told by q: on the documents with a
    safe start at top + 1 the mutant's q is not the rule header's, at each of the four top bits."""
    for name in ("scan_72", "scan_512", "scan_72_chunked", "scan_512_chunked"):
        c = BY_NAME[name]
        o = mc.oracle(c.enc)
        assert _wrong(c, mutant="M_top1") == []
        right, mutant = mc.model(name, True, 0)[0], mc.model(name, True, 0, "M_top1")[0]
        killed = set()
        for doc, r, m in zip(c.docs, right, mutant):
            for sc, sm in zip(r.scans, m.scans):
                assert (sc.base, sc.p) == (sm.base, sm.p)
                if sm.q != _header_q(sim, o, doc, sc):
                    assert sm.q == sc.p - mc.MARGIN + 1 and sc.q < sm.q
                    killed.add(sc.top & 63)
        assert set(mc.EDGE_BITS) <= killed, (name, killed)


@pytest.mark.parametrize("mutant", ["M_sum64", "M_min"])
def test_sum_mutants_are_killed(mutant):
    killed = {c.max_tokens for c in CASES if c.kind == "sum" and _wrong(c, mutant=mutant)}
    assert killed >= ({65, 127, 128, 129} if mutant == "M_sum64" else set(mc.SUM_LIMITS)), killed
    if mutant == "M_sum64":                                                  # (at 64 tokens and below the first sum is the whole sum)
        assert not killed & {63, 64, 2}
