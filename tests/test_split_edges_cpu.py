"""CPU tier of the split edge sweep: the cases of split_edge_cases.py are sound without a GPU.  The 64-bit mask algebra
with waves of 62 blocks (jtk_split_masks.h through tests/hostsim) equals the per-byte rules and the oracle on exactly the
batches that test_split_edges_gpu.py sends through the kernel, so a failure there points at the device glue."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import oracle_lib
import regex_crosscheck as rc
import split_edge_cases as sec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = {1: "cl100k_base", 0: "r50k_base"}


@pytest.fixture(scope="module")
def sim():
    d = os.path.join(ROOT, "tests", "hostsim")
    subprocess.check_call(["make", "-C", d, "-s"])
    L = C.CDLL(os.path.join(d, "libjtk_hostsim.so"))
    L.sim_split.argtypes = [C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p]
    L.sim_split_masks.argtypes = [C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p]
    L.sim_class_bytes_at.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p]
    return L


def _oracle_mask(name, text, doc_off):
    """1 where the oracle's split() starts a piece, joined per document (and at the end of the text)."""
    o = oracle_lib.get(name)
    lib = oracle_lib.lib()
    ms = np.zeros(len(text) + 1, dtype=np.uint8)
    ms[len(text)] = 1
    raw = np.ascontiguousarray(text)
    ends = np.empty(int(np.diff(doc_off).max()) + 1, dtype=np.int64)
    for d in range(len(doc_off) - 1):
        a, n = int(doc_off[d]), int(doc_off[d + 1] - doc_off[d])
        if n == 0:
            continue
        k = lib.jtko_split(o._h, C.c_char_p(raw.ctypes.data + a), n, ends.ctypes.data, len(ends))
        assert k > 0 and ends[k - 1] == n
        ms[a] = 1
        ms[a + ends[:k - 1]] = 1
    return ms


def _batches(kind):
    for i, ch in enumerate(sec.wave_chains(kind)):
        for mode in ("a", "b"):
            yield "wave %d mode %s" % (i, mode), ch, mode
    for what, chains in (("full-span", sec.full_span_chains(kind)), ("beyond", sec.beyond_chains(kind))):
        for i, ch in enumerate(chains):
            for mode in ("a", "b"):
                yield "%s %d mode %s" % (what, i, mode), ch, mode
    for i, ch in enumerate(sec.mode_c_chains(kind)):
        for mode in ("c-1", "c0", "c+1"):
            yield "mode-c %d %s" % (i, mode), ch, mode
    for mode in ("a", "b"):
        yield "block mode %s" % mode, sec.block_chain(kind), mode
    if kind == 1:
        yield "special", sec.special_chain(), "b"


@pytest.mark.parametrize("kind", [1, 0])
def test_mask_algebra_equals_rules_and_oracle_on_the_edge_batches(sim, kind):
    for what, ch, mode in _batches(kind):
        text, doc_off, _ = ch.batch(mode)
        n, nd = len(text), len(doc_off) - 1
        ref = np.zeros(n + 1, dtype=np.uint8)
        sim.sim_split(kind, text.ctypes.data, n, doc_off.ctypes.data, nd, ref.ctypes.data)
        ms = np.zeros(n + 1, dtype=np.uint8)
        n_slow = C.c_int64(0)
        sim.sim_split_masks(kind, text.ctypes.data, n, doc_off.ctypes.data, nd, 62, ms.ctypes.data, C.byref(n_slow))
        bad = np.nonzero(ms != ref)[0]
        assert len(bad) == 0, (what, int(bad[0]), ch.label_at(bad[0]))
        bad = np.nonzero(_oracle_mask(NAME[kind], text, doc_off) != ref)[0]
        assert len(bad) == 0, (what, int(bad[0]), ch.label_at(bad[0]))


def test_text_tails_and_probes_on_the_cpu(sim):
    """The same for the text tails (both kinds) and for every code point's probe document (the mask algebra with the per-byte
    classes; jtk_block_classify.h has its own every-code-point test in test_abi_and_host.py)."""
    text, doc_off, _ = sec.every_codepoint_docs()
    cases = [("probes", text, doc_off)] + sec.text_tails()
    for kind in (1, 0):
        for label, t, off in cases:
            n, nd = len(t), len(off) - 1
            ref = np.zeros(n + 1, dtype=np.uint8)
            sim.sim_split(kind, t.ctypes.data, n, off.ctypes.data, nd, ref.ctypes.data)
            ms = np.zeros(n + 1, dtype=np.uint8)
            n_slow = C.c_int64(0)
            sim.sim_split_masks(kind, t.ctypes.data, n, off.ctypes.data, nd, 62, ms.ctypes.data, C.byref(n_slow))
            assert np.array_equal(ms, ref), (kind, label)
            if label != "probes":
                assert np.array_equal(_oracle_mask(NAME[kind], t, off), ref), (kind, label)


@pytest.mark.parametrize("kind", [1, 0])
def test_sampled_segments_against_the_regex_engine(kind):
    """2,000 seeded segments, each cut out with its own context, construct and tail: a general backtracking regex engine
    with the reference's pattern agrees with the oracle on them."""
    o = oracle_lib.get(NAME[kind])
    chains = sec.wave_chains(kind) + sec.full_span_chains(kind) + sec.beyond_chains(kind) + [sec.block_chain(kind)]
    pool = [(ch, i) for ch in chains for i in range(ch.n_segments() - 1) if not ch.labels[i].startswith("pad")]
    rng = random.Random(2024 + kind)
    for ch, i in rng.sample(pool, 2000):
        a = ch._snap(i * ch.stride + 32)                       # past the tail of the construct before
        b = ch._snap((i + 1) * ch.stride + 32)
        s = ch.text[a:b].tobytes().decode("utf-8")
        assert rc.split(kind, s) == o.split(s), ch.labels[i]


@pytest.mark.parametrize("kind", [1, 0])
def test_generator_self_checks(kind):
    waves = sec.wave_chains(kind)
    others = sec.full_span_chains(kind) + sec.beyond_chains(kind)
    for ch in waves + others + sec.mode_c_chains(kind) + [sec.block_chain(kind), sec.special_chain()]:
        assert len(ch.text) == ch.n_segments() * ch.stride and len(ch.text) < sec.MAX_BATCH
        ch.text.tobytes().decode("utf-8")                      # valid UTF-8: no character was cut
        assert len(set(ch.labels)) == len(ch.labels)
        for mode in ("a", "b", "c-1", "c0", "c+1"):
            off = ch.doc_off(mode)
            assert off[0] == 0 and off[-1] == len(ch.text) and (np.diff(off) > 0).all() and ch.char_start[off[:-1]].all()
    assert all(ch.stride == sec.WAVE for ch in waves)
    # every (construct, k): on a workgroup edge with r = 0 and with a full-span context; every r, the full span included,
    # after every context type its family allows
    on_wg, seen = set(), set()
    for ch in waves + others:
        assert ch is waves[-1] or ch in others or (ch.n_segments() - 1) % 8 == 0
        for i, lab in enumerate(ch.labels[:-1]):
            if lab.startswith("pad"):
                continue
            ck, ctx, r = lab.rsplit("|", 2)
            seen.add((ck, ctx, r))
            if ch in waves and (i + 1) * ch.stride % sec.WORKGROUP == 0:
                on_wg.add((ck, r))
    for family, name, body, _ in sec.constructs(kind):
        ks = ["%s:%s|k=%d" % (family, name, k) for k in range(len(body.encode("utf-8")) + 2)]
        for ck in ks:
            assert (ck, "r=0") in on_wg and (ck, "r=full") in on_wg, ck
            for ctx in sec.CONTEXTS_OF[family]:
                assert {(ck, "ctx=" + ctx, "r=%s" % r) for r in sec.R_WAVE if r != 0} <= seen, (ck, ctx)
        assert any((ck, "ctx=" + sec.WG_FULL[kind], "r=beyond") in seen for ck in ks), name
    assert {ck for ck, _, _ in seen} == {"%s:%s|k=%d" % (f, n, k) for f, n, b, _ in sec.constructs(kind)
                                         for k in range(len(b.encode("utf-8")) + 2)}
    # the block chain: no edge is a wave edge
    bc = sec.block_chain(kind)
    for i, lab in enumerate(bc.labels[:-1]):
        assert lab.startswith("pad") == ((i + 1) * bc.stride % sec.WAVE == 0)


def test_what_the_code_point_probes_can_see(sim):
    """For each class of c, how many code points' probe tokens differ from the tokens the probe gives when a fixed character
    of another class stands in for c -- compared by where the token boundaries fall among the probe's fixed ASCII
    characters.  Non-zero for every ordered pair of N, W and {L, O}; the counts are printed as a record of what
    test_every_code_point_on_the_device can see, not as a threshold."""
    text, doc_off, cps = sec.every_codepoint_docs()
    lead = np.ascontiguousarray(doc_off[:-1] + 1)                # c's first byte in its probe
    codes = np.zeros(len(cps), dtype=np.uint8)
    sim.sim_class_bytes_at(text.ctypes.data, len(text), lead.ctypes.data, len(lead), codes.ctypes.data)
    cls = np.array(["O", "L", "N", "W"])[codes & 3]              # JTK_CLS_O, _L, _N, _W of the project's own class table
    grp = np.where((cls == "L") | (cls == "O"), "LO", cls)
    reps = {"N": ["٣"], "W": [" "], "LO": ["é", "€"]}
    for name in ("cl100k_base", "r50k_base"):
        o = oracle_lib.get(name)
        tok, tok_off = o.encode_batch(text, doc_off, threads=8)
        tlen = {int(t): len(o.decode_bytes([int(t)])) for t in np.unique(tok)}
        lens = np.array([tlen[int(t)] for t in tok], dtype=np.int64)
        ends = np.cumsum(lens)
        doc_of_tok = np.repeat(np.arange(len(cps)), np.diff(tok_off))
        rel = ends - doc_off[doc_of_tok]                         # byte offset in its document where each token ends
        n_u = (np.diff(doc_off)[doc_of_tok] - 8) // 2
        assert (ends[tok_off[1:] - 1] == doc_off[1:]).all()
        bit = np.where(rel == 1, 0, np.where((rel >= 1 + n_u) & (rel <= 8 + n_u), 1 + rel - (1 + n_u), -1))
        sig = np.zeros(len(cps), dtype=np.int64)
        ok = bit >= 0
        np.bitwise_or.at(sig, doc_of_tok[ok], 1 << bit[ok])
        sig_of = lambda ch: int(sig[np.searchsorted(cps, ord(ch))])
        for x in ("N", "W", "LO"):
            for y in ("N", "W", "LO"):
                if x == y:
                    continue
                differs = np.ones(len(cps), dtype=bool)
                for ch in reps[y]:
                    differs &= sig != sig_of(ch)
                count = int((differs & (grp == x)).sum())
                print("%s: class %s taken for %s: visible for %d of %d code points" % (name, x, y, count, int((grp == x).sum())))
                assert count > 0, (name, x, y)
        for x, y, ch in (("L", "O", "€"), ("O", "L", "é")):
            print("%s: class %s taken for %s: boundaries among the ASCII characters differ for %d of %d code points (merges over c "
                  "aside)" % (name, x, y, int(((sig != sig_of(ch)) & (cls == x)).sum()), int((cls == x).sum())))
