"""CPU tier of the fill-in-the-middle encode (JTK_ENCODE_FIM): the rule header jtokkit_amd/csrc/jtk_fim_rules.h -- run serially
through the shim tests/fim_sim the way the kernels partition the work -- against the plain restatement tests/fim_ref.py on
every case of tests/fim_cases.py.  kind, cut, sub_off and the stitched ids are compared exactly (segment ids come from the CPU
oracle's encode_ordinary); the draws are checked for the shard property, the rates and the uniformity of the cuts against
bounds derived from the binomial distribution; and a stand-alone sanitizer build of the shim runs every case in buffers of
exactly the arrays' sizes.  No GPU."""
import ctypes as C
import math
import os
import struct
import subprocess

import numpy as np
import pytest

import fim_cases as fc
import fim_ref as fr
import oracle_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIM_DIR = os.path.join(ROOT, "tests", "fim_sim")
IDS = (100258, 100259, 100260)               # cl100k_base's <|fim_prefix|>, <|fim_middle|>, <|fim_suffix|>
_REF, _CASES = {}, {}


def oracle_encode(doc):
    """Segment ids from the CPU oracle.  It takes well-formed text only; an ill-formed part stands as one made-up id per byte,
    the same in the restatement and in what the shim stitches -- neither looks inside a part's ids."""
    if not fr.well_formed(doc):
        return [200000 + x for x in doc]
    return oracle_lib.get("cl100k_base").encode_ordinary(doc)


def all_cases():
    if not _CASES:
        count = lambda b: len(oracle_encode(b))
        for c in fc.cases() + fc.gather_edge_cases(count) + [fc.tiny_documents(), fc.zero_token_parts_at_tile_starts()]:
            _CASES[c.name] = c
    return _CASES


CASE_NAMES = [c.name for c in fc.cases()] + ["gather_%s_%d_%s" % (s, c, m) for s in ("suf", "mid") for c in (fc.TILE - 1, fc.TILE)
                                             for m in ("psm", "spm")] + ["tiny_documents", "zero_token_parts_at_tile_starts"]


def ref(case):
    """The reference's result for a case, computed once."""
    if case.name not in _REF:
        _REF[case.name] = fr.encode_batch(oracle_encode, case.docs, case.seed, case.base, case.fim_rate, case.spm_rate, IDS)
    return _REF[case.name]


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("fim_sim") / "libfim_sim.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas", "-o", out,
                           os.path.join(SIM_DIR, "fim_sim.cpp")])
    L = C.CDLL(out)
    L.sim_fim_cuts.restype = C.c_int
    L.sim_fim_cuts.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_uint64, C.c_int64, C.c_uint32, C.c_uint32, C.c_void_p,
                               C.c_void_p, C.c_void_p]
    L.sim_fim_stitch.restype = C.c_int64
    L.sim_fim_stitch.argtypes = [C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int,
                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return L


def pack(docs):
    doc_off = np.zeros(len(docs) + 1, dtype=np.int64)
    if docs:
        np.cumsum([len(x) for x in docs], out=doc_off[1:])
    return np.frombuffer(b"".join(docs) + b"\0", dtype=np.uint8), doc_off      # (one spare byte: an address for an empty text)


def sim_cuts(sim, docs, seed, base, fim_rate, spm_rate, doc_off=None):
    text, off = pack(docs)
    if doc_off is not None:
        off = np.ascontiguousarray(doc_off, dtype=np.int64)
    n = len(off) - 1
    kind, cut, sub_off = np.full(max(n, 1), 9, dtype=np.uint8), np.full((max(n, 1), 2), -7, dtype=np.int64), np.full(3 * n + 1, -7, dtype=np.int64)
    bad = sim.sim_fim_cuts(text.ctypes.data, off.ctypes.data, n, len(text) - 1, seed, base, fim_rate, spm_rate, kind.ctypes.data,
                           cut.ctypes.data, sub_off.ctypes.data)
    return bad, kind[:n], cut[:n], sub_off


def encode_subs(docs, sub_off, encode=oracle_encode):
    """The pipeline's result on the sub-documents, by the oracle: (sub_tok_off, sub_status, sub_tokens)."""
    text = b"".join(docs)
    toks, off, status = [], [0], []
    for j in range(len(sub_off) - 1):
        t = encode(text[sub_off[j]:sub_off[j + 1]])
        if not isinstance(t, list):
            status.append(t)
            t = [7] * int(sub_off[j + 1] - sub_off[j])                 # (a refused sub-document still has tokens: they must not be used)
        else:
            status.append(0)
        toks += t
        off.append(len(toks))
    return np.array(off, dtype=np.int64), np.array(status + [0], dtype=np.int32), np.array(toks + [0], dtype=np.int32)


def sim_stitch(sim, n, kind, subs, n_blocks=2, bad=0, count_only=False):
    sub_tok_off, sub_status, sub_tokens = subs
    status, part, tok_off = np.full(max(n, 1), -7, dtype=np.int32), np.full((max(n, 1), 3), -7, dtype=np.int64), np.full(n + 1, -7, dtype=np.int64)
    tokens = np.full(len(sub_tokens) + 3 * n + 1, -7, dtype=np.int32)
    kind = np.ascontiguousarray(kind if n else np.zeros(1, dtype=np.uint8))
    total = sim.sim_fim_stitch(n, bad, kind.ctypes.data, sub_tok_off.ctypes.data, sub_status.ctypes.data, sub_tokens.ctypes.data, IDS[0], IDS[1],
                               IDS[2], n_blocks, status.ctypes.data, part.ctypes.data, tok_off.ctypes.data, None if count_only else tokens.ctypes.data)
    assert (tokens[total:] == -7).all()
    return status[:n], part[:n], tok_off, tokens[:total]


def test_the_shim_uses_the_tile_the_cases_are_built_for(sim):
    assert sim.sim_fim_tile() == fc.TILE


def test_case_names_are_the_case_set():
    assert list(all_cases()) == CASE_NAMES


@pytest.mark.parametrize("name", CASE_NAMES)
def test_rule_header_equals_the_restatement(sim, name):
    case = all_cases()[name]
    exp = ref(case)
    n = len(case.docs)
    bad, kind, cut, sub_off = sim_cuts(sim, case.docs, case.seed, case.base, case.fim_rate, case.spm_rate)
    assert bad == 0
    assert np.array_equal(kind, exp.kind), (name, np.flatnonzero(kind != exp.kind)[:10])
    assert np.array_equal(cut, exp.cut), (name, np.flatnonzero((cut != exp.cut).any(axis=1))[:10])
    assert np.array_equal(sub_off, exp.sub_off)
    subs = encode_subs(case.docs, sub_off)
    for n_blocks in (1, 2, 5):
        status, part, tok_off, tokens = sim_stitch(sim, n, kind, subs, n_blocks)
        assert np.array_equal(status, exp.status) and np.array_equal(part, exp.part_tok)
        assert np.array_equal(tok_off, exp.tok_off)
        assert np.array_equal(tokens, exp.tokens), (name, n_blocks, np.flatnonzero(tokens != exp.tokens)[:10])
    counts = sim_stitch(sim, n, kind, subs, count_only=True)
    assert np.array_equal(counts[2], exp.tok_off) and len(counts[3]) == len(exp.tokens)


def test_case_set_reaches_the_edges():
    reached = set()
    for case in all_cases().values():
        reached |= fc.edges_reached(case)
    assert fc.ALL_EDGES - reached == set()
    # a four-byte character is cut before or after it, never inside
    case = all_cases()["one_four_byte_character"]
    assert set(ref(case).cut.ravel().tolist()) == {0, 4}
    # the gather cases put each sentinel on either side of a tile boundary, in a document that crosses it
    for s, which in (("suf", 2), ("mid", 1)):
        for cell in (fc.TILE - 1, fc.TILE):
            for m in ("psm", "spm"):
                r = ref(all_cases()["gather_%s_%d_%s" % (s, cell, m)])
                assert r.tokens[cell] == IDS[which]
                d = int(np.searchsorted(r.tok_off, cell, side="right")) - 1
                assert r.tok_off[d] < fc.TILE < r.tok_off[d + 1] - 1          # (cells on both sides of the boundary)
    r = ref(all_cases()["zero_token_parts_at_tile_starts"])
    sent = fc.sentinel_cells(r, IDS)
    assert sum(1 for t in range(fc.TILE, len(sent), fc.TILE) if sent[t] and sent[t - 1]) >= 2
    r = ref(all_cases()["tiny_documents"])
    assert len(r.tokens) > 8 * fc.TILE and np.diff(r.tok_off).max() <= 8


def test_a_refused_part_refuses_the_document_and_no_other(sim):
    """The lowest of the three statuses; a document with a negative status has no tokens; its neighbours are unaffected."""
    docs = [b"hello world", b"the unencodable Q here", b"fine again"] * 12

    def encode(b):
        return -12 if b"Q" in b else oracle_encode(b)
    exp = fr.encode_batch(encode, docs, 31, 0, fr.ALWAYS, fc.HALF, IDS)
    bad, kind, cut, sub_off = sim_cuts(sim, docs, 31, 0, fr.ALWAYS, fc.HALF)
    status, part, tok_off, tokens = sim_stitch(sim, len(docs), kind, encode_subs(docs, sub_off, encode))
    assert status.tolist() == [0, -12, 0] * 12 and np.array_equal(status, exp.status)
    assert np.array_equal(part, exp.part_tok) and np.array_equal(tok_off, exp.tok_off) and np.array_equal(tokens, exp.tokens)
    # the Q lands in each of the three parts somewhere in the set
    where = {int(np.searchsorted(cut[d], docs[d].index(b"Q"), side="right")) for d in range(1, len(docs), 3)}
    assert where == {0, 1, 2}


def test_bad_offsets_are_reported_and_never_followed(sim):
    docs = [b"hello", b"world", b"again"]
    for off in ([0, 5, 4, 15], [0, 5, 10, 99], [1, 5, 10, 15], [0, -1, 10, 15], [0, 5, 10, 14]):
        bad, kind, cut, sub_off = sim_cuts(sim, docs, 1, 0, fr.ALWAYS, 0, doc_off=off)
        assert bad == 1
        # the sub-documents are bad where the documents are: what the pipeline's own check reports
        assert sub_off[0::3].tolist() == off
        n = 3
        subs = (np.arange(3 * n + 1, dtype=np.int64) * 2, np.zeros(3 * n + 1, dtype=np.int32), np.zeros(6 * n + 1, dtype=np.int32))
        status, part, tok_off, tokens = sim_stitch(sim, n, kind, subs, bad=1)
        assert tok_off.tolist() == [0] * 4 and len(tokens) == 0 and not part.any()


def test_shard_property(sim):
    """Documents [k, n) with doc_index_base = k give the same per-document results as the whole batch."""
    docs = fc.MIXED * 4
    whole = sim_cuts(sim, docs, 77, 1000, fc.HALF, fc.HALF)
    for k in (1, 7, len(docs) - 1):
        part = sim_cuts(sim, docs[k:], 77, 1000 + k, fc.HALF, fc.HALF)
        assert np.array_equal(part[1], whole[1][k:]) and np.array_equal(part[2], whole[2][k:])
        r_whole = fr.encode_batch(lambda b: [len(b)], docs, 77, 1000, fc.HALF, fc.HALF, IDS)
        r_part = fr.encode_batch(lambda b: [len(b)], docs[k:], 77, 1000 + k, fc.HALF, fc.HALF, IDS)
        assert r_part.docs == r_whole.docs[k:]
    assert len(set(whole[1].tolist())) == 3


N_DRAWS = 100000


def test_rates(sim):
    """fim_rate = spm_rate = 2^31 over 100,000 one-character documents: the transformed count is binomial(n, 1/2), sigma =
    sqrt(n / 4) = 158, and lies within 6 sigma = 949 of n / 2; the SPM count among the m transformed ones is binomial(m, 1/2) and
    lies within 6 sqrt(m / 4) of m / 2."""
    _, kind, _, _ = sim_cuts(sim, [b"x"] * N_DRAWS, 2024, 0, fc.HALF, fc.HALF)
    m = int((kind != 0).sum())
    assert abs(m - N_DRAWS / 2) <= 6 * math.sqrt(N_DRAWS / 4)
    assert abs(int((kind == 2).sum()) - m / 2) <= 6 * math.sqrt(m / 4)
    assert [fr.kind_of(2024, g, 1, fc.HALF, fc.HALF) for g in range(2000)] == kind[:2000].tolist()


def test_cut_uniformity(sim):
    """A 9-byte ASCII document over 100,000 global indices: each of the 10 values of p_0 is binomial(n, 1/10), sigma =
    sqrt(n * 0.1 * 0.9) = 95, and occurs within 6 sigma of n / 10.  p_0 itself is not a result (the results are the lower and
    the higher cut), so the restatement's draw gives it -- and the shim's cuts must be the sorted pair of the two draws."""
    doc = b"abcdefghi"
    _, kind, cut, _ = sim_cuts(sim, [doc] * N_DRAWS, 99, 0, fr.ALWAYS, 0)
    p0 = np.array([fr.raw_cut(99, g, 0, 9) for g in range(N_DRAWS)])
    p1 = np.array([fr.raw_cut(99, g, 1, 9) for g in range(N_DRAWS)])
    assert np.array_equal(cut[:, 0], np.minimum(p0, p1)) and np.array_equal(cut[:, 1], np.maximum(p0, p1))
    sigma = math.sqrt(N_DRAWS * 0.1 * 0.9)
    for name, p in (("p0", p0), ("p1", p1)):
        hist = np.bincount(p, minlength=10)
        assert len(hist) == 10 and np.abs(hist - N_DRAWS / 10).max() <= 6 * sigma, (name, hist)


def test_reference_on_hand_computed_values():
    """The restatement itself, on values small enough to check by hand."""
    assert fr.mix(0) == 0 and fr.mix(0x9E3779B97F4A7C15) == 0xE220A8397B1DCDAF       # splitmix64's first output from state 0
    assert fr.rate_u32(0.0) == 0 and fr.rate_u32(0.5) == 1 << 31 and fr.rate_u32(1.0) == 0xFFFFFFFF
    assert fr.snap(b"a\xe6\x97\xa5b", 3) == 1 and fr.snap(b"a\xe6\x97\xa5b", 4) == 4 and fr.snap(b"\x80\x80", 1) == 0
    assert fr.snap(b"\x80" * 8, 7) == 4 and fr.snap(b"\x80" * 8, 8) == 8 and fr.snap(b"\x80" * 8, 0) == 0
    enc = lambda b: list(b)
    assert fr.encode_doc(enc, b"abcde", fr.PSM, 1, 3, (-1, -2, -3)) == (0, [-1, 97, -3, 100, 101, -2, 98, 99], (1, 2, 2))
    assert fr.encode_doc(enc, b"abcde", fr.SPM, 1, 3, (-1, -2, -3)) == (0, [-1, -3, 100, 101, -2, 97, 98, 99], (1, 2, 2))
    assert fr.encode_doc(enc, b"abcde", fr.NONE, 5, 5, (-1, -2, -3)) == (0, [97, 98, 99, 100, 101], (5, 0, 0))
    assert fr.encode_doc(enc, b"ab\xff", fr.PSM, 1, 2, (-1, -2, -3), validate=True) == (-6, [], (0, 0, 0))


def test_sanitizer_build_runs_every_case_in_exact_buffers(tmp_path):
    exe = str(tmp_path / "fim_sim_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, os.path.join(SIM_DIR, "fim_sim_main.cpp")])
    cases, results = str(tmp_path / "cases.bin"), str(tmp_path / "results.bin")
    todo = list(all_cases().values())
    with open(cases, "wb") as f:
        for c in todo:
            exp = ref(c)
            sub_tok_off, sub_status, sub_tokens = encode_subs(c.docs, exp.sub_off)
            text, doc_off = pack(c.docs)
            f.write(struct.pack("<3qQ6q", len(c.docs), len(text) - 1, len(sub_tokens) - 1, c.seed, c.base, c.fim_rate, c.spm_rate, *IDS))
            f.write(doc_off.astype("<i8").tobytes())
            f.write(text[:-1].tobytes())
            f.write(sub_tok_off.astype("<i8").tobytes())
            f.write(sub_status[:-1].astype("<i4").tobytes())
            f.write(sub_tokens[:-1].astype("<i4").tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe, cases, results], env=env, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-4000:]
    assert p.stdout.strip() == "%d cases" % len(todo)
    raw = open(results, "rb").read()
    at = 0
    for c in todo:
        n = len(c.docs)
        exp = ref(c)
        for e, dt in ((exp.kind, "u1"), (exp.cut, "<i8"), (exp.sub_off, "<i8"), (exp.status, "<i4"), (exp.part_tok, "<i8"),
                      (exp.tok_off, "<i8"), (exp.tokens, "<i4")):
            got = np.frombuffer(raw, dtype=dt, count=e.size, offset=at)
            at += got.nbytes
            assert np.array_equal(got, e.ravel()), c.name
    assert at == len(raw)


def test_abi_refuses_null_arguments():
    """What the FIM entry points refuse before they touch a device."""
    so = os.path.join(ROOT, "jtokkit_amd", "libjtokkit_amd.so")
    if not os.path.exists(so):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "jtokkit_amd", "csrc")])
    from jtokkit_amd import _native as N
    L = N.lib()
    p = N.FimParamsStruct(1, 0, 1 << 31, 1 << 31, 100258, 100259, 100260)
    assert L.jtk_batch_set_fim(None, C.byref(p)) == N.JTK_ERR_INVALID_ARGUMENT
    assert L.jtk_batch_set_fim(None, None) == N.JTK_ERR_INVALID_ARGUMENT
    a, b, c = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert L.jtk_batch_fim_result(None, C.byref(a), C.byref(b), C.byref(c)) == N.JTK_ERR_INVALID_ARGUMENT
    assert L.jtk_batch_fim_result_fetch(None, None, None, None) == N.JTK_ERR_INVALID_ARGUMENT
    assert N.JTK_ENCODE_FIM == 64 and C.sizeof(N.FimParamsStruct) == 40
    import jtokkit_amd
    assert jtokkit_amd.encoding.fim_rate_u32(0.5) == 1 << 31 and jtokkit_amd.encoding.fim_rate_u32(1.0) == 0xFFFFFFFF
    with pytest.raises(ValueError):
        jtokkit_amd.FimParams(1.5)
