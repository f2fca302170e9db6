"""pretok_split's device glue on its structural edges: the cases of split_edge_cases.py (every construct at every shift
over block, wave and workgroup edges, after runs of every reach, in every document mode), text ends at every kind of
partial load, and every code point through the kernel's LDS copy of the class table -- all through
Batch.encode_device with torch-owned buffers, bit-exact against the CPU oracle.  test_split_edges_cpu.py proves the
shared headers on the same inputs, so a failure here points at the kernel's shuffles, halo lanes, LDS staging or
device-only instruction forms.
"""
import numpy as np
import pytest

import oracle_lib
import split_edge_cases as sec

pytestmark = pytest.mark.gpu

KIND = {"cl100k_base": 1, "r50k_base": 0}


@pytest.fixture(scope="module")
def jt():
    import jtokkit_amd
    return jtokkit_amd


_expected = {}


def _oracle(name, key, text, doc_off):
    """The oracle's (tokens, tok_off) of a generated batch, computed once per module run."""
    k = (name,) + key
    if k not in _expected:
        _expected[k] = oracle_lib.get(name).encode_batch(text, doc_off, threads=8)
    return _expected[k]


def _to_device(text, doc_off):
    """d_utf8 is 16-byte aligned (a torch allocation) and readable 16 bytes past the text, as the ABI asks."""
    import torch
    dev = torch.device("cuda:0")
    d_text = torch.from_numpy(np.concatenate([text, np.zeros(16, dtype=np.uint8)])).to(dev)
    d_off = torch.from_numpy(np.ascontiguousarray(doc_off, dtype=np.int64)).to(dev)
    assert d_text.data_ptr() % 16 == 0
    torch.cuda.synchronize()
    return d_text, d_off


def _encode(b, text, doc_off, ordinary=True):
    d_text, d_off = _to_device(text, doc_off)
    b.encode_device(d_text.data_ptr(), d_off.data_ptr(), len(doc_off) - 1, len(text), ordinary=ordinary)
    return b.fetch()


def _where(name, exp_tok, exp_off, got_tok, got_off, doc_off, label_of):
    """First differing document, its label and the byte position of its first differing token."""
    n_docs = len(doc_off) - 1
    for d in range(n_docs):
        e = exp_tok[exp_off[d]:exp_off[d + 1]]
        g = got_tok[got_off[d]:got_off[d + 1]] if d + 1 < len(got_off) else got_tok[:0]
        if len(e) == len(g) and np.array_equal(e, g):
            continue
        j = 0
        while j < min(len(e), len(g)) and e[j] == g[j]:
            j += 1
        p = int(doc_off[d]) + len(oracle_lib.get(name).decode_bytes(e[:j]))
        return ("document %d [%s]: token %d differs at byte %d (mod 64: %d, mod 3968: %d, mod 31744: %d); expected %s, got %s"
                % (d, label_of(p), j, p, p % 64, p % 3968, p % 31744, e[j:j + 4].tolist(), g[j:j + 4].tolist()))
    return "no document differs (offsets only)"


def _check(name, res, exp, doc_off, label_of, what):
    exp_tok, exp_off = exp
    same = (np.array_equal(res.tok_off, exp_off) and np.array_equal(res.tokens, exp_tok))
    assert same, "%s %s: %s" % (name, what, _where(name, exp_tok, exp_off, res.tokens, res.tok_off, doc_off, label_of))
    assert np.array_equal(res.status, np.zeros(len(doc_off) - 1, dtype=np.int32)), (name, what)


def _run_chain(b, name, key, chain, mode):
    text, doc_off, _ = chain.batch(mode)
    res = _encode(b, text, doc_off)
    _check(name, res, _oracle(name, key + (mode,), text, doc_off), doc_off, chain.label_at, "%s mode %s" % (key, mode))
    return res


@pytest.mark.parametrize("name", ["cl100k_base", "r50k_base"])
def test_wave_and_workgroup_edges(jt, name):
    """Every construct at every shift over 3,968-byte wave edges (every 8th a 31,744-byte workgroup edge) after every
    context: as one document, as a document per segment, and with a document boundary at edge - 1, edge, edge + 1."""
    enc = jt.get_encoding(name)
    b = enc.new_batch()
    for i, chain in enumerate(sec.wave_chains(KIND[name])):
        for mode in ("a", "b"):
            _run_chain(b, name, ("wave", i), chain, mode)
    for i, chain in enumerate(sec.beyond_chains(KIND[name])):   # runs over a whole wave and the block before it
        for mode in ("a", "b"):
            _run_chain(b, name, ("beyond", i), chain, mode)
    for i, chain in enumerate(sec.mode_c_chains(KIND[name])):
        for mode in ("c-1", "c0", "c+1"):
            _run_chain(b, name, ("mode-c", i), chain, mode)
    b.close()


@pytest.mark.parametrize("name", ["cl100k_base", "r50k_base"])
def test_full_span_runs_of_one_piece(jt, name):
    """Every construct at every shift after a full-span run of every context type that is ONE 3,968-byte piece, a document per
    segment (as one document the oracle's quadratic bytePairMerge would take 20 s: split_edge_cases.CHEAP_FULL)."""
    enc = jt.get_encoding(name)
    b = enc.new_batch()
    for i, chain in enumerate(sec.full_span_chains(KIND[name])):
        _run_chain(b, name, ("full-span", i), chain, "b")
    b.close()


@pytest.mark.parametrize("name", ["cl100k_base", "r50k_base"])
def test_block_edges(jt, name):
    """The same constructs and shifts on 64-byte edges inside a wave (192-byte stride): the in-wave shuffle carries."""
    enc = jt.get_encoding(name)
    b = enc.new_batch()
    chain = sec.block_chain(KIND[name])
    for mode in ("a", "b"):
        _run_chain(b, name, ("block",), chain, mode)
    b.close()


def _has_literal(name, doc):
    return any(lit.encode() in doc for lit in oracle_lib.ENCODINGS[name]["specials"])


def _check_encode_path(name, res, text, doc_off, label_of, what):
    """encode(): status -2 exactly for the documents that hold a whole literal; the others' tokens equal the oracle."""
    raw = text.tobytes()
    n_docs = len(doc_off) - 1
    exp_status = np.array([-2 if _has_literal(name, raw[doc_off[d]:doc_off[d + 1]]) else 0 for d in range(n_docs)], dtype=np.int32)
    assert np.array_equal(res.status, exp_status), (what, np.nonzero(res.status != exp_status)[0][:8].tolist(),
                                                    [label_of(int(doc_off[d])) for d in np.nonzero(res.status != exp_status)[0][:3]])
    exp_tok, exp_off = oracle_lib.get(name).encode_batch(text, doc_off, threads=8, ordinary=True)
    for d in np.nonzero(exp_status == 0)[0]:
        e = exp_tok[exp_off[d]:exp_off[d + 1]]
        g = res.tokens[res.tok_off[d]:res.tok_off[d + 1]]
        assert np.array_equal(e, g), (what, int(d), label_of(int(doc_off[d + 1])), int(doc_off[d]) % 3968, e[:8].tolist(), g[:8].tolist())
    return exp_status


def test_encode_path_specials_at_edges(jt):
    """special_check_at beside wave edges: <|endoftext|>, <|fim_prefix|> and <|endofprompt|> (and cut look-alikes) at every
    shift over an edge on which a document starts, so a literal cut by the edge is in no document."""
    name = "cl100k_base"
    enc = jt.get_encoding(name)
    b = enc.new_batch()
    chain = sec.special_chain()
    text, doc_off, _ = chain.batch("b")
    res = _encode(b, text, doc_off, ordinary=False)
    st = _check_encode_path(name, res, text, doc_off, chain.label_at, "specials")
    assert (st == -2).sum() >= 3 * 2 and (st == 0).sum() >= 3 * 10           # both kinds of placement are present
    b.close()


def test_text_tails(jt):
    """Texts that end 1 byte around block, wave, workgroup and two-workgroup sizes, on one batch object, longest first:
    the `valid` mask, the partial 16-byte loads, special_check_at at the very end, and no stale mask word of the
    longer text before."""
    name = "cl100k_base"
    enc = jt.get_encoding(name)
    b = enc.new_batch()
    for label, text, doc_off in sec.text_tails():
        res = _encode(b, text, doc_off, ordinary=False)
        st = _check_encode_path(name, res, text, doc_off, lambda p: label, label)
        assert st[0] == (-2 if "whole-literal" in label else 0), label
    b.close()


@pytest.mark.parametrize("name", ["cl100k_base", "r50k_base"])
def test_every_code_point_on_the_device(jt, name):
    """Every code point through the kernel's class-table copy in LDS: one probe document each (split_edge_cases.probe);
    cl100k a second time on the same batch object."""
    enc = jt.get_encoding(name)
    b = enc.new_batch()
    text, doc_off, cps = sec.every_codepoint_docs()
    exp = _oracle(name, ("probes",), text, doc_off)
    for rep in range(2 if name == "cl100k_base" else 1):
        res = _encode(b, text, doc_off)
        _check(name, res, exp, doc_off, lambda p: "U+%04X" % cps[np.searchsorted(doc_off, p, side="right") - 1], "probes run %d" % rep)
    b.close()


def test_same_result_on_repeat(jt):
    """The main cl100k sweep three times while a second batch object encodes the mixed corpus on its own stream: the
    table copy that races between waves and the fixed-point loop must not depend on timing."""
    import torch
    from jtokkit_amd import corpus
    name = "cl100k_base"
    enc = jt.get_encoding(name)
    b, other = enc.new_batch(), enc.new_batch()
    mt, moff = corpus.mixed(900, seed=72)
    d_mt, d_moff = _to_device(mt, moff)
    for i, chain in enumerate(sec.wave_chains(1)):
        text, doc_off, _ = chain.batch("a")
        d_text, d_off = _to_device(text, doc_off)
        first = None
        for rep in range(3):
            other.encode_device(d_mt.data_ptr(), d_moff.data_ptr(), len(moff) - 1, len(mt), ordinary=True, sync=False)
            b.encode_device(d_text.data_ptr(), d_off.data_ptr(), len(doc_off) - 1, len(text), ordinary=True)
            res = b.fetch()
            if first is None:
                first = res
                _check(name, res, _oracle(name, ("wave", i, "a"), text, doc_off), doc_off, chain.label_at, "repeat chain %d" % i)
            else:
                assert np.array_equal(res.tok_off, first.tok_off) and np.array_equal(res.tokens, first.tokens), (i, rep)
        mixed = other.fetch()
    exp = oracle_lib.get(name).encode_batch(mt, moff, threads=8)
    assert np.array_equal(mixed.tokens, exp[0]) and np.array_equal(mixed.tok_off, exp[1])
    torch.cuda.synchronize()
    b.close()
    other.close()
