"""k_piece_resolve's chunk passes (jtokkit_amd/csrc/jtk_kernels.hip) on the texts of resolve_cases.py -- tiles whose piece
counts stand on both sides of every pair-pass and single-pass edge, alone and between neighbours, pieces of 8, 9, 16 and 17
bytes at the first and last lane of each chunk of a pass, every queue bin one short of, at and one past what pack stages of it,
pieces of 300, 600 and 9,000 bytes and a gap piece in one chunk beside a chunk of ordinary pieces, and pieces that have to look
at their secondary table slot (test_resolve_cases_cpu.py checks that the texts hold all that).  Device encode against the CPU
oracle, bit-exact: tokens, offsets, status."""
import numpy as np
import pytest

import oracle_lib
import resolve_cases as rc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def jt():
    import jtokkit_amd
    return jtokkit_amd


@pytest.fixture(scope="module")
def g():
    return rc.Gen()


@pytest.fixture(scope="module")
def batch(jt):
    b = jt.get_encoding(rc.NAME).new_batch()
    yield b
    b.close()


def _run(b, case, count_too=False):
    import torch
    text, doc_off = case.text, case.doc_off
    exp_tok, exp_off = oracle_lib.get(rc.NAME).encode_batch(text, doc_off, threads=8)
    dev = torch.device("cuda:0")
    d_text = torch.from_numpy(np.concatenate([text, np.zeros(16, dtype=np.uint8)])).to(dev)
    d_off = torch.from_numpy(np.ascontiguousarray(doc_off, dtype=np.int64)).to(dev)
    torch.cuda.synchronize()
    b.encode_device(d_text.data_ptr(), d_off.data_ptr(), len(doc_off) - 1, len(text), ordinary=True)
    res = b.fetch()
    assert np.array_equal(res.tok_off, exp_off), (case.label, res.tok_off.tolist()[:4], exp_off.tolist()[:4])
    if not np.array_equal(res.tokens, exp_tok):
        j = int(np.nonzero(res.tokens != exp_tok)[0][0])
        raise AssertionError("%s: token %d: expected %s, got %s" % (case.label, j, exp_tok[j:j + 6].tolist(), res.tokens[j:j + 6].tolist()))
    assert not res.status.any()
    if count_too:
        b.encode_device(d_text.data_ptr(), d_off.data_ptr(), len(doc_off) - 1, len(text), ordinary=True, count_only=True)
        counts, status = b.fetch_counts()
        assert np.array_equal(counts, np.diff(exp_off)) and not status.any()


@pytest.mark.parametrize("n_pieces", rc.np_counts())
def test_one_tile_on_both_sides_of_every_pass_edge(batch, g, n_pieces):
    _run(batch, rc.one_tile(g, n_pieces))


def test_middle_tile_of_three_and_a_tile_inside_a_piece(batch, g):
    _run(batch, rc.middle_tiles(g), count_too=True)


def test_lengths_8_9_16_17_at_the_lanes_at_pass_edges(batch, g):
    _run(batch, rc.length_edges(g))


def test_every_bin_at_its_staging_edge(batch, g):
    _run(batch, rc.bin_edges(g), count_too=True)


def test_rare_kinds_beside_an_ordinary_chunk(batch, g):
    _run(batch, rc.rare_chunk(g))


def test_gap_piece_in_a_chunk_with_the_long_pieces(jt, g):
    """the caller's pattern leaves one ordinary piece of the second chunk out: a gap piece next to the 300-, 600- and 9,000-byte
    pieces; expected = the oracle's loop over the same matches"""
    case = rc.rare_chunk(g)
    ends = np.cumsum([len(p) for p in case.parts])
    begins = ends - np.array([len(p) for p in case.parts])
    keep = np.ones(len(begins), dtype=bool)
    keep[case.gap] = False
    pb, pe = begins[keep].astype(np.int64), ends[keep].astype(np.int64)
    b = jt.get_encoding(rc.NAME).new_batch()
    nt = b.encode_pieces(case.text, case.doc_off, pb, pe)
    res = b.fetch()
    exp = oracle_lib.get(rc.NAME).encode_pieces(case.text.tobytes(), pb, pe)
    assert nt == len(exp) and res.tokens.tolist() == exp and not res.status.any()
    whole = oracle_lib.get(rc.NAME).encode_ordinary(case.text.tobytes())
    assert len(exp) < len(whole)                                    # the gap piece gave no tokens
    b.close()


def test_pieces_that_read_their_secondary_slot(batch, g):
    import merge_cases
    sim = merge_cases.Sim(rc.NAME)
    sim.L.sim_tok8_bits.argtypes = [merge_cases.C.c_void_p]
    case = rc.secondary_case(g, sim.L.sim_tok8_bits(sim.h))
    print("entries that share a primary slot: %d (the first 1500 in the text); absent pieces that must read their secondary slot: %d"
          % (case.n_displaced, case.n_absent))
    assert case.n_displaced >= 2 and case.n_absent >= 1
    _run(batch, case)
