"""k_piece_resolve around its probe loop (jtokkit_amd/csrc/jtk_kernels.hip) on the texts of resolve_list_cases.py: mask words
with 0, 1, 63 and 64 piece starts, starts at bit 0 and bit 63 of a word and in a tile's first and last word, tiles whose pieces
all lie in one word of each wave, a tile inside one piece, a text that ends in mid-word, a second chunk that starts in mid-tile;
and tiles whose misses fill none, one, 63 or all lanes of a chunk, both chunks of a pair pass, lanes 0 and 63 only, only a
single pass, only wave 3's chunks, 64 and 65 queued pieces, and as many as 3- and 4-byte pieces allow
(test_resolve_list_cases_cpu.py checks that the texts hold all that; every bin one short of, at and one past what pack stages
is test_resolve_passes_gpu.py's).  Device encode against the CPU oracle, bit-exact: tokens, offsets, status."""
import numpy as np
import pytest

import oracle_lib
import resolve_cases as rc
import resolve_list_cases as lc

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
    b = jt.get_encoding(lc.NAME).new_batch()
    yield b
    b.close()


def _run(b, case, count_too=False):
    import torch
    text, doc_off = case.text, case.doc_off
    exp_tok, exp_off = oracle_lib.get(lc.NAME).encode_batch(text, doc_off, threads=8)
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


def test_mask_words_of_0_1_63_and_64_starts(batch, g):
    _run(batch, lc.word_shapes(g), count_too=True)


def test_all_pieces_in_one_word_of_each_wave_and_a_tile_inside_a_piece(batch, g):
    _run(batch, lc.one_word_tiles(g), count_too=True)


def test_second_chunk_starts_in_mid_tile(jt, g):
    from jtokkit_amd import _native as N
    case = lc.second_chunk(g)
    b = jt.get_encoding(lc.NAME).new_batch()
    b.set_option(N.JTK_OPT_CHUNK_BYTES, lc.CHUNK)
    assert lc.CHUNK < len(case.text) <= 2 * lc.CHUNK and case.doc_off[1] == lc.SECOND_BASE
    _run(b, case, count_too=True)
    b.close()


@pytest.mark.parametrize("label", sorted(lc.MISS_TILES))
def test_misses(batch, g, label):
    _run(batch, lc.miss_case(g, label))


def test_miss_tiles_side_by_side(batch, g):
    """all of them in one text, a tile each: what one tile leaves in LDS or claims of a queue is not the next one's"""
    parts = [p for label in sorted(lc.MISS_TILES) for p in lc.miss_case(g, label).parts]
    _run(batch, lc.Case("side_by_side", parts), count_too=True)
