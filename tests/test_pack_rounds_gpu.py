"""k_pack_tokens' steps and rounds (pack_round_cases.py; test_pack_round_cases_cpu.py checks that the texts hold what they
say): every piece count at a step and round edge in a tile assembled in LDS and in a tile written directly, 767 / 768 / 769
tokens on both sides of a step edge, hard pieces of 2, 3, 4, 7 and more than 7 tokens in the first and last lane of the first
and last step of a round and of the second round's first step, general-path steps beside common ones in both orders, tiny
pieces across step edges and beyond their staging area, document starts at the step and round edges with tiles without any in
between.  Each text through Batch.encode_device as a job of its own (a small job: pack adds up the tiles itself), as a
count-only job, and as the second chunk of a two-chunk job -- bit-exact against the CPU oracle."""
import numpy as np
import pytest

import oracle_lib
import pack_round_cases as prc
import pack_stage_cases as psc

pytestmark = pytest.mark.gpu

LABELS = ("counts_small_staged", "counts_round_staged", "counts_small_direct", "counts_round_direct", "counts_big", "edge_512",
          "edge_576", "lanes_staged", "lanes_direct", "general", "tiny", "docs")


@pytest.fixture(scope="module")
def jt():
    import jtokkit_amd
    return jtokkit_amd


@pytest.fixture(scope="module")
def built():
    """label -> base -> (text, doc_off, oracle tokens, oracle offsets); the counts are asserted before anything runs"""
    words = psc.Words()
    out = {}
    for txt in prc.texts(words):
        out[txt.label] = {}
        for base in (0, prc.SECOND_BASE):
            text, doc_off = prc.check(words, txt, base)
            out[txt.label][base] = (text, doc_off) + tuple(oracle_lib.get(prc.NAME).encode_batch(text, doc_off, threads=8))
    assert set(out) == set(LABELS)
    return out


def _to_device(text, doc_off):
    import torch
    dev = torch.device("cuda:0")
    d_text = torch.from_numpy(np.concatenate([text, np.zeros(16, dtype=np.uint8)])).to(dev)
    d_off = torch.from_numpy(np.ascontiguousarray(doc_off, dtype=np.int64)).to(dev)
    assert d_text.data_ptr() % 16 == 0
    torch.cuda.synchronize()
    return d_text, d_off


def _first_difference(exp_tok, exp_off, got_tok, got_off, doc_off):
    if not np.array_equal(exp_off, got_off):
        d = int(np.nonzero(exp_off != got_off)[0][0]) if len(exp_off) == len(got_off) else -1
        return "offset of document %d (starts at byte %d, tile %d, byte %d of it): expected %s, got %s" % (
            d, doc_off[d], doc_off[d] // prc.T, doc_off[d] % prc.T, exp_off[d:d + 2].tolist(), got_off[d:d + 2].tolist())
    if len(exp_tok) != len(got_tok):
        return "%d tokens expected, got %d" % (len(exp_tok), len(got_tok))
    j = int(np.nonzero(exp_tok != got_tok)[0][0])
    d = int(np.searchsorted(exp_off, j, side="right")) - 1
    return "token %d (document %d, which starts in tile %d): expected %s, got %s" % (
        j, d, doc_off[d] // prc.T, exp_tok[j:j + 6].tolist(), got_tok[j:j + 6].tolist())


def _run(b, item, count_only=False):
    text, doc_off, exp_tok, exp_off = item
    d_text, d_off = _to_device(text, doc_off)
    b.encode_device(d_text.data_ptr(), d_off.data_ptr(), len(doc_off) - 1, len(text), ordinary=True, count_only=count_only)
    if count_only:
        counts, status = b.fetch_counts()
        assert np.array_equal(counts, np.diff(exp_off)), np.nonzero(counts != np.diff(exp_off))[0][:8].tolist()
    else:
        res = b.fetch()
        status = res.status
        same = np.array_equal(res.tok_off, exp_off) and np.array_equal(res.tokens, exp_tok)
        assert same, _first_difference(exp_tok, exp_off, res.tokens, res.tok_off, doc_off)
    assert not status.any()


@pytest.mark.parametrize("label", LABELS)
def test_small_job(jt, built, label):
    b = jt.get_encoding(prc.NAME).new_batch()
    _run(b, built[label][0])
    b.close()


@pytest.mark.parametrize("label", LABELS)
def test_count_only(jt, built, label):
    b = jt.get_encoding(prc.NAME).new_batch()
    _run(b, built[label][0], count_only=True)
    _run(b, built[label][prc.SECOND_BASE], count_only=True)
    b.close()


@pytest.mark.parametrize("label", LABELS)
def test_second_chunk_of_two(jt, built, label):
    from jtokkit_amd import _native as N
    b = jt.get_encoding(prc.NAME).new_batch()
    b.set_option(N.JTK_OPT_CHUNK_BYTES, prc.CHUNK)
    item = built[label][prc.SECOND_BASE]
    assert prc.CHUNK < len(item[0]) <= 2 * prc.CHUNK and item[1][1] == prc.SECOND_BASE
    _run(b, item)
    _run(b, item, count_only=True)
    b.close()


def test_one_batch_object_through_every_text(jt, built):
    """All texts on one batch object: nothing that a tile left in LDS or in the lists is there for a later one."""
    b = jt.get_encoding(prc.NAME).new_batch()
    for label in LABELS + ("counts_big", "counts_small_staged"):
        _run(b, built[label][0])
    b.close()
