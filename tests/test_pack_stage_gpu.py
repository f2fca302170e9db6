"""k_pack_tokens' staging of merge results in LDS (jtokkit_amd/csrc/jtk_stage_rules.h): tiles with as many merged pieces per
bin as the staged heads hold, one fewer and one more, up to and past the end of the free room, the worst a tile can hold,
several bins overflowing together, token totals at the edge of the LDS assembly, results of exactly 7 and of more than 7
tokens in the extension, and documents that start on pieces of every kind (pack_stage_cases.py; test_pack_stage_cases_cpu.py
checks that the texts hold those counts).  Each text through Batch.encode_device with torch-owned buffers as a job of its own
(a small job: pack adds up the tiles itself), as a count-only job, and as the second chunk of a two-chunk job (tile scan by
its own kernel, the chunk's first document inside a tile) -- bit-exact against the CPU oracle."""
import numpy as np
import pytest

import oracle_lib
import pack_stage_cases as psc

pytestmark = pytest.mark.gpu

LABELS = ("cap", "room", "worst", "stage", "free", "counts", "docs")


@pytest.fixture(scope="module")
def jt():
    import jtokkit_amd
    return jtokkit_amd


@pytest.fixture(scope="module")
def built():
    """label -> base -> (text, doc_off, oracle tokens, oracle offsets); the counts are asserted before anything runs"""
    words = psc.Words()
    out = {}
    for label, (case, want) in psc.cases(words).items():
        out[label] = {}
        for base in (0, psc.SECOND_BASE):
            text, doc_off = psc.check_targets(words, case, want, base)
            out[label][base] = (text, doc_off) + tuple(oracle_lib.get(psc.NAME).encode_batch(text, doc_off, threads=8))
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
            d, doc_off[d], doc_off[d] // psc.T, doc_off[d] % psc.T, exp_off[d:d + 2].tolist(), got_off[d:d + 2].tolist())
    j = int(np.nonzero(exp_tok != got_tok)[0][0])
    d = int(np.searchsorted(exp_off, j, side="right")) - 1
    return "token %d (document %d, which starts in tile %d): expected %s, got %s" % (
        j, d, doc_off[d] // psc.T, exp_tok[j:j + 6].tolist(), got_tok[j:j + 6].tolist())


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
    b = jt.get_encoding(psc.NAME).new_batch()
    _run(b, built[label][0])
    b.close()


@pytest.mark.parametrize("label", LABELS)
def test_count_only(jt, built, label):
    b = jt.get_encoding(psc.NAME).new_batch()
    _run(b, built[label][0], count_only=True)
    _run(b, built[label][psc.SECOND_BASE], count_only=True)
    b.close()


@pytest.mark.parametrize("label", LABELS)
def test_second_chunk_of_two(jt, built, label):
    from jtokkit_amd import _native as N
    b = jt.get_encoding(psc.NAME).new_batch()
    b.set_option(N.JTK_OPT_CHUNK_BYTES, psc.CHUNK)
    item = built[label][psc.SECOND_BASE]
    assert psc.CHUNK < len(item[0]) <= 2 * psc.CHUNK and item[1][1] == psc.SECOND_BASE
    _run(b, item)
    _run(b, item, count_only=True)
    b.close()


def test_one_batch_object_through_every_case(jt, built):
    """All texts on one batch object, the crowded ones first: nothing of an earlier tile's extension is left for a later one."""
    b = jt.get_encoding(psc.NAME).new_batch()
    for label in ("worst", "cap", "room", "stage", "worst", "free", "counts", "docs", "cap"):
        _run(b, built[label][0])
    b.close()
