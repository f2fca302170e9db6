"""The early exit of the lean merge steps (lean_steps in jtk_kernels.hip: a step whose lookups no lane wants is finished without
them and leaves the loop) against the CPU oracle, bit-exact over all documents, tokens and offsets, on the texts of
merge_exit_cases.py: for each of the 8-, 12-, 16-, 32- and 64-slot instantiations waves in which the exit is taken, in which one
lane keeps it from being taken (side 1, side 2, both; first, middle, last), in which one lane runs on and takes it later, which
end with a wanted lookup, table entries that merge down to one token, and a wave with idle lanes -- once one wave per shard (the
bins of a shard side by side, one workgroup each), once in a shard just long enough for all four of its workgroups to take a
slice; and for the 4..8-byte bin in windows of 2 and 4 rounds at their thresholds.  test_merge_exit_cases_cpu.py asserts on the
CPU that the texts hold these waves.  Every tile is a document, as in test_merge_order_gpu.py."""
import numpy as np
import pytest

import merge_exit_cases as mx
import oracle_lib

pytestmark = pytest.mark.gpu

_cache = {}


def _plan():
    if "plan" not in _cache:
        _cache["plan"] = mx.Plan()
    return _cache["plan"]


def _item(kind, arg):
    """(text, oracle tokens, oracle offsets), built once"""
    if (kind, arg) not in _cache:
        t = getattr(_plan(), kind)(arg)
        _cache[(kind, arg)] = (t,) + tuple(oracle_lib.get(mx.NAME).encode_batch(t.text, t.doc_off, threads=8))
    return _cache[(kind, arg)]


def _run(b, item, count_only=False):
    import torch
    t, exp_tok, exp_off = item
    dev = torch.device("cuda:0")
    d_text = torch.from_numpy(np.concatenate([t.text, np.zeros(16, dtype=np.uint8)])).to(dev)
    d_off = torch.from_numpy(t.doc_off).to(dev)
    torch.cuda.synchronize()
    b.encode_device(d_text.data_ptr(), d_off.data_ptr(), len(t.doc_off) - 1, len(t.text), ordinary=True, count_only=count_only)
    if count_only:
        counts, status = b.fetch_counts()
        bad = np.nonzero(counts != np.diff(exp_off))[0]
        assert not len(bad), "%d documents with another count; the first: %s" % (len(bad), t.where(int(bad[0])))
    else:
        res = b.fetch()
        status = res.status
        assert np.array_equal(res.tok_off, exp_off), "token counts differ first in %s" % t.where(
            int(np.nonzero(np.diff(res.tok_off) != np.diff(exp_off))[0][0]))
        diff = np.nonzero(res.tokens != exp_tok)[0]
        if len(diff):
            d = int(np.searchsorted(exp_off, diff[0], side="right")) - 1
            docs = np.unique(np.searchsorted(exp_off, diff, side="right") - 1)
            raise AssertionError("%d tokens differ in %d documents (shards %s); the first: token %d of %s: expected %s, got %s" % (
                len(diff), len(docs), sorted(set((docs % mx.Q_SHARDS).tolist())), diff[0] - exp_off[d], t.where(d),
                exp_tok[diff[0]:diff[0] + 6].tolist(), res.tokens[diff[0]:diff[0] + 6].tolist()))
    assert not status.any()


@pytest.mark.parametrize("slots", mx.SLOTS)
def test_one_wave_per_shard(slots):
    """at most 64 entries per bin and shard: the side-by-side dispatch; then the counts alone, then again on the same Batch"""
    import jtokkit_amd
    b = jtokkit_amd.get_encoding(mx.NAME).new_batch()
    item = _item("small", slots)
    _run(b, item)
    _run(b, item, count_only=True)
    _run(b, item)
    b.close()


@pytest.mark.parametrize("slots", mx.SLOTS)
def test_every_workgroup_takes_a_slice(slots):
    """three passes' worth of entries and one wave more in one shard: 64 consecutive entries per wave in all four workgroups"""
    import jtokkit_amd
    b = jtokkit_amd.get_encoding(mx.NAME).new_batch()
    item = _item("large", slots)
    _run(b, item)
    _run(b, item, count_only=True)
    b.close()


@pytest.mark.parametrize("R", [2, 4])
def test_windows_at_their_thresholds(R):
    """exactly R x 4096 entries of 4..8 bytes in one shard: one pass of windows of R rounds, ordered by length"""
    import jtokkit_amd
    b = jtokkit_amd.get_encoding(mx.NAME).new_batch()
    item = _item("windows", R)
    _run(b, item)
    _run(b, item, count_only=True)
    b.close()
