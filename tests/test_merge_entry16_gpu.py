"""The 16-byte entries of the queue of 4..8-byte pieces -- bytes, position and length in one word, written by k_piece_resolve
and read by lean_window and the loop of lean_bin<.., 0> (jtk_kernels.hip) -- against the CPU oracle (encodeOrdinary), bit-exact
over all documents, tokens and offsets, plus count_only runs, on the texts of merge_entry16_cases.py:

    shards    0, 1, 63, 64 and 65 entries in a shard (the loop of 64 consecutive entries alone); one below, at and above the
              2 x 4096 entries from which a shard is taken in ordered windows, and 1 and 63 entries behind the last window of 2
              and of 4 rounds; windows whose rounds are of one length (4, 5, 8) and whose rounds end at every length (the edges
              of a scan sized to the round's longest piece, were one built); 8-byte pieces that merge nothing -- eight single-byte tokens, the
              case that reads an entry's position before the result replaces it -- in windows and in the loop
    dense     every shard above the threshold; a prefix of it with every shard below; the same text in chunks of 1 MiB and of
              2.25 MiB, whose origins lie off the tile edges: positions relative to a chunk with a lead
    placed    pieces that merge nothing as a tile's first piece, as its last, and across tile edges
    others    r50k_base and p50k_base on mixed lengths
test_merge_entry16_cases_cpu.py asserts on the CPU that the texts hold what is said here."""
import numpy as np
import pytest

import merge_entry16_cases as mc
import oracle_lib

pytestmark = pytest.mark.gpu

NAME = "cl100k_base"
MIB = 1 << 20
_cache = {}


def _item(key):
    """(case, oracle tokens, oracle offsets), built once"""
    if key not in _cache:
        kind, name = key
        if kind == "main":
            t = mc.Shards(name, mc.MAIN_SPEC, mc.tiles_needed(mc.MAIN_SPEC))
        elif kind == "other":
            t = mc.Shards(name, mc.OTHER_SPEC, mc.tiles_needed(mc.OTHER_SPEC))
        elif kind == "dense":
            t = mc.dense(name)
        elif kind == "below":
            t = mc.below(mc.dense(name))
        else:
            t = mc.Placed(name)
        _cache[key] = (t,) + tuple(oracle_lib.get(name).encode_batch(t.text, t.doc_off, threads=8))
    return _cache[key]


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
            raise AssertionError("%d tokens differ in %d documents; the first: token %d of %s: expected %s, got %s" % (
                len(diff), len(docs), diff[0] - exp_off[d], t.where(d), exp_tok[diff[0]:diff[0] + 8].tolist(),
                res.tokens[diff[0]:diff[0] + 8].tolist()))
    assert not status.any()


def _batch(name=NAME, chunk_bytes=None):
    import jtokkit_amd
    from jtokkit_amd import _native as N
    b = jtokkit_amd.get_encoding(name).new_batch()
    if chunk_bytes:
        b.set_option(N.JTK_OPT_CHUNK_BYTES, chunk_bytes)
    return b


def test_shards_at_every_edge():
    """one chunk; then the counts alone; then the same batch again on the same Batch (stale LDS, stale queue entries)"""
    b = _batch()
    item = _item(("main", NAME))
    _run(b, item)
    _run(b, item, count_only=True)
    _run(b, item)
    b.close()


def test_every_shard_in_windows_then_every_shard_below():
    """the dense text, then on the same Batch its prefix that keeps every shard in the loop of 64 entries per wave"""
    b = _batch()
    _run(b, _item(("dense", NAME)))
    _run(b, _item(("below", NAME)))
    _run(b, _item(("below", NAME)), count_only=True)
    b.close()


@pytest.mark.parametrize("chunk_bytes", [MIB, mc.WINDOW_CHUNK])
def test_chunks_with_a_lead(chunk_bytes):
    """chunks that start off the tile edges: 1 MiB (no windows), 2.25 MiB (windows in both chunks)"""
    b = _batch(chunk_bytes=chunk_bytes)
    item = _item(("dense", NAME))
    _run(b, item)
    _run(b, item, count_only=True)
    b.close()


def test_pieces_that_merge_nothing_at_tile_edges():
    b = _batch()
    item = _item(("placed", NAME))
    _run(b, item)
    _run(b, item, count_only=True)
    b.close()


@pytest.mark.parametrize("name", ["r50k_base", "p50k_base"])
def test_other_encodings(name):
    b = _batch(name)
    item = _item(("other", name))
    _run(b, item)
    _run(b, item, count_only=True)
    b.close()
