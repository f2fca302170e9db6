"""Queues at their bounds, docpre at its largest value, and device-resident batches on 1..4 scratch sets (GPU).

Everything is compared bit-exact with the CPU oracle; every status must be 0."""
import numpy as np
import pytest

import oracle_lib
import scratch_cases as sc

pytestmark = pytest.mark.gpu

T = 2048


@pytest.fixture(scope="module")
def enc():
    import jtokkit_amd
    return jtokkit_amd.get_encoding(sc.NAME, device=0)


@pytest.fixture(scope="module")
def oracle():
    return oracle_lib.get(sc.NAME)


def expect(oracle, text, doc_off):
    return oracle.encode_batch(np.frombuffer(text, dtype=np.uint8), np.asarray(doc_off, dtype=np.int64), threads=4)


def same(res, exp):
    assert np.array_equal(res.tok_off, exp[1]) and np.array_equal(res.tokens, exp[0])
    assert not res.status.any()


# ---- queues at their bounds ---------------------------------------------------------------------------------------------
# 3 tiles + 1 byte, and 65 tiles: the smallest count with two tiles in a queue shard (shard 0) and one in the others
@pytest.mark.parametrize("tiles", [3, 65])
@pytest.mark.parametrize("b", [7, 0, 1, 2])
def test_queue_of_a_bin_at_its_bound(enc, oracle, b, tiles):
    r = sc.rules()
    assert (tiles + r["shards"] - 1) // r["shards"] == (2 if tiles == 65 else 1)
    p = sc.hard_piece(sc.bin_lengths(r, b)[0])
    for shift in (0, 1):
        text = sc.back_to_back(p, tiles * T + 1, shift=shift)
        q = sc.queued(r, text)                                   # (the oracle alone accepts the input, and it fills the bin)
        assert max(n for (bb, _), n in q.items() if bb == b) >= r["tile_cap"][b] - 1
        doc_off = [0, len(text)]
        same(enc.encode_batch_packed(np.frombuffer(text, dtype=np.uint8), np.asarray(doc_off, dtype=np.int64), ordinary=True),
             expect(oracle, text, doc_off))


# ---- docpre: the count of tokens before a document start inside its tile ---------------------------------------------------
def test_document_starts_behind_a_tile_of_one_byte_pieces(enc, oracle):
    P = sc.pieces()
    # a digit and a mark, alternating: every byte a piece of its own, 2048 tokens in the tile; then documents that start at the
    # tile's last byte and at byte 0 of the next tile, with empty documents at both places
    text = b"1!" * (T // 2) + b"1!1!1"
    assert all(len(p) == 1 for p in P.o.split(text[:T - 1])) and len(P.o.split(text[:T - 1])) == T - 1
    doc_off = [0, T - 1, T - 1, T, T, T, len(text)]
    same(enc.encode_batch_packed(np.frombuffer(text, dtype=np.uint8), np.asarray(doc_off, dtype=np.int64), ordinary=True),
         expect(oracle, text, doc_off))


# ---- sets -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def five_chunks():
    """documents of uneven length over five chunks of 64 KiB, one of them a chunk by itself"""
    from jtokkit_amd import corpus
    text, off = corpus.mixed(80, seed=5)
    rnd = np.random.default_rng(7)
    docs = [bytes(text[off[i]:off[i + 1]]) for i in range(len(off) - 1)]
    out, doc_off, k = [], [0], 0
    while doc_off[-1] < 4 * 65536 + 30000:
        d = docs[k % len(docs)][:int(rnd.integers(1, 6000))]
        d = d.decode("utf-8", "ignore").encode()
        if k == 9:
            d = (docs[3] * 40)[:70000].decode("utf-8", "ignore").encode()      # alone a chunk
        out.append(d)
        doc_off.append(doc_off[-1] + len(d))
        k += 1
    return b"".join(out), np.asarray(doc_off, dtype=np.int64)


@pytest.fixture(scope="module")
def five_chunks_on_device(oracle, five_chunks):
    import torch
    text, doc_off = five_chunks
    return (expect(oracle, text, doc_off), torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).cuda(),
            torch.from_numpy(doc_off).cuda(), len(doc_off) - 1, len(text))


# (every case equals the oracle, so the five are identical to each other; None: the library's default)
@pytest.mark.parametrize("sets", [1, 2, 3, 4, None])
def test_every_number_of_sets_gives_the_same_answer(enc, five_chunks_on_device, sets):
    from jtokkit_amd import _native as N
    exp, d_text, d_off, n_docs, n_bytes = five_chunks_on_device
    b = enc.new_batch()
    b.set_option(N.JTK_OPT_CHUNK_BYTES, 65536)
    if sets:
        b.set_option(N.JTK_OPT_CHUNKS_IN_FLIGHT, sets)
    run = lambda: b.encode_device(d_text.data_ptr(), d_off.data_ptr(), n_docs, n_bytes, ordinary=True, sync=True, validate=True)
    run()
    same(b.fetch(), exp)
    # again on the same batch, with the chunk plan kept and the stages timed
    b.set_option(N.JTK_OPT_REUSE_CHUNK_PLAN, 1)
    b.set_profiling(True)
    run()
    run()                                                # (this one finds the plan of the one before)
    same(b.fetch(), exp)
    times = b.kernel_times()
    assert set(times) == {"mark_docs", "validate_utf8", "pretok_split", "piece_resolve", "bpe_merge", "tile_scan", "pack", "doc_offsets"}
    assert all(v > 0 for v in times.values()), times
    b.close()
