"""The ordered windows of the 4..8-byte merge bin (lean_window in jtk_kernels.hip, jtk_merge_order_rules.h) against the CPU
oracle, bit-exact over all documents, tokens and offsets, plus count_only runs.

One text of 60 x 64 tiles, every tile a document.  A shard's bin-0 queue switches to windows of 64 R entries once it holds
2 x 4096 (R = 2) or 4 x 4096 (R = 4) entries -- 4096 = what the shard's four workgroups take in a pass of one round --, so
the hard pieces stand in the tiles of a few shards only, each shard with its own count and length pattern, and all other
tiles are one-token fillers:
    window edges     8191, 8192, 8193 and 16383, 16384, 16385 entries (one below, at, one above each threshold; the latter also
                     4 T K - 1, 4 T K, 4 T K + 1), and 16384 + 1, 63, 64, 65, 255 and 16384 + 8192 + 1 (what a pass of 4 and a
                     pass of 2 rounds leave for the passes of one round)
    length patterns  ascending, descending, all equal, 4 and 8 alternating, one 8-byte piece among 255 of 4 bytes, with period
                     256 along the shard's queue (tiles claim their queue space in any order, so a window is some 256
                     consecutive entries of these sequences, not an aligned one)
    to the end       two shards whose pieces run through all 60 tiles, so that every chunk of a three-chunk job has ordered
                     windows, the queues reused per scratch set
Pieces cycle through pools of 97 (4 bytes) and 251 (5..8 bytes) different hard pieces, so that a result written to another
entry of a window changes the tokens.  The longer lean bins are not ordered (the 17..32-byte bin was tried
and was no faster) and keep their tests in test_merge_paths_gpu.py."""
import numpy as np
import pytest

import oracle_lib
import pack_stage_cases as psc

pytestmark = pytest.mark.gpu

NAME = "cl100k_base"
T, Q_SHARDS = psc.T, 64
SPAN = 4 * 1024                                # JTK_M_WGS_PER_SHARD x JTK_ML_THREADS
TILES_PER_SHARD = 60
CHUNK_TILES = 20                               # tiles of a shard per chunk
CHUNK = CHUNK_TILES * Q_SHARDS * T             # 2.5 MiB: three chunks
ALL = 1 << 30

SPEC = {1: (2 * SPAN - 1, "four"), 2: (2 * SPAN, "four"), 3: (2 * SPAN + 1, "four"),
        4: (4 * SPAN - 1, "four"), 5: (4 * SPAN, "four"), 6: (4 * SPAN + 1, "four"),
        7: (4 * SPAN + 63, "four"), 8: (4 * SPAN + 64, "four"), 9: (4 * SPAN + 65, "four"), 10: (4 * SPAN + 255, "four"),
        11: (6 * SPAN + 1, "four"),
        20: (4 * SPAN + 100, "ascending"), 21: (4 * SPAN + 100, "descending"), 22: (4 * SPAN + 100, "equal"),
        23: (4 * SPAN + 100, "alternating"), 24: (6 * SPAN + 100, "one_long"), 25: (2 * SPAN + 100, "ascending"),
        26: (2 * SPAN + 100, "alternating"),
        40: (ALL, "four"), 41: (ALL, "ascending")}


def _length(pattern, i):
    k = i % 256
    if pattern == "four":
        return 4
    if pattern == "ascending":
        return 4 + k * 5 // 256
    if pattern == "descending":
        return 8 - k * 5 // 256
    if pattern == "equal":
        return 6
    if pattern == "alternating":
        return 4 if k % 2 == 0 else 8
    assert pattern == "one_long"
    return 8 if k == 137 else 4


class _Case:
    def __init__(self):
        w = self.w = psc.Words(NAME)
        pools = {4: w.hard(4, 97)}
        for n in (5, 6, 7, 8):
            pools[n] = w.hard(n, 251)
        filler = b"".join(psc.tile(w, []))
        assert len(filler) == T
        done = {s: 0 for s in SPEC}
        self.plan = {}                                     # tile -> its hard pieces
        parts = []
        for g in range(TILES_PER_SHARD * Q_SHARDS):
            s = g % Q_SHARDS
            if s not in SPEC or done[s] >= SPEC[s][0]:
                parts.append(filler)
                continue
            used, mine = 0, []
            while done[s] < SPEC[s][0]:
                n = _length(SPEC[s][1], done[s])
                if used + n > T or T - used - n == 1:
                    break
                mine.append(pools[n][done[s] % len(pools[n])])
                used += n
                done[s] += 1
            rest = T - used
            parts.append(b"".join(mine + w.fillers(rest, (rest + 9) // 10)))
            self.plan[g] = mine
        self.count = done
        for s, (n, _) in SPEC.items():
            assert done[s] == n or n == ALL, (s, done[s], n)
        assert done[40] == TILES_PER_SHARD * (T // 4) and done[41] > 4 * SPAN
        self.text = np.frombuffer(b"".join(parts), dtype=np.uint8).copy()
        self.doc_off = np.arange(TILES_PER_SHARD * Q_SHARDS + 1, dtype=np.int64) * T
        assert len(self.text) == self.doc_off[-1] and 2 * CHUNK < len(self.text) <= 3 * CHUNK
        # the plan is what the oracle splits: the first and the last tile with hard pieces of every shard
        o, raw = w.o, self.text.tobytes()
        for s in SPEC:
            tiles = [g for g in self.plan if g % Q_SHARDS == s]
            for g in (tiles[0], tiles[-1]):
                pieces = o.split(raw[g * T:(g + 1) * T])
                assert pieces[:len(self.plan[g])] == self.plan[g], (s, g)
                assert all(w.count(p) == 1 for p in pieces[len(self.plan[g]):]), (s, g)
        # every chunk of the three-chunk job has ordered windows in the shards that run to the end
        for c in range(3):
            per_chunk = sum(len(self.plan.get(g, ())) for g in range(c * CHUNK_TILES * Q_SHARDS, (c + 1) * CHUNK_TILES * Q_SHARDS)
                            if g % Q_SHARDS == 40)
            assert per_chunk >= 2 * SPAN
        self.exp_tok, self.exp_off = o.encode_batch(self.text, self.doc_off, threads=8)


_cache = {}


@pytest.fixture(scope="module")
def case():
    if "case" not in _cache:
        _cache["case"] = _Case()
    return _cache["case"]


@pytest.fixture(scope="module")
def dev(case):
    import torch
    d = torch.device("cuda:0")
    d_text = torch.from_numpy(np.concatenate([case.text, np.zeros(16, dtype=np.uint8)])).to(d)
    d_off = torch.from_numpy(case.doc_off).to(d)
    torch.cuda.synchronize()
    return d_text, d_off


def _where(case, d):
    s = d % Q_SHARDS
    return "tile %d, shard %d (%s)" % (d, s, "%d entries, %s" % (case.count[s], SPEC[s][1]) if s in SPEC else "fillers")


def _run(b, case, dev, count_only=False):
    d_text, d_off = dev
    b.encode_device(d_text.data_ptr(), d_off.data_ptr(), len(case.doc_off) - 1, len(case.text), ordinary=True, count_only=count_only)
    if count_only:
        counts, status = b.fetch_counts()
        bad = np.nonzero(counts != np.diff(case.exp_off))[0]
        assert not len(bad), "%d documents with another count; the first: %s" % (len(bad), _where(case, int(bad[0])))
    else:
        res = b.fetch()
        status = res.status
        assert np.array_equal(res.tok_off, case.exp_off), "token counts differ first in %s" % _where(
            case, int(np.nonzero(np.diff(res.tok_off) != np.diff(case.exp_off))[0][0]))
        diff = np.nonzero(res.tokens != case.exp_tok)[0]
        if len(diff):
            d = int(np.searchsorted(case.exp_off, diff[0], side="right")) - 1
            docs = np.unique(np.searchsorted(case.exp_off, diff, side="right") - 1)
            raise AssertionError("%d tokens differ in %d documents (shards %s); the first: token %d of %s: expected %s, got %s" % (
                len(diff), len(docs), sorted(set((docs % Q_SHARDS).tolist())), diff[0] - case.exp_off[d], _where(case, d),
                case.exp_tok[diff[0]:diff[0] + 6].tolist(), res.tokens[diff[0]:diff[0] + 6].tolist()))
    assert not status.any()


def test_window_edges_and_length_patterns(case, dev):
    """one chunk; then the counts alone; then the same batch again on the same Batch (stale LDS, stale queue tails)"""
    import jtokkit_amd
    b = jtokkit_amd.get_encoding(NAME).new_batch()
    _run(b, case, dev)
    _run(b, case, dev, count_only=True)
    _run(b, case, dev)
    b.close()


def test_three_chunks(case, dev):
    """2.5 MiB chunks: ordered windows in the first, second and third chunk, the queues reused per scratch set"""
    import jtokkit_amd
    from jtokkit_amd import _native as N
    b = jtokkit_amd.get_encoding(NAME).new_batch()
    b.set_option(N.JTK_OPT_CHUNK_BYTES, CHUNK)
    _run(b, case, dev)
    _run(b, case, dev, count_only=True)
    b.close()
