"""Every implementation of bytePairMerge inside k_bpe_merge against the CPU oracle, bit-exact over all documents, on the texts of
merge_cases.py: irregular pieces of four kinds at the first and last lengths of each path (tiny, the three 16-byte lean bins, the
two text-reading lean bins, the two state-machine bins, the two wave-per-piece lists, giants), at pos & 15 of 0, 1 and 15, at a
tile's end, first in a document and last in the text; the same pieces in one document, as the second chunk of a two-chunk job,
behind a ballast that takes every shard out of the side-by-side dispatch, in shards with more entries than one pass
takes, and in lists longer than the grid.  tests/test_merge_cases_cpu.py asserts what these texts cover, and that an oracle
with the wrong tie-break or a stale neighbour rank would not produce these tokens.  Then table entries of 600 and 8,300 bytes
that k_long_shortcut must find and merge_long / merge_giant must skip.

Each text goes through Batch.encode_device on torch-owned buffers; a difference is reported with the case piece it falls in."""
import base64
import random

import numpy as np
import pytest

import merge_cases as mc
import merge_ref
import oracle_lib
import pack_stage_cases as psc

pytestmark = pytest.mark.gpu

_cache = {}


@pytest.fixture(scope="module")
def jt():
    import jtokkit_amd
    return jtokkit_amd


def _plan(name):
    if ("plan", name) not in _cache:
        _cache[("plan", name)] = mc.Plan(name)
    return _cache[("plan", name)]


def _item(name, label):
    """(Text, oracle tokens, oracle offsets) of one text, built once; the split into the planned pieces is asserted first"""
    key = (name, label)
    if key not in _cache:
        plan = _plan(name)
        if label == "crowded":
            texts = [mc.crowded(plan.P)[0]]
        elif label == "lists":
            texts = [mc.lists(plan.P)]
        elif label == "tails":
            texts = plan.tail_texts()
        else:
            texts = [getattr(plan, label)()]
        out = []
        for t in texts:
            mc.check_splits(plan.P, t)
            out.append((t,) + tuple(oracle_lib.get(name).encode_batch(t.text, t.doc_off, threads=8)))
        _cache[key] = out if label == "tails" else out[0]
    return _cache[key]


def _to_device(text, doc_off):
    import torch
    dev = torch.device("cuda:0")
    d_text = torch.from_numpy(np.concatenate([text, np.zeros(16, dtype=np.uint8)])).to(dev)
    d_off = torch.from_numpy(np.ascontiguousarray(doc_off, dtype=np.int64)).to(dev)
    assert d_text.data_ptr() % 16 == 0
    torch.cuda.synchronize()
    return d_text, d_off


def _token_bytes(name):
    if ("len", name) not in _cache:
        ranks = merge_ref.load_ranks(name)
        lens = np.zeros(max(ranks.values()) + 1, dtype=np.int64)
        for k, v in ranks.items():
            lens[v] = len(k)
        _cache[("len", name)] = lens
    return _cache[("len", name)]


def _first_difference(name, t, exp_tok, exp_off, got_tok, got_off):
    """the first differing document or token, and the case piece it belongs to"""
    if len(exp_off) != len(got_off):
        return "%s: %d documents expected, %d returned" % (t.label, len(exp_off) - 1, len(got_off) - 1)
    counts_e, counts_g = np.diff(exp_off), np.diff(got_off)
    n = min(len(exp_tok), len(got_tok))
    diff = np.nonzero(exp_tok[:n] != got_tok[:n])[0]
    bad_doc = np.nonzero(counts_e != counts_g)[0]
    j = int(diff[0]) if len(diff) else n
    d = int(np.searchsorted(exp_off, j, side="right")) - 1
    if len(bad_doc) and bad_doc[0] < d:
        d = int(bad_doc[0])
        j = int(exp_off[d])
    d = min(d, len(t.doc_off) - 2)
    lens = _token_bytes(name)
    at = int(t.doc_off[d]) + int(lens[exp_tok[exp_off[d]:j]].sum())
    return "document %d (bytes %d..%d, %d tokens expected, %d returned), token %d of it at byte %d: expected %s, got %s -- %s" % (
        d, t.doc_off[d], t.doc_off[d + 1], counts_e[d], counts_g[d], j - exp_off[d], at, exp_tok[j:j + 6].tolist(),
        got_tok[j:j + 6].tolist(), t.where(at))


def _run(b, name, item, count_only=False):
    t, exp_tok, exp_off = item
    d_text, d_off = _to_device(t.text, t.doc_off)
    b.encode_device(d_text.data_ptr(), d_off.data_ptr(), len(t.doc_off) - 1, len(t.text), ordinary=True, count_only=count_only)
    if count_only:
        counts, status = b.fetch_counts()
        bad = np.nonzero(counts != np.diff(exp_off))[0]
        assert not len(bad), "%d documents with another count; the first: %d (%d expected, %d returned) -- %s" % (
            len(bad), bad[0], np.diff(exp_off)[bad[0]], counts[bad[0]], t.where(int(t.doc_off[bad[0]])))
    else:
        res = b.fetch()
        status = res.status
        same = np.array_equal(res.tok_off, exp_off) and np.array_equal(res.tokens, exp_tok)
        assert same, _first_difference(name, t, exp_tok, exp_off, res.tokens, res.tok_off)
    assert not status.any()


@pytest.mark.parametrize("name", ["cl100k_base", "r50k_base"])
def test_per_piece(jt, name):
    """every piece in a document of its own, and the texts that end with their piece; r50k_base: the same generators on that
    table (pieces, hunts and splits redone with its oracle)"""
    b = jt.get_encoding(name).new_batch()
    _run(b, name, _item(name, "per_piece"))
    for item in _item(name, "tails"):
        _run(b, name, item)
    b.close()


def test_one_document(jt):
    b = jt.get_encoding(mc.NAME).new_batch()
    _run(b, mc.NAME, _item(mc.NAME, "one_document"))
    b.close()


def test_second_chunk_of_two(jt):
    from jtokkit_amd import _native as N
    b = jt.get_encoding(mc.NAME).new_batch()
    b.set_option(N.JTK_OPT_CHUNK_BYTES, psc.CHUNK)
    item = _item(mc.NAME, "second_chunk")
    assert psc.CHUNK * 5 // 4 < len(item[0].text) <= 2 * psc.CHUNK and item[0].doc_off[1] == psc.SECOND_BASE
    _run(b, mc.NAME, item)
    _run(b, mc.NAME, item, count_only=True)
    b.close()


def test_count_only(jt):
    b = jt.get_encoding(mc.NAME).new_batch()
    _run(b, mc.NAME, _item(mc.NAME, "per_piece"), count_only=True)
    _run(b, mc.NAME, _item(mc.NAME, "crowded"), count_only=True)
    b.close()


def test_sliced_dispatch(jt):
    """1536 bin-0 entries in every shard: no shard runs its bins side by side; its first two workgroups take slices of bin 0
    and its first one the other bins"""
    b = jt.get_encoding(mc.NAME).new_batch()
    _run(b, mc.NAME, _item(mc.NAME, "sliced"))
    b.close()


def test_crowded_shards(jt):
    """one shard per bin with more entries than one pass takes (more than M_CHUNK in bin 5), all pieces different"""
    b = jt.get_encoding(mc.NAME).new_batch()
    _run(b, mc.NAME, _item(mc.NAME, "crowded"))
    b.close()


def test_lists_longer_than_the_grid(jt):
    """4099 mid pieces, 259 long ones, 257 giants: a second piece in the same wave's and workgroup's LDS"""
    b = jt.get_encoding(mc.NAME).new_batch()
    _run(b, mc.NAME, _item(mc.NAME, "lists"))
    b.close()


def test_same_batch_object(jt):
    """nothing that a long or giant piece left in the scratch words of its byte positions leaks into a later job"""
    b = jt.get_encoding(mc.NAME).new_batch()
    for label in ("lists", "per_piece", "crowded", "per_piece"):
        _run(b, mc.NAME, _item(mc.NAME, label))
    b.close()


@pytest.mark.parametrize("kind", [0, 1])
def test_long_and_giant_table_entries(jt, kind):
    """A listed piece that is itself a table entry is one token (GptBytePairEncoding.java:81-83): k_long_shortcut marks it and
    merge_long / merge_giant skip it.  A trained table plus irregular entries of 600 and 8,300 bytes that merging cannot
    produce; the entry alone, doubled, with a byte more, with a byte less and between other words, against an oracle built
    from the same table."""
    from jtokkit_amd import corpus
    from test_gpu_parity import _train_tiny_bpe
    ranks = _train_tiny_bpe(corpus.english(40, seed=5)[0].tobytes(), 400)
    rnd = random.Random(kind)
    extra = [b" " + "".join(rnd.choice("abcdefghijklmnopqrstuvwxyz") for _ in range(n - 1)).encode() for n in (600, 8300)]
    for e in extra:
        assert e not in ranks
        ranks[e] = len(ranks) + 3
    enc = jt.new_custom_encoding("long_entries_%d" % kind, kind, ranks, {})
    data = b"\n".join(base64.b64encode(k) + b" " + str(v).encode() for k, v in sorted(ranks.items(), key=lambda kv: kv[1])) + b"\n"
    o = oracle_lib.OracleEncoding("long_entries_%d" % kind, kind, data, {})
    texts = []
    for e in extra:
        s = e.decode()
        texts += [s, s + s, s + "q", s[:-1], "the of" + s + " and a", s + s[:-1] + s + "x" + s, "a" + s[1:]]
    res = enc.encode_batch(texts, ordinary=True)
    assert not res.status.any()
    for d, t in enumerate(texts):
        exp = o.encode_ordinary(t)
        got = res.doc(d).tolist()
        assert got == exp, "text %d (%d bytes, starts %r): %d tokens expected, %d returned; first difference at token %d" % (
            d, len(t), t[:12], len(exp), len(got), next((k for k, (x, y) in enumerate(zip(exp, got)) if x != y), min(len(exp), len(got))))
    for e in extra:
        assert enc.encode_ordinary(e.decode()) == [ranks[e]] and enc.encode_ordinary((e + e).decode()) == [ranks[e]] * 2
        assert len(enc.encode_ordinary(e.decode() + "q")) > 100
    enc.close()
