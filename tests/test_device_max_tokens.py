"""jtk_batch_encode_device_max_tokens / HipEncoding.encode_batch_max_tokens_device: Encoding.encode(text, maxTokens) for a
device-resident batch into [n_docs, max_tokens] rows, with the early exit run as kernels.  Every check is against the CPU
oracle and, where stated, against the host call jtk_batch_encode_max_tokens on the same bytes (all fields equal).
Every test here needs a real MI355X (`-m gpu`)."""
import os
import random

import numpy as np
import pytest

import golden_util
import oracle_lib
import regex_crosscheck as rc

pytestmark = pytest.mark.gpu

NAMES = golden_util.ENCODING_NAMES
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD = -7


@pytest.fixture(scope="module")
def jt():
    import jtokkit_amd
    return jtokkit_amd


def _pack(texts):
    bs = [t if isinstance(t, (bytes, bytearray)) else t.encode("utf-8") for t in texts]
    doc_off = np.zeros(len(bs) + 1, dtype=np.int64)
    np.cumsum([len(x) for x in bs], out=doc_off[1:])
    text = np.frombuffer(b"".join(bs), dtype=np.uint8) if doc_off[-1] else np.zeros(0, dtype=np.uint8)
    return text, doc_off


def _device(enc, text, doc_off, mx, ordinary, pad_id=PAD, out=None):
    """The new call on torch tensors -> numpy (rows, kept, truncated, status)."""
    import torch
    dev = torch.device("cuda:0")
    d_text = torch.from_numpy(np.ascontiguousarray(text)).to(dev)
    d_off = torch.from_numpy(np.ascontiguousarray(doc_off)).to(dev)
    rows, kept, tr, st = enc.encode_batch_max_tokens_device(d_text, d_off, mx, ordinary=ordinary, pad_id=pad_id, out=out)
    torch.cuda.synchronize()
    return rows.cpu().numpy(), kept.cpu().numpy(), tr.cpu().numpy(), st.cpu().numpy()


def _assert_equals_host(enc, text, doc_off, mx, ordinary, got):
    """Every field equal to jtk_batch_encode_max_tokens on the same bytes; rows padded with PAD after kept."""
    rows, kept, tr, st = got
    b = enc.new_batch()
    h_rows, h_kept, h_tr, h_st = b.encode_max_tokens(text, doc_off, mx, ordinary)
    b.close()
    assert np.array_equal(st, h_st)
    assert np.array_equal(kept, h_kept)
    assert np.array_equal(tr.astype(np.uint8), h_tr)
    if mx > 0 and len(kept):
        cols = np.arange(mx)[None, :]
        live = cols < kept[:, None]
        assert np.array_equal(np.where(live, rows, 0), np.where(live, h_rows, 0))
        assert (rows[~live] == PAD).all()


def _assert_equals_oracle(o, texts, mx, ordinary, got, docs=None):
    rows, kept, tr, st = got
    for d in (range(len(texts)) if docs is None else docs):
        t = texts[d]
        if not ordinary and ("<|" in t if isinstance(t, str) else b"<|" in t):
            continue
        try:
            exp_toks, exp_tr = o.encode_ordinary(t, mx) if ordinary else o.encode(t, mx)
        except oracle_lib.OracleError:
            continue
        assert st[d] == 0, (d, mx)
        assert rows[d, :kept[d]].tolist() == exp_toks and bool(tr[d]) == exp_tr, (d, mx, t[:80])


@pytest.mark.parametrize("name", NAMES)
def test_golden_rows(jt, name):
    """encode(text, 10) for every fixture row: ids == the fixture's third column, truncated == the oracle, pad cells."""
    enc = jt.get_encoding(name)
    o = oracle_lib.get(name)
    rows_in = golden_util.load_rows(name)
    text, doc_off = _pack([r[0] for r in rows_in])
    rows, kept, tr, st = _device(enc, text, doc_off, 10, False)
    for d, (inp, _, expected10) in enumerate(rows_in):
        exp_toks, exp_tr = o.encode(inp, 10)
        assert st[d] == 0 and rows[d, :kept[d]].tolist() == expected10 and bool(tr[d]) == exp_tr, inp
        assert (rows[d, kept[d]:] == PAD).all()
    _assert_equals_host(enc, text, doc_off, 10, False, (rows, kept, tr, st))


def test_fuzz(jt):
    """The generator of test_batch_max_tokens_fuzz (multi-byte characters cut by the limit, U+FFFD, empty documents)."""
    enc = jt.get_encoding("cl100k_base")
    o = oracle_lib.get("cl100k_base")
    rng = random.Random(7)
    texts = [rc.random_text(rng, rng.randint(0, 60)) for _ in range(300)]
    texts += ["", "\ufffd", "a\ufffd\ufffdb", "\U0001F355" * 3, "I love \U0001F355", "\ufffd" * 7, "é" * 9, "한국어 " * 5]
    text, doc_off = _pack(texts)
    for mx in (0, 1, 2, 3, 5, 8, 13, 40, 4096):
        for ordinary in (True, False):
            got = _device(enc, text, doc_off, mx, ordinary)
            _assert_equals_host(enc, text, doc_off, mx, ordinary, got)
            _assert_equals_oracle(o, texts, mx, ordinary, got)


def _long_docs():
    from jtokkit_amd import corpus
    rng = random.Random(11)
    docs = []
    for text, off in (corpus.english(40, seed=3), corpus.mixed(60, seed=4)):
        docs += [bytes(text[off[i]:off[i + 1]]).decode("utf-8") for i in range(len(off) - 1)]
    ws = [" ", "  ", "\n", " \n", "\n\n ", "\t", "\r\n", "\u00a0", "\u2003", "\u3000", " \n \n  \n ", "   "]
    for mx in (1, 4, 10, 50):
        for grow in (1, 4, 16):
            cut = (8 * mx + 64) * grow
            for _ in range(6):
                head = rc.random_text(rng, 400)[:cut - rng.randint(0, 40)]
                run = "".join(rng.choice(ws) for _ in range(rng.randint(1, 30)))
                docs.append(head + run + rc.random_text(rng, 200) + "they'll we've 1234567 " * 20)
    docs += [" " * 5000 + "x", "\n" * 3000 + "end", "a" * 9000, "1234567890" * 700, ("it's " * 40 + "\n") * 30,
             "word " * 2000, "한국어 텍스트 " * 600, "x" + " \n" * 2500 + "y" * 50]
    return docs


def test_long_documents_need_later_rounds(jt):
    """White-space runs with line breaks placed around every prefix size the rounds try (rounds 2 and 3 are needed), all
    four encodings, limits 1, 4, 10, 50, 700: == the oracle on the whole document and == the host call."""
    docs = _long_docs()
    text, doc_off = _pack(docs)
    for name in NAMES:
        enc = jt.get_encoding(name)
        o = oracle_lib.get(name)
        for mx in (1, 4, 10, 50, 700):
            got = _device(enc, text, doc_off, mx, True)
            _assert_equals_oracle(o, docs, mx, True, got)
            _assert_equals_host(enc, text, doc_off, mx, True, got)


def test_encode_versus_encode_ordinary(jt):
    """encode() looks for special-token literals in the WHOLE document, not in the prefix it encodes; a literal split across
    two documents flags neither; encodeOrdinary() encodes the same document."""
    enc = jt.get_encoding("cl100k_base")
    o = oracle_lib.get("cl100k_base")
    far = "x" * 5000 + "<|endoftext|>"
    texts = ["hello world", far, "abc <|endof", "text|> def", "plain text again"]
    text, doc_off = _pack(texts)
    rows, kept, tr, st = _device(enc, text, doc_off, 3, False)
    assert st.tolist() == [0, jt._native.JTK_ERR_UNSUPPORTED_SPECIAL, 0, 0, 0]
    assert kept[1] == 0 and not tr[1] and (rows[1] == PAD).all()
    for d in (0, 2, 3, 4):
        exp, exp_tr = o.encode(texts[d], 3)
        assert rows[d, :kept[d]].tolist() == exp and bool(tr[d]) == exp_tr
    _assert_equals_host(enc, text, doc_off, 3, False, (rows, kept, tr, st))
    got = _device(enc, text, doc_off, 3, True)
    assert (got[3] == 0).all()
    assert got[0][1, :got[1][1]].tolist() == o.encode_ordinary(far, 3)[0]
    _assert_equals_host(enc, text, doc_off, 3, True, got)


@pytest.mark.parametrize("in_flight", [1, 2, 3])
def test_prefixes_over_several_chunks(jt, in_flight):
    """Small chunks so that the gathered prefixes span many chunks: the per-chunk decision against scratch-set reuse."""
    from jtokkit_amd import corpus
    enc = jt.new_encoding("cl100k_base")
    try:
        o = oracle_lib.get("cl100k_base")
        text, doc_off = corpus.mixed(3000, seed=21)
        b = enc._b()
        b.set_option(jt._native.JTK_OPT_CHUNK_BYTES, 1 << 16)
        b.set_option(jt._native.JTK_OPT_CHUNKS_IN_FLIGHT, in_flight)
        for mx in (10, 40):
            assert (3000 * (8 * mx + 64)) > 3 * (1 << 16)           # three chunks or more
            got = _device(enc, text, doc_off, mx, False)
            texts = [text[doc_off[d]:doc_off[d + 1]].tobytes().decode("utf-8") for d in range(len(doc_off) - 1)]
            _assert_equals_oracle(o, texts, mx, False, got, docs=range(0, 3000, 7))
            _assert_equals_host(enc, text, doc_off, mx, False, got)
    finally:
        enc.close()


def test_stream_ordering(jt):
    """The text is filled on a side stream and the call is made under that stream without a synchronise."""
    import torch
    enc = jt.get_encoding("cl100k_base")
    o = oracle_lib.get("cl100k_base")
    texts = ["The quick brown fox jumps over the lazy dog. " * (1 + d % 9) for d in range(500)]
    text, doc_off = _pack(texts)
    dev = torch.device("cuda:0")
    side = torch.cuda.Stream(device=dev)
    h_text = torch.from_numpy(text.copy()).pin_memory()
    h_off = torch.from_numpy(doc_off.copy()).pin_memory()
    with torch.cuda.stream(side):
        d_text = torch.zeros(len(text), dtype=torch.uint8, device=dev)
        d_off = torch.zeros(len(doc_off), dtype=torch.int64, device=dev)
        torch.cuda._sleep(20000000)                                  # the copies land well after the call is issued
        d_text.copy_(h_text, non_blocking=True)
        d_off.copy_(h_off, non_blocking=True)
        rows, kept, tr, st = enc.encode_batch_max_tokens_device(d_text, d_off, 12, pad_id=PAD)
    side.synchronize()
    got = (rows.cpu().numpy(), kept.cpu().numpy(), tr.cpu().numpy(), st.cpu().numpy())
    _assert_equals_oracle(o, texts, 12, False, got)
    _assert_equals_host(enc, text, doc_off, 12, False, got)


def test_caller_layouts_and_bad_offsets(jt):
    """Text at an odd address inside a larger tensor; a caller's `out` with the default pad; offsets that decrease or run
    past n_bytes are refused with JTK_ERR_INVALID_ARGUMENT and no row is written."""
    import torch
    enc = jt.get_encoding("cl100k_base")
    o = oracle_lib.get("cl100k_base")
    rng = random.Random(5)
    texts = [rc.random_text(rng, rng.randint(0, 300)) for _ in range(200)]
    text, doc_off = _pack(texts)
    dev = torch.device("cuda:0")
    big = torch.zeros(len(text) + 64, dtype=torch.uint8, device=dev)
    big[3:3 + len(text)] = torch.from_numpy(text).to(dev)
    d_text = big[3:3 + len(text)]
    assert d_text.data_ptr() % 2 == 1
    d_off = torch.from_numpy(doc_off).to(dev)
    out = torch.full((len(texts), 9), 12345, dtype=torch.int32, device=dev)
    rows, kept, tr, st = enc.encode_batch_max_tokens_device(d_text, d_off, 9, ordinary=True, out=out)
    assert rows.data_ptr() == out.data_ptr()
    got = (rows.cpu().numpy(), kept.cpu().numpy(), tr.cpu().numpy(), st.cpu().numpy())
    _assert_equals_oracle(o, texts, 9, True, got)
    cols = np.arange(9)[None, :]
    assert (got[0][cols >= got[1][:, None]] == -1).all()
    with pytest.raises(ValueError):
        enc.encode_batch_max_tokens_device(d_text, d_off, 9, out=torch.empty((len(texts), 8), dtype=torch.int32, device=dev))
    dec = doc_off.copy()
    dec[50] = dec[52] + 1                                             # decreasing
    past = doc_off.copy()
    past[-1] = len(text) + 5                                          # past n_bytes
    for bad in (dec, past):
        sentinel = torch.full((len(texts), 9), 777, dtype=torch.int32, device=dev)
        with pytest.raises(jt.EncodingError) as e:
            enc.encode_batch_max_tokens_device(d_text, torch.from_numpy(bad).to(dev), 9, out=sentinel)
        assert e.value.code == jt._native.JTK_ERR_INVALID_ARGUMENT
        assert (sentinel.cpu().numpy() == 777).all()


def test_rank_map_without_all_single_bytes(jt):
    """The map of test_rank_map_without_all_single_bytes (eleven single bytes removed): statuses and rows == the host call."""
    import base64
    from jtokkit_amd import corpus
    from test_gpu_parity import _train_tiny_bpe
    ranks = _train_tiny_bpe(corpus.english(40, seed=8)[0].tobytes() + "mañana 日本語 q z 789 qu iz".encode() * 20, 500)
    for bb in (b"q", b"z", b"7", b"8", b"9", b"\n", b"\xc3", b"\xe6", b"Q", b"~", b"\x00"):
        ranks.pop(bb, None)
    enc = jt.new_custom_encoding("partial_bytes", 1, ranks, {})
    try:
        rng = random.Random(9)
        words = ["the", "quick", "quiz", "zebra", "a", "of", "mañana", "日本語", "789", "1", "q", "z", "~", "Queen",
                 "size", "\n", " ", "  ", "x", "iz", "qu", "."]
        texts = [" ".join(rng.choice(words) for _ in range(rng.randint(0, 60))) for _ in range(600)]
        texts += [rc.random_text(rng, rng.randint(0, 80)) for _ in range(300)] + ["", "q", "the quiz", "no bad letters here"]
        text, doc_off = _pack(texts)
        for mx in (1, 3, 10, 50):
            got = _device(enc, text, doc_off, mx, True)
            assert (got[3] == jt._native.JTK_ERR_UNENCODABLE).sum() > 50
            _assert_equals_host(enc, text, doc_off, mx, True, got)
    finally:
        enc.close()


def test_custom_host_pattern_is_refused(jt):
    import re
    from jtokkit_amd.encoding import HipEncoding
    import torch
    enc = jt.get_encoding("cl100k_base")
    enc._host_pattern, saved = re.compile(r"\S+"), enc._host_pattern
    try:
        with pytest.raises(ValueError, match="custom split pattern"):
            enc.encode_batch_max_tokens_device(torch.zeros(4, dtype=torch.uint8, device="cuda:0"),
                                               torch.zeros(2, dtype=torch.int64, device="cuda:0"), 4)
    finally:
        enc._host_pattern = saved
    assert isinstance(enc, HipEncoding)


@pytest.mark.parametrize("mx", [10, 128])
def test_headline_corpus_200k(jt, mx):
    """200k documents of the headline corpus: every field == the host call; 3000 sampled documents == the oracle."""
    import sys
    sys.path.insert(0, ROOT)
    import bench
    enc = jt.get_encoding("cl100k_base")
    o = oracle_lib.get("cl100k_base")
    text, doc_off = bench.make_corpus("mixed", 200000, 3, min(16, len(os.sched_getaffinity(0))))
    got = _device(enc, text, doc_off, mx, False)
    _assert_equals_host(enc, text, doc_off, mx, False, got)
    rng = np.random.default_rng(4)
    rows, kept, tr, st = got
    for d in rng.choice(len(doc_off) - 1, 3000, replace=False).tolist():
        t = text[doc_off[d]:doc_off[d + 1]].tobytes().decode("utf-8")
        exp, exp_tr = o.encode(t, mx)
        assert st[d] == 0 and rows[d, :kept[d]].tolist() == exp and bool(tr[d]) == exp_tr, d
