"""The part of the Python front end that every HipEncoding.*_device method shares: the check of doc_off, the re-staging of a
text that is not 16-byte aligned or has no readable tail, the fork to the batch's own stream from the legacy default stream and
the join back, the encode call and the copies of tok_off and status.  One tiny batch goes through every method that encodes a
device-resident batch, on the legacy default stream and on a torch.cuda.Stream(), with the text aligned and with tail slack
and as a view at byte offset 1 of a buffer that ends exactly where the text ends (so the staging branch runs).  Every returned
tensor is bit-equal over the four settings and equal to the method's host counterpart.  The results are read through the
stream the call ran on and through nothing else: a missing join shows as a mismatch, a device-wide wait would hide it.
Every test here needs a real MI355X (`-m gpu`)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DOCS = ["The quick brown fox jumps over the lazy dog, twice over; 1234567 times!",
        "",
        "naïve café — déjà vu \U0001F642 東京タワー",                      # ends in a 3-byte character
        "first part<|endoftext|>second part after the literal",
        "def f(x):\n    return x * 2  # twice\n\nprint(f(21))\n",
        "Line one.\nLine two? Yes!\n\nA new paragraph starts here and goes on a little."]
HELD_OUT = ["jumps over the lazy dog", "A new paragraph starts here"]
SPANS = [[(4, 19), (40, 55)], [], [(0, 6)], [(10, 23)], [], [(10, 24)]]      # byte ranges per document, sorted and disjoint
MINHASH = dict(ngram=3, num_hashes=32, bands=8, seed=7)
CHUNK = dict(chunk_tokens=8, overlap=2, unit="char", prefer="all")
SEQ_LEN, SEP = 16, "<|endoftext|>"
SETTINGS = [("default", "aligned"), ("default", "offset1"), ("side", "aligned"), ("side", "offset1")]
METHODS = ["compact_batch_device", "minhash_batch_device", "ngram_overlap_batch_device", "chunk_batch_device", "pack_batch_device",
           "token_spans_device", "token_offsets_device", "encode_batch_utf16_device"]


@pytest.fixture(scope="module")
def enc():
    import jtokkit_amd
    return jtokkit_amd.get_encoding("cl100k_base")


@pytest.fixture(scope="module")
def batch():
    bs = [d.encode("utf-8") for d in DOCS]
    doc_off = np.concatenate([[0], np.cumsum([len(x) for x in bs])]).astype(np.int64)
    us = [np.frombuffer(d.encode("utf-16-le"), dtype=np.uint16) for d in DOCS]
    unit_off = np.concatenate([[0], np.cumsum([len(x) for x in us])]).astype(np.int64)
    assert len(bs) == 6 and 250 <= doc_off[-1] <= 350 and b"" in bs and bs[2][-1] >= 0x80 and SEP.encode() in bs[3]
    begin = np.array([doc_off[d] + a for d, spans in enumerate(SPANS) for a, _ in spans], dtype=np.int64)
    end = np.array([doc_off[d] + e for d, spans in enumerate(SPANS) for _, e in spans], dtype=np.int64)
    return dict(text=np.frombuffer(b"".join(bs), dtype=np.uint8), doc_off=doc_off, units=np.concatenate(us), unit_off=unit_off,
                span_begin=begin, span_end=end)


@pytest.fixture(scope="module")
def held_out(enc):
    s = enc.ngram_set(3)
    s.add_texts(HELD_OUT)
    assert len(s) > 0
    yield s
    s.close()


def _place(arr, how):
    """The array on the device: 16-byte aligned with 32 readable bytes after it, or one element into a buffer that ends with it."""
    import torch
    if how == "aligned":
        buf = torch.from_numpy(np.concatenate([arr, np.zeros(32, dtype=arr.dtype)])).cuda()
        t = buf[:len(arr)]
        assert t.data_ptr() % 16 == 0
    else:
        buf = torch.from_numpy(np.concatenate([np.zeros(1, dtype=arr.dtype), arr])).cuda()
        t = buf[1:]
        st = t.untyped_storage()
        assert t.data_ptr() % 16 == arr.itemsize and st.data_ptr() + st.nbytes() == t.data_ptr() + arr.nbytes
    return t


def _call(enc, method, batch, held_out, how):
    import torch
    d = lambda a: torch.from_numpy(a.copy()).cuda()
    if method == "encode_batch_utf16_device":
        return enc.encode_batch_utf16_device(_place(batch["units"], how), d(batch["unit_off"]), ordinary=True)
    text, doc_off = _place(batch["text"], how), d(batch["doc_off"])
    if method == "compact_batch_device":
        return enc.compact_batch_device(text, doc_off, ordinary=True)
    if method == "minhash_batch_device":
        return enc.minhash_batch_device(text, doc_off, ordinary=True, **MINHASH)
    if method == "ngram_overlap_batch_device":
        return enc.ngram_overlap_batch_device(text, doc_off, held_out, ordinary=True)
    if method == "chunk_batch_device":
        return enc.chunk_batch_device(text, doc_off, ordinary=True, **CHUNK)
    if method == "pack_batch_device":
        return enc.pack_batch_device(text, doc_off, SEQ_LEN, sep=SEP, ordinary=True, span_begin=d(batch["span_begin"]),
                                     span_end=d(batch["span_end"]))
    if method == "token_spans_device":
        return enc.token_spans_device(text, doc_off, d(batch["span_begin"]), d(batch["span_end"]), ordinary=True)
    assert method == "token_offsets_device"
    return enc.token_offsets_device(text, doc_off, unit="char", ordinary=True)


def _run(enc, method, batch, held_out, stream, how):
    """The method's result as a dict of numpy arrays (and plain values), read through the stream the call ran on alone."""
    import torch
    s = torch.cuda.Stream() if stream == "side" else torch.cuda.default_stream()
    with torch.cuda.stream(s):
        # (the inputs are uploaded on `s` too: the call is ordered after them by the stream, as a caller's would be)
        res = _call(enc, method, batch, held_out, how)
        assert torch.cuda.current_stream() == s
        items = res.items() if isinstance(res, dict) else enumerate(res)
        return {k: v.cpu().numpy() if isinstance(v, torch.Tensor) else v for k, v in items}          # (.cpu() waits for `s`)


def _host(enc, method, batch, held_out):
    """The host counterpart's result under the device result's keys (a subset of them)."""
    if method == "compact_batch_device":
        r = enc.encode_batch_packed(batch["text"], batch["doc_off"], ordinary=True, compact=True)
        return {0: r.lo, 1: r.hi.view(np.int32), 2: r.tok_off, 3: r.status}
    if method == "minhash_batch_device":
        sig, nsh, keys = enc.minhash_batch(DOCS, ordinary=True, **MINHASH)
        return {0: sig.view(np.int32), 1: nsh, 2: keys.view(np.int64)}
    if method == "ngram_overlap_batch_device":
        return dict(enumerate(enc.ngram_overlap_batch(DOCS, held_out, ordinary=True)))
    if method == "chunk_batch_device":
        per_doc = enc.chunk_batch(DOCS, ordinary=True, **CHUNK)
        recs = [(d,) + rec for d, chunks in enumerate(per_doc) for rec in chunks]
        rows = np.full((len(recs), CHUNK["chunk_tokens"]), -1, dtype=np.int32)
        for c, rec in enumerate(recs):
            rows[c, :len(rec[1])] = rec[1]
        return dict(rows=rows, doc=np.array([r[0] for r in recs], dtype=np.int64), n_tok=np.array([len(r[1]) for r in recs], dtype=np.int32),
                    char_begin=np.array([r[2] for r in recs], dtype=np.int64), char_end=np.array([r[3] for r in recs], dtype=np.int64),
                    split=np.array([r[4] for r in recs], dtype=bool), level=np.array([r[5] for r in recs], dtype=np.uint8),
                    chunk_off=np.concatenate([[0], np.cumsum([len(c) for c in per_doc])]).astype(np.int64))
    if method == "pack_batch_device":
        return enc.pack_batch(DOCS, SEQ_LEN, sep=SEP, ordinary=True, train_spans=SPANS)
    if method == "token_spans_device":
        r = enc.pack_batch(DOCS, SEQ_LEN, ordinary=True, train_spans=SPANS)
        return {0: r["tok_span"], 2: r["status"]}
    if method == "token_offsets_device":
        r, begin, end = enc.encode_batch_with_offsets(DOCS, unit="char", ordinary=True)
        return {0: begin, 1: end, 2: r.tok_off, 3: r.status}
    assert method == "encode_batch_utf16_device"
    r = enc.encode_batch_utf16(batch["units"], batch["unit_off"], ordinary=True)
    return {0: r.tokens, 1: r.tok_off, 2: r.status, 3: batch["doc_off"]}


def _same(got, exp, what):
    if isinstance(exp, np.ndarray):
        assert isinstance(got, np.ndarray) and got.dtype == exp.dtype and got.shape == exp.shape, (what, got, exp)
        assert got.tobytes() == exp.tobytes(), (what, np.flatnonzero(got.ravel() != exp.ravel())[:10])
    else:
        assert type(got) is type(exp) and got == exp, (what, got, exp)


@pytest.mark.parametrize("method", METHODS)
def test_stream_and_staging_settings_agree(enc, batch, held_out, method):
    runs = {st: _run(enc, method, batch, held_out, *st) for st in SETTINGS}
    first = runs[SETTINGS[0]]
    assert len(first) >= 3 and any(isinstance(v, np.ndarray) and v.size > 6 for v in first.values())
    for st in SETTINGS[1:]:
        assert runs[st].keys() == first.keys(), (method, st)
        for k in first:
            _same(runs[st][k], first[k], (method, st, k))
    host = _host(enc, method, batch, held_out)
    assert host.keys() <= first.keys(), (method, sorted(map(str, host)), sorted(map(str, first)))
    for k, exp in host.items():
        _same(first[k], np.ascontiguousarray(exp) if isinstance(exp, np.ndarray) else exp, (method, "host", k))
