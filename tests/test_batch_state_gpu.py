"""What a batch holds and when it is dropped: every encode entry point gives up the last encode's result and what was
derived from it -- chunks, pack, truncation, the byte scan, the character index --, every decode entry point the last decode's
and its UTF-16 units and stops, at the point of no return.  So a call that fails past that point leaves no result, and a call
refused for its arguments leaves the batch as it was.

One batch of 8 small documents of cl100k_base.  Every erroneous second input has the document and unit / byte counts of the
first, so no buffer is regrown, and every "dropped" is asserted as a host-side refusal (JTK_ERR_INVALID_ARGUMENT from the raw
jtk_batch_* call): no kernel runs on a dropped result.  Every test here needs a real MI355X (`-m gpu`)."""
import ctypes as C

import numpy as np
import pytest

import decode_cases as dc
import oracle_lib
import special_ref

pytestmark = pytest.mark.gpu

TABLE = "cl100k_base"
EOT = "<|endoftext|>"
DOCS = ["The quick brown fox jumps over the lazy dog.", "x", "naïve café — 日本語 \U0001f600 ok",
        "line one\nline two\n\nparagraph", "", "fim " + EOT + " tail", "    indented(code) { return 42; }", "1234567890 " * 5]
assert len(DOCS) == 8 and all(len(d.encode("utf-8")) <= 64 for d in DOCS)


@pytest.fixture(scope="module")
def jt():
    import jtokkit_amd
    return jtokkit_amd


@pytest.fixture(scope="module")
def N(jt):
    from jtokkit_amd import _native
    return _native


@pytest.fixture(scope="module")
def enc(jt):
    return jt.get_encoding(TABLE)


@pytest.fixture(scope="module")
def o():
    return oracle_lib.get(TABLE)


class _Input:
    """One order of DOCS in every form an encode entry takes, and the oracle's answer (encodeOrdinary), computed once."""

    def __init__(self, o, docs):
        bs = [d.encode("utf-8") for d in docs]
        self.docs = bs
        self.doc_off = np.zeros(len(bs) + 1, dtype=np.int64)
        np.cumsum([len(x) for x in bs], out=self.doc_off[1:])
        self.text = np.frombuffer(b"".join(bs), dtype=np.uint8)
        us = [np.frombuffer(d.encode("utf-16-le"), dtype=np.uint16) for d in docs]
        self.unit_off = np.zeros(len(us) + 1, dtype=np.int64)
        np.cumsum([len(u) for u in us], out=self.unit_off[1:])
        self.units = np.concatenate(us)
        self.piece_begin, self.piece_end = [], []
        for x, base in zip(bs, self.doc_off):                      # the oracle's own split: the pieces cover every byte
            p = int(base)
            for piece in o.split(x):
                self.piece_begin.append(p)
                p += len(piece)
                self.piece_end.append(p)
        self.tokens, self.tok_off = o.encode_batch(self.text, self.doc_off, ordinary=True)
        assert len(self.tokens) < 256
        allowed = {k.encode(): v for k, v in oracle_lib.ENCODINGS[TABLE]["specials"].items()}
        self.special = [special_ref.encode(o, x, allowed, ordinary=True) for x in bs]    # every special literal as its id
        for a in (self.doc_off, self.text, self.unit_off, self.units, self.tokens, self.tok_off):
            a.setflags(write=False)


@pytest.fixture(scope="module")
def first(o):
    return _Input(o, DOCS)


@pytest.fixture(scope="module")
def second(o, first):
    """The same documents in another order: the same counts, other offsets, another answer."""
    r = _Input(o, DOCS[::-1])
    assert r.tokens.tolist() != first.tokens.tolist()
    return r


def _dev(a):
    import torch
    t = torch.from_numpy(np.array(a)).cuda()
    torch.cuda.synchronize()
    return t


def _same_as_oracle(b, inp):
    r = b.fetch()
    assert r.tokens.tolist() == inp.tokens.tolist() and r.tok_off.tolist() == inp.tok_off.tolist() and not r.status.any()


def _derive(b, prefer=True):
    """Everything that exists only relative to the last encode."""
    (b.chunk_prefer if prefer else b.chunk)(4)
    b.pack(16)
    b.char_index("utf16")
    b.truncate(3)


# the raw reads, by the result they need: each returns JTK_OK while it is there (rows: room for the chunk and the pack rows of
# any order of DOCS, which make fewer than 256 tokens)
def _reads(N, b):
    import torch
    L, h = N.lib(), b._h
    p = C.c_void_p()
    scratch = torch.zeros(4096, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    rows = scratch.data_ptr()
    return {
        "keep": scratch,
        "result": lambda: L.jtk_batch_result(h, None, None, None),
        "fetch": lambda: L.jtk_batch_fetch(h, None, 0, None, None),
        "chunk_fetch": lambda: L.jtk_batch_chunk_fetch(h, None, None, None, None, None, None, None),
        "chunk_rows": lambda: L.jtk_batch_chunk_rows(h, 0, rows, None),
        "chunk_levels": lambda: L.jtk_batch_chunk_levels(h, None, C.byref(p)),
        "pack_write": lambda: L.jtk_batch_pack_write(h, 0, rows, None, None, None, None),
        "fetch_truncated": lambda: L.jtk_batch_fetch_truncated(h, None, None),
        "token_offsets": lambda: L.jtk_batch_token_offsets(h, None, None),
        "char_positions": lambda: L.jtk_batch_char_positions(h, N.JTK_UNIT_UTF16, N.JTK_CHAR_FLOOR, None, None, 0, None, None),
        "compact": lambda: L.jtk_batch_compact(h, None, None, None),
        "decode_utf16_fetch": lambda: L.jtk_batch_decode_utf16_fetch(h, None, 0, None, None),
        "decode_stops_fetch": lambda: L.jtk_batch_decode_stops_fetch(h, None, None, None, None),
    }


DERIVED = ("chunk_fetch", "chunk_rows", "chunk_levels", "pack_write", "fetch_truncated")


def _refused(N, reads, names):
    for name in names:
        assert reads[name]() == N.JTK_ERR_INVALID_ARGUMENT, name


def test_a_failed_encode_leaves_no_result(jt, N, enc, first):
    """jtk_batch_encode_utf16_device with unit offsets that the device check refuses: the transcode has written the new
    offsets over the last encode's by then."""
    b = enc.new_batch()
    b.encode_utf16_host(first.units, first.unit_off, ordinary=True)
    _same_as_oracle(b, first)
    _derive(b, prefer=False)
    reads = _reads(N, b)
    bad = np.array(first.unit_off)
    bad[1], bad[2] = bad[2], bad[1]
    assert bad[1] > bad[2] and len(bad) == len(first.unit_off) and bad.max() <= len(first.units)
    d_units, d_bad = _dev(first.units), _dev(bad)
    with pytest.raises(jt.EncodingError) as e:
        b.encode_utf16_device(d_units.data_ptr(), d_bad.data_ptr(), len(DOCS), len(first.units), ordinary=True)
    assert e.value.code == N.JTK_ERR_INVALID_ARGUMENT
    _refused(N, reads, ("result", "fetch", "chunk_fetch", "chunk_rows", "chunk_levels", "pack_write", "fetch_truncated", "token_offsets",
                    "char_positions", "compact"))
    d_off = _dev(first.unit_off)
    b.encode_utf16_device(d_units.data_ptr(), d_off.data_ptr(), len(DOCS), len(first.units), ordinary=True)
    _same_as_oracle(b, first)
    b.close()


def _entries(b, inp):
    """Every encode entry point on input `inp` -> the device arrays to keep alive, {name: (call, what the batch's result must be
    afterwards: "oracle", "special" (every literal as its id), None (an internal prefix group: not compared) or "none")}."""
    import torch
    keep = dict(text=_dev(inp.text), doc_off=_dev(inp.doc_off), units=_dev(inp.units), unit_off=_dev(inp.unit_off))
    nd, nb, nu, mt = len(inp.docs), len(inp.text), len(inp.units), 4
    rows = torch.zeros((nd, mt), dtype=torch.int32, device="cuda")
    kept = torch.zeros(nd, dtype=torch.int64, device="cuda")
    trunc = torch.zeros(nd, dtype=torch.uint8, device="cuda")
    status = torch.zeros(nd, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    keep.update(rows=rows, kept=kept, trunc=trunc, status=status)
    return keep, {
        "encode_host": (lambda: b.encode_host(inp.text, inp.doc_off, ordinary=True), "oracle"),
        "encode_device": (lambda: b.encode_device(keep["text"].data_ptr(), keep["doc_off"].data_ptr(), nd, nb, ordinary=True), "oracle"),
        "encode_pieces": (lambda: b.encode_pieces(inp.text, inp.doc_off, inp.piece_begin, inp.piece_end), "oracle"),
        "encode_utf16_host": (lambda: b.encode_utf16_host(inp.units, inp.unit_off, ordinary=True), "oracle"),
        "encode_utf16_device": (lambda: b.encode_utf16_device(keep["units"].data_ptr(), keep["unit_off"].data_ptr(), nd, nu,
                                                              ordinary=True), "oracle"),
        "encode_host_allow_special": (lambda: b.encode_host(inp.text, inp.doc_off, ordinary=True, allow_special=True), "special"),
        "encode_max_tokens": (lambda: b.encode_max_tokens(inp.text, inp.doc_off, mt, ordinary=True), None),
        "encode_device_max_tokens": (lambda: b.encode_device_max_tokens(keep["text"].data_ptr(), keep["doc_off"].data_ptr(), nd, nb, mt,
                                                                        rows.data_ptr(), kept.data_ptr(), trunc.data_ptr(),
                                                                        status.data_ptr(), ordinary=True), "none"),
    }


ENTRIES = ("encode_host", "encode_device", "encode_pieces", "encode_utf16_host", "encode_utf16_device", "encode_host_allow_special",
           "encode_max_tokens", "encode_device_max_tokens")


@pytest.mark.parametrize("entry", ENTRIES)
def test_every_encode_entry_drops_what_was_derived(N, enc, first, second, entry):
    b = enc.new_batch()
    b.encode_host(first.text, first.doc_off, ordinary=True)
    _derive(b)
    reads = _reads(N, b)
    for name in DERIVED:
        assert reads[name]() == N.JTK_OK, name                      # (each read is there to be dropped)
    keep, entries = _entries(b, second)
    call, expect = entries[entry]
    call()
    _refused(N, reads, DERIVED)
    if expect == "none":
        _refused(N, reads, ("result",))
    elif expect == "oracle":
        _same_as_oracle(b, second)
    elif expect == "special":
        assert any(EOT.encode() in x for x in second.docs)          # the stitched path: an allowed literal is there
        r = b.fetch()
        assert [r.doc(d).tolist() for d in range(len(second.docs))] == second.special and not r.status.any()
    del keep
    b.close()


def _decode_inputs(first):
    """Two id batches of 8 sequences with the same counts: the oracle's tokens, and the same sequences in reverse order."""
    seqs = [first.tokens[first.tok_off[d]:first.tok_off[d + 1]] for d in range(len(DOCS))]
    out = []
    for ss in (seqs, seqs[::-1]):
        off = np.zeros(len(ss) + 1, dtype=np.int64)
        np.cumsum([len(s) for s in ss], out=off[1:])
        out.append((np.concatenate(ss).astype(np.int32), off))
    return out


def _rows_of(ids, seq_off, pad):
    width = int(np.diff(seq_off).max())
    m = np.full((len(seq_off) - 1, width), pad, dtype=np.int32)
    for q in range(len(seq_off) - 1):
        m[q, :seq_off[q + 1] - seq_off[q]] = ids[seq_off[q]:seq_off[q + 1]]
    return m


@pytest.mark.parametrize("entry", ("decode_host", "decode_device", "decode_rows_host", "decode_rows_device"))
def test_every_decode_entry_drops_what_was_derived(N, enc, first, entry):
    tab = dc.table(TABLE)
    pad = 0                                                         # skipped as the pad id: "!" is in none of the documents
    assert not (first.tokens == pad).any()
    b = enc.new_batch()

    def run(ids, seq_off):
        if entry == "decode_host":
            b.decode_host(ids, seq_off)
        elif entry == "decode_device":
            d_ids, d_off = _dev(ids), _dev(seq_off)
            b.decode_device(d_ids.data_ptr(), d_off.data_ptr(), len(seq_off) - 1, len(ids))
        elif entry == "decode_rows_host":
            b.decode_rows_host(_rows_of(ids, seq_off, pad), pad_id=pad, skip_pad=True)
        else:
            m = _dev(_rows_of(ids, seq_off, pad))
            b.decode_rows_device(m.data_ptr(), 4, m.shape[0], m.shape[1], pad_id=pad, skip_pad=True)

    one, two = _decode_inputs(first)
    run(*one)
    b.decode_utf16()
    b.decode_find_stops([b"x"])
    reads = _reads(N, b)
    assert reads["decode_utf16_fetch"]() == N.JTK_OK and reads["decode_stops_fetch"]() == N.JTK_OK
    run(*two)
    _refused(N, reads, ("decode_utf16_fetch", "decode_stops_fetch"))
    out, byte_off, status = b.decode_fetch()
    exp_out, exp_off, exp_status = tab.decode_ref(*two)
    assert out.tobytes() == exp_out and byte_off.tolist() == exp_off.tolist() and status.tolist() == exp_status.tolist()
    b.close()


def test_a_call_refused_for_its_arguments_keeps_the_batch(N, enc, first):
    L = N.lib()
    b = enc.new_batch()
    b.encode_host(first.text, first.doc_off, ordinary=True)
    b.chunk(4)
    b.pack(16)
    b.decode_host(first.tokens, first.tok_off)                      # and a decode with what is derived from it
    b.decode_utf16()
    b.decode_find_stops([b"x"])

    def decode_state():
        return [np.array(a) for r in (b.decode_fetch(), b.decode_utf16_fetch(), b.decode_stops_fetch()) for a in r]

    before = (b.chunk_fetch(), b.pack_fetch(), b.fetch(), decode_state())
    assert bytes(before[3][0]) == first.text.tobytes()
    nt = C.c_int64(0)
    bad_off = np.array(first.doc_off)
    bad_off[0] = 1
    assert L.jtk_batch_encode(b._h, first.text.ctypes.data, bad_off.ctypes.data, len(DOCS), N.JTK_ENCODE_ORDINARY,
                              C.byref(nt)) == N.JTK_ERR_INVALID_ARGUMENT
    d_text, d_off = _dev(np.concatenate([first.text, np.zeros(16, dtype=np.uint8)])), _dev(first.doc_off)
    assert L.jtk_batch_encode_device(b._h, d_text.data_ptr() + 1, d_off.data_ptr(), len(DOCS), len(first.text), N.JTK_ENCODE_ORDINARY,
                                     None, C.byref(nt)) == N.JTK_ERR_INVALID_ARGUMENT
    ids = np.zeros(4, dtype=np.int32)
    seq_off = np.array([0, 3, 2, 4], dtype=np.int64)
    assert L.jtk_batch_decode(b._h, ids.ctypes.data, seq_off.ctypes.data, 3, C.byref(nt)) == N.JTK_ERR_INVALID_ARGUMENT
    after = (b.chunk_fetch(), b.pack_fetch(), b.fetch(), decode_state())
    for x, y in zip(before[:2], after[:2]):
        assert x.keys() == y.keys() and all(np.array_equal(x[k], y[k]) for k in x)
    assert all(np.array_equal(getattr(before[2], k), getattr(after[2], k)) for k in ("tokens", "tok_off", "status"))
    assert len(before[3]) == len(after[3]) == 10 and all(np.array_equal(x, y) for x, y in zip(before[3], after[3]))
    _same_as_oracle(b, first)
    b.close()


@pytest.fixture(scope="module")
def prompts(o):
    """About 300 KB of text: the golden prompts of the encoding, one document each, over and over; the oracle's ids, once."""
    import golden_util
    rows = [r[0].encode("utf-8") for r in golden_util.load_rows(TABLE) if r[0]]
    docs, total = [], 0
    while total < 300_000:
        docs.append(rows[len(docs) % len(rows)])
        total += len(docs[-1])
    doc_off = np.zeros(len(docs) + 1, dtype=np.int64)
    np.cumsum([len(x) for x in docs], out=doc_off[1:])
    text = np.frombuffer(b"".join(docs), dtype=np.uint8)
    tokens, tok_off = o.encode_batch(text, doc_off, ordinary=True)
    for a in (text, doc_off, tokens, tok_off):
        a.setflags(write=False)
    return text, doc_off, tokens, tok_off


def test_three_lives_of_everything_a_batch_owns(jt, N, enc, first, prompts):
    """Create, run, close, three times over, with one call of every family that makes the batch (or an n-gram set) own
    something: a host encode streamed to pinned memory in 64 KiB chunks (the scratch sets, their streams and events, the copy
    stream, the pinned planes), a device encode with chunk, pack, character index and truncation, UTF-16 in and out, a rows
    decode with stops, the device maxTokens rounds, an n-gram set that takes the batch.  Every round's ids are the oracle's:
    nothing a close() gave back is still in use, nothing the next batch allocates is stale."""
    import torch
    text, doc_off, tokens, tok_off = prompts
    assert len(text) > 4 * (1 << 16)
    nd, nb, mt, pad = len(DOCS), len(first.text), 4, 0
    d_text, d_off = _dev(np.concatenate([first.text, np.zeros(16, dtype=np.uint8)])), _dev(first.doc_off)
    seqs = [first.tokens[first.tok_off[d]:first.tok_off[d + 1]].tolist() for d in range(nd)]
    n_keys = set()
    for _ in range(3):
        b = enc.new_batch()
        b.set_option(N.JTK_OPT_HOST_CHUNK_BYTES, 1 << 16)
        assert b.encode_host(text, doc_off, ordinary=True, to_host=True) == len(tokens)
        r = b.host_result()
        assert np.array_equal(r.tokens, tokens) and np.array_equal(r.tok_off, tok_off) and not r.status.any()

        b.encode_device(d_text.data_ptr(), d_off.data_ptr(), nd, nb, ordinary=True)
        _same_as_oracle(b, first)
        _derive(b)
        s = enc.ngram_set(3)
        s.add_last_encode(b)
        n_keys.add(len(s))
        s.close()

        b.encode_utf16_host(first.units, first.unit_off, ordinary=True)
        _same_as_oracle(b, first)
        b.decode_host(first.tokens, first.tok_off)
        b.decode_utf16()
        units, unit_off, status = b.decode_utf16_fetch()
        assert units.tolist() == first.units.tolist() and unit_off.tolist() == first.unit_off.tolist() and not status.any()

        b.decode_rows_host(_rows_of(first.tokens, first.tok_off, pad), pad_id=pad, skip_pad=True)
        b.decode_find_stops([b"x"])
        out, byte_off, status = b.decode_fetch()
        assert out.tobytes() == first.text.tobytes() and byte_off.tolist() == first.doc_off.tolist() and not status.any()
        assert len(b.decode_stops_fetch()[0]) == nd

        rows = torch.zeros((nd, mt), dtype=torch.int32, device="cuda")
        kept = torch.zeros(nd, dtype=torch.int64, device="cuda")
        trunc = torch.zeros(nd, dtype=torch.uint8, device="cuda")
        st = torch.zeros(nd, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        b.encode_device_max_tokens(d_text.data_ptr(), d_off.data_ptr(), nd, nb, mt, rows.data_ptr(), kept.data_ptr(), trunc.data_ptr(),
                                   st.data_ptr(), ordinary=True)
        torch.cuda.synchronize()
        rows, kept = rows.cpu().numpy(), kept.cpu().numpy()
        assert not st.cpu().numpy().any() and (kept <= mt).all() and kept.sum() > 0
        assert all(rows[d, :kept[d]].tolist() == seqs[d][:kept[d]] for d in range(nd))
        b.close()
    assert len(n_keys) == 1 and min(n_keys) > 0
