"""jtk_batch_char_index / _char_positions / _byte_positions / _token_char_offsets and the Python methods on top of them
(encode_batch_with_offsets, chunk_batch(unit=...), chunk_batch_device(unit=...), pack_batch(span_unit=...),
token_offsets_device): character positions of the batch text in UTF-16 units and code points.  Expected values come from the
plain restatement of the rule (tests/charpos_ref.py), for the tokens applied to the CPU oracle's tokens and to byte lengths taken
from the oracle's decode of single ids; nothing the device computes enters them.  Every entry is compared.
Every test here needs a real MI355X (`-m gpu`)."""
import random

import numpy as np
import pytest

import charpos_cases as cc
import charpos_ref as cr
import golden_util
import label_ref
import oracle_lib
import special_ref

pytestmark = pytest.mark.gpu

EOT = "<|endoftext|>"
EOT_ID = 100257
UNITS = ((cr.UTF16, "utf16"), (cr.CODEPOINT, "char"))


@pytest.fixture(scope="module")
def jt():
    import jtokkit_amd
    return jtokkit_amd


@pytest.fixture(scope="module")
def o():
    return oracle_lib.get("cl100k_base")


_len_cache = {}


def _tok_len(o, specials, t):
    """Decoded byte length of one id: the oracle's decode of the single id, a special id's literal."""
    if t not in _len_cache:
        _len_cache[t] = len(specials[t]) if t in specials else len(o.decode_bytes([t]))
    return _len_cache[t]


def _token_expectation(r, doc_lens, unit):
    """FLOOR of every token's first byte and CEIL of its end, relative to its document, by the reference."""
    p, q = label_ref.token_positions(doc_lens, r.doc_off)
    doc = np.repeat(np.arange(len(doc_lens)), [len(x) for x in doc_lens])
    begin = np.array([r.char_index(int(d), int(x), unit, cr.FLOOR) for d, x in zip(doc, p)], dtype=np.int64)
    end = np.array([r.char_index(int(d), int(x), unit, cr.CEIL) for d, x in zip(doc, q)], dtype=np.int64)
    return begin, end


@pytest.fixture(scope="module")
def batch(o):
    """One batch of about 20 KB: the CPU case set (its edge documents first, so that they sit on the index's edges), a few golden
    prompts, an emoji run and empty documents -- more than four superblocks and a ragged tail.  `full` holds the malformed
    documents too (positions); `tok` is the well-formed part (more than 2,048 tokens: the token pass crosses a tile) with the
    oracle's tokens and their byte lengths.  The reference's answers to every query, computed once."""
    golden = [r[0].encode("utf-8") for r in golden_util.load_rows("cl100k_base")][::60]
    extra = golden + [b"", ("\U0001F355\U0001F469‍\U0001F373" * 12).encode("utf-8"), b"", b""]
    full = cr.Ref(cc.edge_docs() + cc.malformed_docs() + cc.script_docs() + extra)
    assert cc.edges_reached(full.docs) == cc.ALL_EDGES and 18000 < full.n_bytes < 24000
    exp = {}
    pos, doc = full.all_positions()
    free = full.free_positions()
    for unit, _ in UNITS:
        exp[("units", unit)] = full.doc_units(unit)
        for rnd in cr.ROUNDS:
            exp[("named", unit, rnd)] = full.expected_char_positions(unit, rnd, pos, doc)
            exp[("free", unit, rnd)] = full.expected_char_positions(unit, rnd, free)
        qd, qk = full.all_char_queries(unit)
        exp[("inverse", unit)] = (qd, qk, full.expected_byte_positions(unit, qd, qk))
    tok = cr.Ref(cc.edge_docs() + cc.script_docs() + extra)
    docs = [o.encode_ordinary(x) for x in tok.docs]
    doc_lens = [[_tok_len(o, {}, t) for t in d] for d in docs]
    assert all(sum(lens) == len(x) for lens, x in zip(doc_lens, tok.docs))    # the tokens decode to the text
    n_tok = sum(len(d) for d in docs)
    assert 2048 < n_tok < 16000
    tok_exp = {unit: _token_expectation(tok, doc_lens, unit) for unit, _ in UNITS}
    b, e = tok_exp[cr.CODEPOINT]
    assert (e > b).all() and (e - b > 1).any()
    p, _ = label_ref.token_positions(doc_lens, tok.doc_off)
    assert any((tok.text[int(x)] & 0xC0) == 0x80 for x in p)                  # a token that starts inside a character
    return dict(full=full, pos=pos, doc=doc, free=free, exp=exp, tok=tok, docs=docs, doc_lens=doc_lens, n_tok=n_tok, tok_exp=tok_exp,
                tok_off=np.concatenate([[0], np.cumsum([len(d) for d in docs])]).astype(np.int64))


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()                              # (a copy: frombuffer views are read-only)


def _out(n):
    import torch
    return torch.full((n + 1,), 12345, dtype=torch.int64, device="cuda")


def _get(t):
    """The call's output without the sentinel behind it, which must be untouched."""
    import torch
    torch.cuda.synchronize()
    a = t.cpu().numpy()
    assert a[-1] == 12345
    return a[:-1]


def _char_positions(b, unit, rnd, pos, doc=None):
    import torch
    d_pos, d_doc, out = _dev(pos), None if doc is None else _dev(doc), _out(len(pos))
    torch.cuda.synchronize()                                                # (the library's streams do not wait for torch's)
    b.char_positions(unit, d_pos.data_ptr(), len(pos), out.data_ptr(), rnd, None if doc is None else d_doc.data_ptr())
    return _get(out)


def _byte_positions(b, unit, doc, k):
    import torch
    d_doc, d_k, out = _dev(doc), _dev(k), _out(len(doc))
    torch.cuda.synchronize()
    b.byte_positions(unit, d_doc.data_ptr(), d_k.data_ptr(), len(doc), out.data_ptr())
    return _get(out)


def _doc_units(b, unit, nd):
    import torch
    out = _out(nd)
    torch.cuda.synchronize()
    b.char_index(unit, out.data_ptr())
    return _get(out)


def _check_positions(b, r, exp, pos, doc, free, units=UNITS):
    for unit, _ in units:
        assert np.array_equal(_doc_units(b, unit, len(r.docs)), exp[("units", unit)]), unit
        for rnd in cr.ROUNDS:
            got = _char_positions(b, unit, rnd, pos, doc)
            assert np.array_equal(got, exp[("named", unit, rnd)]), (unit, rnd, "named", np.flatnonzero(got != exp[("named", unit, rnd)])[:10])
            got = _char_positions(b, unit, rnd, free)
            assert np.array_equal(got, exp[("free", unit, rnd)]), (unit, rnd, "searched", np.flatnonzero(got != exp[("free", unit, rnd)])[:10])
        qd, qk, e = exp[("inverse", unit)]
        got = _byte_positions(b, unit, qd, qk)
        assert np.array_equal(got, e), (unit, "inverse", np.flatnonzero(got != e)[:10])


def test_every_position_of_the_batch(jt, batch):
    """char_positions for every byte position (and one past either end) of every document, both rounds, UTF-16 and code points,
    with the document named and searched; byte_positions for every (d, k) from -1 to doc_units + 2; doc_units.  After a
    count-only encode of host input (these calls read only the text) and after an encode of device input."""
    import torch
    enc = jt.get_encoding("cl100k_base")
    r = batch["full"]
    b = enc.new_batch()
    b.encode_host(r.text, r.doc_off, ordinary=True, count_only=True)
    _check_positions(b, r, batch["exp"], batch["pos"], batch["doc"], batch["free"])
    d_text, d_off = _dev(np.concatenate([r.text, np.full(16, 0xFF, dtype=np.uint8)])), _dev(r.doc_off)   # (bytes past the end must count 0)
    torch.cuda.synchronize()
    b.encode_device(d_text.data_ptr(), d_off.data_ptr(), len(r.docs), r.n_bytes, ordinary=True)
    _check_positions(b, r, batch["exp"], batch["pos"], batch["doc"], batch["free"])
    # JTK_UNIT_BYTE: document-relative byte offsets, rounded to characters
    pos, doc = batch["pos"], batch["doc"]
    for rnd in cr.ROUNDS:
        assert np.array_equal(_char_positions(b, "byte", rnd, pos, doc), r.expected_char_positions(cr.BYTE, rnd, pos, doc)), rnd
    qd, qk = r.all_char_queries(cr.BYTE)
    assert np.array_equal(_byte_positions(b, cr.BYTE, qd, qk), r.expected_byte_positions(cr.BYTE, qd, qk))
    b.close()


def _token_offsets(b, unit, n_tok, with_end=True):
    import torch
    begin, end = _out(n_tok), _out(n_tok)
    torch.cuda.synchronize()
    b.token_char_offsets(unit, begin.data_ptr(), end.data_ptr() if with_end else None)
    return _get(begin), _get(end)


def test_token_char_offsets(jt, batch):
    """Host-input and device-input encodes, with and without a chunk call before (the byte scan is reused), with and without
    the end array: begin and end of every token equal the reference applied to the oracle's tokens."""
    import torch
    enc = jt.get_encoding("cl100k_base")
    r, n_tok = batch["tok"], batch["n_tok"]
    d_text, d_off = _dev(r.text), _dev(r.doc_off)
    b = enc.new_batch()
    for chunk_first in (False, True):
        b.encode_host(r.text, r.doc_off, ordinary=True)
        assert b.result()[0] == n_tok
        if chunk_first:
            b.chunk(64)
        for unit, name in UNITS:
            eb, ee = batch["tok_exp"][unit]
            gb, ge = _token_offsets(b, name, n_tok)
            assert np.array_equal(gb, eb), ("host", chunk_first, name, "begin", np.flatnonzero(gb != eb)[:10])
            assert np.array_equal(ge, ee), ("host", chunk_first, name, "end", np.flatnonzero(ge != ee)[:10])
    gb, ge = _token_offsets(b, cr.UTF16, n_tok, with_end=False)
    assert np.array_equal(gb, batch["tok_exp"][cr.UTF16][0]) and (ge == 12345).all()
    b.close()
    for unit, name in UNITS:
        eb, ee = batch["tok_exp"][unit]
        gb, ge, t_off, st = enc.token_offsets_device(d_text, d_off, name, ordinary=True)
        torch.cuda.synchronize()
        assert gb.dtype == torch.int64 and np.array_equal(gb.cpu().numpy(), eb) and np.array_equal(ge.cpu().numpy(), ee), ("device", name)
        assert np.array_equal(t_off.cpu().numpy(), batch["tok_off"]) and (st.cpu().numpy() == 0).all()


def test_token_char_offsets_with_special_tokens_as_ids(jt, o):
    """allowed_special="all": <|endoftext|> is one token that spans its literal's 13 characters."""
    import torch
    enc = jt.get_encoding("cl100k_base")
    texts = ["héad " + EOT + " tail 語", EOT + EOT, "plain text without one", "\U0001F600" + EOT, ""]
    r = cr.Ref([t.encode("utf-8") for t in texts])
    amap = {k.encode(): v for k, v in enc._specials.items()}
    lits = {v: k for k, v in amap.items()}
    docs = [special_ref.encode(o, x, amap) for x in r.docs]
    assert sum(d.count(EOT_ID) for d in docs) == 4
    doc_lens = [[_tok_len(o, lits, t) for t in d] for d in docs]
    assert all(sum(lens) == len(x) for lens, x in zip(doc_lens, r.docs))
    n_tok = sum(len(d) for d in docs)
    b = enc.new_batch()
    b.set_allowed_special("all")
    assert b.encode_host(r.text, r.doc_off, allow_special=True) == n_tok
    for unit, name in UNITS:
        eb, ee = _token_expectation(r, doc_lens, unit)
        gb, ge = _token_offsets(b, name, n_tok)
        assert np.array_equal(gb, eb) and np.array_equal(ge, ee), name
        flat = [t for d in docs for t in d]
        assert all(ee[i] - eb[i] == len(EOT) for i, t in enumerate(flat) if t == EOT_ID)
        db, de, _, st = enc.token_offsets_device(_dev(r.text), _dev(r.doc_off), name, allowed_special="all")
        torch.cuda.synchronize()
        assert (st.cpu().numpy() == 0).all() and np.array_equal(db.cpu().numpy(), eb) and np.array_equal(de.cpu().numpy(), ee), name
    b.close()


def test_a_new_encode_and_another_unit_drop_the_index(jt, batch):
    """Batch A, query; a different batch B on the same Batch, query: B's answers; then the other unit: B's answers in it."""
    enc = jt.get_encoding("cl100k_base")
    a = batch["full"]
    rb = cr.Ref(list(reversed(cc.script_docs())) + [cc.fill(random.Random(2), 4096 + 77)] + cc.malformed_docs())
    b = enc.new_batch()
    b.encode_host(a.text, a.doc_off, ordinary=True)
    assert np.array_equal(_char_positions(b, cr.UTF16, cr.FLOOR, batch["free"]), batch["exp"][("free", cr.UTF16, cr.FLOOR)])
    b.encode_host(rb.text, rb.doc_off, ordinary=True)
    free = rb.free_positions()
    assert rb.n_bytes != a.n_bytes
    for unit in (cr.UTF16, cr.CODEPOINT, cr.UTF16):
        for rnd in cr.ROUNDS:
            assert np.array_equal(_char_positions(b, unit, rnd, free), rb.expected_char_positions(unit, rnd, free)), (unit, rnd)
        assert np.array_equal(_doc_units(b, unit, len(rb.docs)), rb.doc_units(unit)), unit
        qd, qk = rb.all_char_queries(unit)
        assert np.array_equal(_byte_positions(b, unit, qd, qk), rb.expected_byte_positions(unit, qd, qk)), unit
    assert not np.array_equal(rb.doc_units(cr.UTF16), rb.doc_units(cr.CODEPOINT))
    b.close()


def test_refusals(jt):
    """Every call that include/jtokkit_amd.h says is refused, and the empty calls that are not."""
    import torch
    N = jt._native
    enc = jt.get_encoding("cl100k_base")
    texts = [b"hello w\xc3\xb6rld", b"second document"]
    r = cr.Ref(texts)
    x = torch.zeros(64, dtype=torch.int64, device="cuda")
    d_text, d_off = _dev(np.concatenate([r.text, np.zeros(32, dtype=np.uint8)])), _dev(r.doc_off)
    torch.cuda.synchronize()
    p = x.data_ptr()
    b = enc.new_batch()

    def refused(fn):
        with pytest.raises(jt.EncodingError) as e:
            fn()
        assert e.value.code == N.JTK_ERR_INVALID_ARGUMENT

    def all_four(check):
        check(lambda: b.char_index("char", p))
        check(lambda: b.char_positions("char", p, 1, p + 64))
        check(lambda: b.byte_positions("char", p, p + 64, 1, p + 128))
        check(lambda: b.token_char_offsets("char", p, p + 256))

    all_four(refused)                                                                           # no encode yet
    b.encode_pieces(r.text, r.doc_off, np.array([0, 6], dtype=np.int64), np.array([5, 11], dtype=np.int64))
    all_four(refused)                                                                           # positions in the decoded stream
    mt = [torch.zeros(8, dtype=dt, device="cuda") for dt in (torch.int32, torch.int64, torch.uint8, torch.int32)]
    b.encode_host(r.text, r.doc_off, ordinary=True)
    torch.cuda.synchronize()
    b.encode_device_max_tokens(d_text.data_ptr(), d_off.data_ptr(), 2, r.n_bytes, 4, *(t.data_ptr() for t in mt), ordinary=True)
    torch.cuda.synchronize()
    all_four(refused)                                                                           # that call leaves no result
    b.encode_host(r.text, r.doc_off, ordinary=True, count_only=True)
    refused(lambda: b.token_char_offsets("char", p, p + 256))                                    # no token ids
    b.char_index("char", p)                                                                     # the others read only the text
    b.char_positions("char", p, 1, p + 64)
    b.byte_positions("char", p, p + 64, 1, p + 128)
    b.encode_host(r.text, r.doc_off, ordinary=True)
    for unit in (3, -1):
        refused(lambda: b.char_index(unit, p))
        refused(lambda: b.char_positions(unit, p, 1, p + 64))
        refused(lambda: b.byte_positions(unit, p, p + 64, 1, p + 128))
        refused(lambda: b.token_char_offsets(unit, p, p + 256))
    refused(lambda: b.char_positions("char", p, 1, p + 64, round=2))
    refused(lambda: b.char_positions("char", None, 1, p + 64))                                   # NULL with a count
    refused(lambda: b.char_positions("char", p, 1, None))
    refused(lambda: b.byte_positions("char", None, p + 64, 1, p + 128))
    refused(lambda: b.byte_positions("char", p, None, 1, p + 128))
    refused(lambda: b.byte_positions("char", p, p + 64, 1, None))
    refused(lambda: b.token_char_offsets("char", None, p + 256))
    refused(lambda: b.char_positions("char", p, -1, p + 64))
    b.char_positions("char", None, 0, None)                                                     # n == 0: nothing to do
    b.byte_positions("char", None, None, 0, None)
    b.char_index("utf16")                                                                       # the build alone
    torch.cuda.synchronize()
    assert np.array_equal(_doc_units(b, "utf16", 2), [11, 15])
    b.encode_host(np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.int64), ordinary=True)       # n_docs == 0
    b.char_index("char", None)
    b.token_char_offsets("char", None, None)
    torch.cuda.synchronize()
    b.close()
    with pytest.raises(ValueError):
        enc.chunk_batch(["a"], 4, unit="graphemes")
    with pytest.raises(ValueError):
        enc.pack_batch(["abc"], 8, train_spans=[[(0, 4)]], span_unit="char")                     # past the text's 3 characters
    with pytest.raises(ValueError):
        enc.pack_batch(["abc", "d"], 8, train_spans=[[(0, 1)]], span_unit="char")                # one list per text


def _strs(batch):
    return [d.decode("utf-8") for d in batch["tok"].docs]


def test_chunk_batch_in_characters(jt, batch, o):
    """chunk_batch(unit="char") / "utf16" on str inputs: the tokens of every unsplit chunk decode to text[start:end]; the
    device-input form agrees with the host-input form."""
    import torch
    enc = jt.get_encoding("cl100k_base")
    texts = _strs(batch)
    r = batch["tok"]
    by_bytes = enc.chunk_batch(texts, 24, ordinary=True)
    n_unsplit = 0
    for name in ("char", "utf16"):
        chunks = enc.chunk_batch(texts, 24, ordinary=True, unit=name)
        flat = []
        for s, per_doc, per_doc_bytes in zip(texts, chunks, by_bytes):
            assert len(per_doc) == len(per_doc_bytes)
            u16 = s.encode("utf-16-le")
            for (toks, start, end, split), (toks_b, _, _, split_b) in zip(per_doc, per_doc_bytes):
                assert toks == toks_b and split == split_b
                flat.append((start, end))
                if split:
                    continue
                n_unsplit += 1
                piece = s[start:end] if name == "char" else u16[2 * start:2 * end].decode("utf-16-le")
                assert piece.encode("utf-8") == o.decode_bytes(toks), (name, start, end)
        dev = enc.chunk_batch_device(_dev(r.text), _dev(r.doc_off), 24, ordinary=True, unit=name)
        torch.cuda.synchronize()
        assert np.array_equal(dev["char_begin"].cpu().numpy(), [x[0] for x in flat]), name
        assert np.array_equal(dev["char_end"].cpu().numpy(), [x[1] for x in flat]), name
        assert dev["byte_begin"].dtype == torch.int64 and len(dev["byte_begin"]) == len(flat)
    assert n_unsplit > 100
    assert "char_begin" not in enc.chunk_batch_device(_dev(r.text), _dev(r.doc_off), 24, ordinary=True)


def test_pack_batch_spans_in_characters(jt, batch):
    """pack_batch(span_unit="char" / "utf16") gives the labels of pack_batch with the same ranges converted to bytes on the
    host."""
    enc = jt.get_encoding("cl100k_base")
    texts = _strs(batch)
    rng = random.Random(12)
    for name in ("char", "utf16"):
        spans, spans_b = [], []
        for s in texts:
            n = len(s) if name == "char" else len(s.encode("utf-16-le")) // 2
            cuts = sorted(rng.randint(0, n) for _ in range(2 * rng.randint(0, 3)))
            if name == "utf16":                                                # (not on a low surrogate: the host conversion is exact)
                u16 = s.encode("utf-16-le")
                cuts = [c - 1 if 0 < c < n and 0xDC <= u16[2 * c + 1] <= 0xDF else c for c in cuts]
                to_bytes = lambda c: len(u16[:2 * c].decode("utf-16-le").encode("utf-8"))
            else:
                to_bytes = lambda c: len(s[:c].encode("utf-8"))
            spans.append([(cuts[2 * i], cuts[2 * i + 1]) for i in range(len(cuts) // 2)])
            spans_b.append([(to_bytes(a), to_bytes(e)) for a, e in spans[-1]])
        kw = dict(sep=EOT, pad_id=-3, ordinary=True, span_rule="any", label_shift=True)
        got = enc.pack_batch(texts, 128, train_spans=spans, span_unit=name, **kw)
        exp = enc.pack_batch(texts, 128, train_spans=spans_b, **kw)
        assert (exp["tok_span"] >= 0).sum() > 100
        assert np.array_equal(got["tok_span"], exp["tok_span"]) and np.array_equal(got["labels"], exp["labels"]), name
        assert np.array_equal(got["rows"], exp["rows"])


def test_encode_batch_with_offsets(jt, batch):
    """begin / end of every token against Python's own decoder: the characters of the bytes before the token (a cut character
    dropped: the index of the character that holds the token's first byte) and up to its end (a cut character counted)."""
    enc = jt.get_encoding("cl100k_base")
    texts = _strs(batch)
    res, begin, end = enc.encode_batch_with_offsets(texts, ordinary=True)
    assert np.array_equal(res.tok_off, batch["tok_off"]) and begin.dtype == np.int64 and len(begin) == batch["n_tok"]
    t = 0
    for x, lens in zip(batch["tok"].docs, batch["doc_lens"]):
        p = 0
        for n in lens:
            q = p + n
            cut = q < len(x) and (x[q] & 0xC0) == 0x80
            assert begin[t] == len(x[:p].decode("utf-8", errors="ignore")), t
            assert end[t] == len(x[:q].decode("utf-8", errors="ignore")) + (1 if cut else 0), t
            p, t = q, t + 1
    assert np.array_equal(begin, batch["tok_exp"][cr.CODEPOINT][0]) and np.array_equal(end, batch["tok_exp"][cr.CODEPOINT][1])
    _, b16, e16 = enc.encode_batch_with_offsets(texts, unit="utf16", ordinary=True)
    assert np.array_equal(b16, batch["tok_exp"][cr.UTF16][0]) and np.array_equal(e16, batch["tok_exp"][cr.UTF16][1])
    _, bb, be = enc.encode_batch_with_offsets(texts, unit="byte", ordinary=True)
    p, q = label_ref.token_positions(batch["doc_lens"], batch["tok"].doc_off)
    doc = np.repeat(np.arange(len(texts)), np.diff(batch["tok_off"]))
    assert np.array_equal(bb, p - batch["tok"].doc_off[doc]) and np.array_equal(be, q - batch["tok"].doc_off[doc])
