"""UTF-16 in and out on the device (jtk_utf16.hip through jtk_batch_transcode_utf16_device, jtk_batch_encode_utf16*,
jtk_batch_decode_utf16 and the Python methods on top of them) against the plain restatement tests/utf16_ref.py, on the case set
of tests/utf16_cases.py, whose pairs, 4-byte characters and cut characters sit on the kernels' lane, wave and tile edges
(tests/test_utf16_rules_cpu.py shows the restatement equal to the CPython codecs and the case set complete).  Tokens come from
the CPU oracle applied to the reference's UTF-8 bytes, positions from tests/charpos_ref.py; nothing the device computes enters
an expectation, and every byte, unit, offset and token is compared.  Every test here needs a real MI355X (`-m gpu`)."""
import base64
import os

import numpy as np
import pytest

import charpos_ref as cr
import decode_cases as dc
import decode_rows_ref
import golden_util
import label_ref
import oracle_lib
import utf16_cases as uc
import utf16_ref as ur

pytestmark = pytest.mark.gpu

EOT = "<|endoftext|>"
EOT_ID = 100257
INVALID = -1                                                                 # JTK_ERR_INVALID_ARGUMENT
UNKNOWN = -3                                                                 # JTK_ERR_UNKNOWN_TOKEN


@pytest.fixture(scope="module")
def jt():
    import jtokkit_amd
    return jtokkit_amd


@pytest.fixture(scope="module")
def enc(jt):
    return jt.get_encoding("cl100k_base")


@pytest.fixture(scope="module")
def o():
    return oracle_lib.get("cl100k_base")


@pytest.fixture(scope="module")
def golden():
    return golden_util.load_rows("cl100k_base")


@pytest.fixture(scope="module")
def batch(o, golden):
    """One batch: the E case set with a few golden prompts in its middle -- more than four tiles, every edge of the case set --,
    the reference's UTF-8 text and doc_off for it, and the oracle's tokens of every document of that text.  Computed once."""
    prompts = [ur.str_units(r[0]) for r in golden[::4]]
    docs = uc.e_edge_docs(uc.e_script_docs() + prompts)
    assert uc.e_edges_reached(docs) == uc.E_ALL_EDGES
    units, unit_off = ur.batch_units(docs)
    assert 4 * uc.E_TILE < len(units) < 60000
    utf8, doc_off = ur.encode(units, unit_off)
    texts = [utf8[doc_off[d]:doc_off[d + 1]].tobytes() for d in range(len(docs))]
    toks = [o.encode_ordinary(t) for t in texts]
    assert [o.encode(t) for t in texts] == toks                              # (no special-token literal in the batch)
    tok_off = np.concatenate([[0], np.cumsum([len(t) for t in toks])]).astype(np.int64)
    return dict(docs=docs, units=units, unit_off=unit_off, utf8=utf8, doc_off=doc_off, texts=texts, toks=toks, tok_off=tok_off,
                tokens=np.array([t for d in toks for t in d], dtype=np.int32))


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()                              # (a copy: frombuffer views are read-only)


def _sync():
    import torch
    torch.cuda.synchronize()                                                 # (the library's streams do not wait for torch's)


def _transcode(enc, units, unit_off, shift=0):
    """transcode_utf16_device of host arrays; shift: the units start that many elements into their buffer."""
    import torch
    buf = _dev(np.concatenate([np.full(shift, uc.HI, dtype=np.uint16), units]))
    d_units = buf[shift:]
    assert d_units.numel() == 0 or d_units.data_ptr() % 16 == 2 * shift
    d_off = _dev(unit_off)
    _sync()
    utf8, doc_off = enc.transcode_utf16_device(d_units, d_off)
    torch.cuda.synchronize()
    return utf8.cpu().numpy(), doc_off.cpu().numpy()


def _same_text(got, exp, what):
    (g_text, g_off), (e_text, e_off) = got, exp
    assert np.array_equal(g_off, e_off), (what, "doc_off", np.flatnonzero(g_off != e_off)[:10])
    assert len(g_text) == len(e_text), what
    assert np.array_equal(g_text, e_text), (what, "first wrong byte", int(np.flatnonzero(g_text != e_text)[0]))


@pytest.mark.parametrize("shift", [0, 1, 3])
def test_transcode_equals_reference(enc, batch, shift):
    """Every byte and every doc_off of the batch, from a 16-byte aligned pointer and from pointers 2 and 6 bytes past one."""
    _same_text(_transcode(enc, batch["units"], batch["unit_off"], shift), (batch["utf8"], batch["doc_off"]), shift)


@pytest.mark.parametrize("name", [n for n, _ in uc.e_cases()])
def test_transcode_every_case(enc, name):
    """Every case on its own (the edges at the batch positions they were laid out for; no documents, no units, empty documents
    only), aligned and not."""
    units, unit_off = ur.batch_units(dict(uc.e_cases())[name])
    exp = ur.encode(units, unit_off)
    for shift in (0, 1):
        _same_text(_transcode(enc, units, unit_off, shift), exp, (name, shift))


def test_transcode_documents_inside_a_longer_array(enc):
    """unit_off[0] > 0 and unit_off[n_docs] < n_units: the units outside belong to no document."""
    units = np.array([uc.HI, uc.LO, 0x61, uc.HI, uc.LO, uc.HI, uc.LO, 0x62], dtype=np.uint16)
    text, doc_off = _transcode(enc, units, np.array([1, 4, 6], dtype=np.int64))
    assert text.tobytes() == b"?a???" and doc_off.tolist() == [0, 3, 5]


def _same_tokens(res, batch, what):
    tokens, tok_off, status = res
    assert np.array_equal(tok_off, batch["tok_off"]), (what, "tok_off", np.flatnonzero(tok_off != batch["tok_off"])[:10])
    assert np.array_equal(status, np.zeros(len(batch["docs"]), dtype=np.int32)), (what, "status")
    assert np.array_equal(tokens, batch["tokens"]), (what, "first wrong token", int(np.flatnonzero(tokens != batch["tokens"])[0]))


@pytest.mark.parametrize("ordinary", [True, False])
def test_encode_device_and_host_forms(enc, batch, ordinary):
    """tokens, tok_off and status of both forms equal the oracle's encode_ordinary / encode of the reference's UTF-8 bytes;
    doc_off of the device form equals the reference's."""
    import torch
    r = enc.encode_batch_utf16(batch["units"], batch["unit_off"], ordinary=ordinary)
    _same_tokens((r.tokens, r.tok_off, r.status), batch, ("host", ordinary))
    d_units, d_off = _dev(batch["units"]), _dev(batch["unit_off"])
    _sync()
    tokens, tok_off, status, doc_off = enc.encode_batch_utf16_device(d_units, d_off, ordinary=ordinary)
    torch.cuda.synchronize()
    _same_tokens((tokens.cpu().numpy(), tok_off.cpu().numpy(), status.cpu().numpy()), batch, ("device", ordinary))
    assert np.array_equal(doc_off.cpu().numpy(), batch["doc_off"])


def test_encode_flags(jt, enc, batch):
    """COUNT_ONLY counts, VALIDATE_UTF8 (the transcoded text is always well-formed), TO_HOST refused, and allowed_special on a
    document that holds <|endoftext|>."""
    b = enc.new_batch()
    n_tok = int(batch["tok_off"][-1])
    assert b.encode_utf16_host(batch["units"], batch["unit_off"], ordinary=True, count_only=True) == n_tok
    counts, status = b.fetch_counts()
    assert np.array_equal(counts, np.diff(batch["tok_off"])) and not status.any()
    assert b.encode_utf16_host(batch["units"], batch["unit_off"], ordinary=True, validate=True) == n_tok
    _same_tokens(tuple(getattr(b.fetch(), k) for k in ("tokens", "tok_off", "status")), batch, "validate")
    with pytest.raises(jt.encoding.EncodingError) as e:
        b.encode_utf16_host(batch["units"], batch["unit_off"], ordinary=True, to_host=True)
    assert e.value.code == INVALID
    d_units, d_off = _dev(batch["units"]), _dev(batch["unit_off"])
    _sync()
    with pytest.raises(jt.encoding.EncodingError) as e:
        b.encode_utf16_device(d_units.data_ptr(), d_off.data_ptr(), len(batch["docs"]), len(batch["units"]), ordinary=True, to_host=True)
    assert e.value.code == INVALID
    assert b.encode_utf16_device(d_units.data_ptr(), d_off.data_ptr(), len(batch["docs"]), len(batch["units"]), ordinary=True,
                                 count_only=True) == n_tok
    b.close()
    o = oracle_lib.get("cl100k_base")
    docs = ["before " + EOT + " after \U0001F600" + EOT, "no special here", EOT]
    units, unit_off = ur.batch_units([ur.str_units(t) for t in docs])
    r = enc.encode_batch_utf16(units, unit_off, allowed_special="all")
    exp = []
    for t in docs:
        parts = t.split(EOT)
        exp.append([x for i, p in enumerate(parts) for x in ([EOT_ID] if i else []) + o.encode_ordinary(p)])
    assert [r.doc(d).tolist() for d in range(len(docs))] == exp and not r.status.any()
    r = enc.encode_batch_utf16(units, unit_off)                              # encode(): the literal is refused, per document
    assert r.status.tolist() == [-2, 0, -2]


def _i64(n):
    import torch
    return torch.full((n + 1,), 12345, dtype=torch.int64, device="cuda")


def _get(t):
    import torch
    torch.cuda.synchronize()
    a = t.cpu().numpy()
    assert a[-1] == 12345                                                    # the sentinel behind the output is untouched
    return a[:-1]


def test_post_passes_over_the_owned_text(enc, batch, o):
    """After a UTF-16 encode the batch's own transcoded text is the encode's text: UTF-16 document lengths are the original unit
    counts (lone surrogates and pairs included), token ranges in UTF-16 equal charpos_ref on the transcoded text, and chunks
    equal those after a UTF-8 encode of the same text.  A plain transcode in between does not disturb it."""
    nd, n_tok = len(batch["docs"]), int(batch["tok_off"][-1])
    b = enc.new_batch()
    assert b.encode_utf16_host(batch["units"], batch["unit_off"], ordinary=True) == n_tok
    other = _dev(np.full(5000, 0x20AC, dtype=np.uint16))
    other_off = _dev(np.array([0, 5000], dtype=np.int64))
    _sync()
    assert b.transcode_utf16_device(other.data_ptr(), other_off.data_ptr(), 1, 5000) == 15000
    units = _i64(nd)
    _sync()
    b.char_index("utf16", units.data_ptr())
    assert np.array_equal(_get(units), [len(d) for d in batch["docs"]])
    r = cr.Ref(batch["texts"])
    lens = {}
    doc_lens = [[lens.setdefault(t, len(o.decode_bytes([t]))) for t in d] for d in batch["toks"]]
    p, q = label_ref.token_positions(doc_lens, r.doc_off)
    doc = np.repeat(np.arange(nd), [len(x) for x in doc_lens])
    eb = np.array([r.char_index(int(d), int(x), cr.UTF16, cr.FLOOR) for d, x in zip(doc, p)], dtype=np.int64)
    ee = np.array([r.char_index(int(d), int(x), cr.UTF16, cr.CEIL) for d, x in zip(doc, q)], dtype=np.int64)
    begin, end = _i64(n_tok), _i64(n_tok)
    _sync()
    b.token_char_offsets("utf16", begin.data_ptr(), end.data_ptr())
    gb, ge = _get(begin), _get(end)
    assert np.array_equal(gb, eb), np.flatnonzero(gb != eb)[:10]
    assert np.array_equal(ge, ee), np.flatnonzero(ge != ee)[:10]
    # every token's UTF-16 range lies inside its document's original units
    assert (ge <= np.repeat([len(d) for d in batch["docs"]], [len(x) for x in doc_lens])).all()
    b.chunk(48, 5)
    got = b.chunk_fetch()
    b8 = enc.new_batch()
    b8.encode_host(batch["utf8"], batch["doc_off"], ordinary=True)
    b8.chunk(48, 5)
    exp = b8.chunk_fetch()
    assert len(exp["doc"]) > nd
    for k in exp:
        assert np.array_equal(got[k], exp[k]), k
    b.close()
    b8.close()


def test_bad_offsets(jt, enc):
    """The host form refuses negative, decreasing and past-the-end offsets before any launch; the device form finds decreasing
    offsets on the device (all of them inside [0, n_units]: no read can leave the buffer whether or not the check works); an odd
    units pointer is refused."""
    units = np.arange(0x41, 0x41 + 64, dtype=np.uint16)
    b = enc.new_batch()
    for off in ([-1, 10, 64], [0, 40, 30, 64], [0, 10, 65]):
        with pytest.raises((ValueError, jt.encoding.EncodingError)):
            b.encode_utf16_host(units, np.array(off, dtype=np.int64), ordinary=True)
    d_units = _dev(units)
    for off in ([0, 40, 30, 64], [10, 5], [64, 0, 64]):
        d_off = _dev(np.array(off, dtype=np.int64))
        _sync()
        for call in (b.transcode_utf16_device, b.encode_utf16_device):
            with pytest.raises(jt.encoding.EncodingError) as e:
                call(d_units.data_ptr(), d_off.data_ptr(), len(off) - 1, 64)
            assert e.value.code == INVALID, off
    d_off = _dev(np.array([0, 32], dtype=np.int64))
    _sync()
    with pytest.raises(jt.encoding.EncodingError) as e:
        b.transcode_utf16_device(d_units.data_ptr() + 1, d_off.data_ptr(), 1, 32)
    assert e.value.code == INVALID
    assert b.transcode_utf16_device(d_units.data_ptr(), d_off.data_ptr(), 1, 32) == 32      # the batch works on
    b.close()


# ---- out
def test_decode_golden_token_lists(enc, golden):
    rows = golden[::3]
    assert enc.decode_batch_utf16([r[1] for r in rows]) == [r[0] for r in rows]
    assert enc.decode_batch_utf16([]) == [] and enc.decode_batch_utf16([[], []]) == ["", ""]


@pytest.fixture(scope="module")
def byte_ids():
    """The id of every single-byte token of cl100k_base, from the rank file."""
    cfg = oracle_lib.ENCODINGS["cl100k_base"]
    ids = {}
    for line in open(os.path.join(oracle_lib.DATA_DIR, cfg["file"]), "rb"):
        tok, rank = line.split()
        raw = base64.b64decode(tok)
        if len(raw) == 1:
            ids[raw[0]] = int(rank)
    assert len(ids) == 256
    return ids


def test_decode_malformed_sequences(enc, byte_ids):
    """The D case set spelled with single-byte tokens -- more than three tiles of bytes; every row of Table 3-7 cut every way,
    the never-leads, characters across lane, wave, tile and sequence edges: units and unit_off equal the reference, every unit
    compared.  A sequence with an unknown id keeps its status and transcodes what was decoded."""
    seqs = dict(uc.d_cases())["all"]
    assert uc.d_edges_reached(seqs) == uc.D_ALL_EDGES
    lists = [[byte_ids[x] for x in s] for s in seqs]
    bad = len(lists)
    lists.append([byte_ids[0xE2], byte_ids[0x82], 200000, byte_ids[0xAC], byte_ids[0xF0]])   # an id outside the table inside a character
    seqs = seqs + [b"\xe2\x82\xac\xf0"]
    text, byte_off = ur.batch_bytes(seqs)
    exp, exp_off = ur.decode(text, byte_off)
    seq_off = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    b = enc.new_batch()
    assert b.decode_host(np.array([i for x in lists for i in x], dtype=np.int32), seq_off) == len(text)
    assert b.decode_utf16() == len(exp)
    units, unit_off, status = b.decode_utf16_fetch()
    assert np.array_equal(unit_off, exp_off), np.flatnonzero(unit_off != exp_off)[:10]
    assert np.array_equal(units, exp), int(np.flatnonzero(units != exp)[0])
    assert status[bad] == UNKNOWN and not status[:bad].any()
    b.close()
    strs = enc.decode_batch_utf16(lists, strict=False)
    assert strs == [s.decode("utf-8", "replace") for s in seqs]


@pytest.mark.parametrize("name", [n for n, _ in uc.d_cases()])
def test_decode_every_case(enc, byte_ids, name):
    """Every D case on its own: no sequences, empty ones, one byte, whole granules, the edges at the positions they were laid
    out for."""
    seqs = dict(uc.d_cases())[name]
    text, byte_off = ur.batch_bytes(seqs)
    exp, exp_off = ur.decode(text, byte_off)
    b = enc.new_batch()
    b.decode_host(np.array([byte_ids[x] for x in text], dtype=np.int32), byte_off)
    assert b.decode_utf16() == len(exp)
    units, unit_off, _ = b.decode_utf16_fetch()
    assert np.array_equal(unit_off, exp_off) and np.array_equal(units, exp), name
    b.close()


@pytest.mark.parametrize("dtype", [np.int32, np.int64])
def test_decode_rows(enc, byte_ids, golden, dtype):
    """decode_rows_utf16_device with a pad id and a stop id, int32 and int64 rows, against decode_rows_ref + utf16_ref."""
    import torch
    pad = byte_ids[0x00]
    lists = [[byte_ids[x] for x in s] for s in uc.d_bad_seqs() + uc.d_cut_seqs()[::5]] + [r[1] for r in golden[::40]]
    lists = [x + [EOT_ID] + x[:3] if i % 3 == 0 else x for i, x in enumerate(lists)]     # a stop id, and ids behind it
    width = max(len(x) for x in lists) + 2
    rows = np.full((len(lists), width), pad, dtype=dtype)
    for r, x in enumerate(lists):
        rows[r, 1:1 + len(x)] = x                                           # a pad in front, pads behind
    e = decode_rows_ref.decode_rows_ref(dc.table("cl100k_base"), rows, pad_id=pad, stop=(EOT_ID,), skip_pad=True)
    exp, exp_off = ur.decode(np.frombuffer(e["out"], dtype=np.uint8), e["byte_off"])
    assert (exp == 0xFFFD).any() and len(exp) > 500
    d_rows = _dev(rows)
    _sync()
    out = enc.decode_rows_utf16_device(d_rows, pad_id=pad, stop=(EOT_ID,))
    torch.cuda.synchronize()
    assert np.array_equal(out["unit_off"].cpu().numpy(), exp_off)
    assert np.array_equal(out["units"].cpu().numpy(), exp)
    assert np.array_equal(out["status"].cpu().numpy(), e["status"])
    assert np.array_equal(out["bytes"].cpu().numpy(), np.frombuffer(e["out"], dtype=np.uint8))
