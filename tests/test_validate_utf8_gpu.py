"""JTK_ENCODE_VALIDATE_UTF8 on the device: k_validate_utf8 under every entry point that forwards the flag, against CPython's strict
decoder (tests/validate_ref.py) on the batches of tests/validate_cases.py -- whose coverage of the rule and of the partition's
edges the CPU tier (tests/test_validate_rules_cpu.py) asserts.  For every batch the status of EVERY document equals the
reference, and the flag changes nothing else: tokens and offsets equal those of the same batch encoded without it, and the
tokens of every well-formed document equal the CPU oracle's encode_ordinary.  Every test here needs a real MI355X (`-m gpu`)."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib
import special_ref
import validate_cases as vc
import validate_ref as vr

pytestmark = pytest.mark.gpu

NAME = "cl100k_base"
EOT = b"<|endoftext|>"
BATCHES = dict(vc.batches())
SMALL = [b for n, b in vc.batches() if n.startswith("small_")]
_oracle_tokens = {}


@pytest.fixture(scope="module")
def jt():
    import jtokkit_amd
    return jtokkit_amd


@pytest.fixture(scope="module")
def enc(jt):
    return jt.get_encoding(NAME)


def _oracle(doc):
    if doc not in _oracle_tokens:
        _oracle_tokens[doc] = oracle_lib.get(NAME).encode_ordinary(doc)
    return _oracle_tokens[doc]


def _encode(b, docs, mode, ordinary, validate):
    """One encode of the batch -> (tokens or None, tok_off, status), copies on the host."""
    text, doc_off = vc.pack(docs)
    if mode == "device":
        import torch
        d_text, d_off = torch.from_numpy(text.copy()).cuda(), torch.from_numpy(doc_off).cuda()
        torch.cuda.synchronize()
        b.encode_device(d_text.data_ptr(), d_off.data_ptr(), len(docs), len(text), ordinary, validate=validate)
        r = b.fetch()
        return r.tokens, r.tok_off, r.status
    if mode == "count_only":
        b.encode_host(text, doc_off, ordinary, validate, count_only=True)
        counts, status = b.fetch_counts()
        return None, np.concatenate([[0], np.cumsum(counts)]).astype(np.int64), status
    if mode == "to_host":
        b.encode_host(text, doc_off, ordinary, validate, to_host=True)
        r = b.host_result()
        return r.tokens.copy(), r.tok_off.copy(), r.status.copy()
    assert mode == "host"
    b.encode_host(text, doc_off, ordinary, validate)
    r = b.fetch()
    return r.tokens, r.tok_off, r.status


def _check(b, docs, mode="host", ordinary=True):
    """Every status against the reference; tokens and offsets against the same encode without the flag; the tokens of every
    well-formed document against the oracle.  Returns the statuses."""
    exp = np.array(vr.statuses(docs), dtype=np.int32)
    p_tok, p_off, p_st = _encode(b, docs, mode, ordinary, False)
    tok, off, st = _encode(b, docs, mode, ordinary, True)
    assert len(st) == len(docs) and np.array_equal(st, exp), [(int(d), docs[d], int(st[d]), int(exp[d])) for d in np.flatnonzero(st != exp)[:5]]
    assert len(p_st) == len(docs) and not p_st.any()                         # (no batch of the set holds a special-token literal)
    assert np.array_equal(off, p_off)
    if mode == "count_only":
        assert tok is None
        for d in np.flatnonzero(exp == 0):
            assert off[d + 1] - off[d] == len(_oracle(docs[d])), (d, docs[d])
        return st
    assert np.array_equal(tok, p_tok)
    for d in np.flatnonzero(exp == 0):
        assert tok[off[d]:off[d + 1]].tolist() == _oracle(docs[d]), (d, docs[d])
    return st


# ---- the class product
@pytest.mark.parametrize("mode", ["host", "device"])
def test_class_product(enc, mode):
    docs = BATCHES["class_product"]
    b = enc.new_batch()
    st = _check(b, docs, mode)
    assert int((st == 0).sum()) == vc.N_PRODUCT_GOOD
    b.close()


@pytest.mark.parametrize("mode", ["host", "to_host"])
def test_class_product_slice_as_a_tiny_job(enc, mode):
    """Under 128 KiB: offsets and text go down in one copy; with to_host the status atomics land in pinned host memory."""
    docs = BATCHES["class_product_slice"]
    assert sum(len(d) for d in docs) <= vc.TINY_JOB
    b = enc.new_batch()
    _check(b, docs, mode)
    b.close()


# ---- cut rows, malformed kinds and the partition's edges
@pytest.mark.parametrize("ordinary", [True, False])
@pytest.mark.parametrize("mode", ["host", "device", "count_only", "to_host"])
def test_edges_cuts_and_kinds(enc, mode, ordinary):
    b = enc.new_batch()
    _check(b, BATCHES["edges_cuts_kinds"], mode, ordinary)
    b.close()


@pytest.mark.parametrize("mode", ["host", "device"])
def test_first_and_last_bytes_of_a_batch(enc, mode):
    b = enc.new_batch()
    for docs in SMALL:
        _check(b, docs, mode)
    b.close()


# ---- chunked jobs
def _one_chunk_statuses(enc, docs):
    b = enc.new_batch()
    st = _check(b, docs, "host")
    b.close()
    return st


@pytest.mark.parametrize("in_flight", [1, 2, 3])
def test_chunked_host_job(jt, enc, in_flight):
    docs = BATCHES["chunks"]
    _, doc_off = vc.pack(docs)
    assert len(vc.host_chunk_starts(doc_off, vc.MIN_CHUNK)) == 4
    one = _one_chunk_statuses(enc, docs)
    b = enc.new_batch()
    b.set_option(jt._native.JTK_OPT_HOST_CHUNK_BYTES, vc.MIN_CHUNK)
    b.set_option(jt._native.JTK_OPT_CHUNKS_IN_FLIGHT, in_flight)
    for mode in ("host", "to_host"):
        assert np.array_equal(_check(b, docs, mode), one)
    b.close()


def test_chunked_device_job(jt, enc):
    docs = BATCHES["chunks"]
    _, doc_off = vc.pack(docs)
    assert len(vc.device_chunk_starts(doc_off, vc.MIN_CHUNK)) == 4
    one = _one_chunk_statuses(enc, docs)
    b = enc.new_batch()
    b.set_option(jt._native.JTK_OPT_CHUNK_BYTES, vc.MIN_CHUNK)
    assert np.array_equal(_check(b, docs, "device"), one)
    b.close()


# ---- two codes on one document
def test_the_lower_code_wins(enc):
    """A document with a special-token literal and a bad byte under encode(): JTK_ERR_UNSUPPORTED_SPECIAL (-2) and
    JTK_ERR_BAD_UTF8 (-6) both apply; the status is the lower one, as the header says."""
    docs = [b"a " + EOT + b" \xff", b"\x80" + EOT, EOT + b"\xe4\xb8", b"only " + EOT, b"only \xff", b"fine", b""]
    text, doc_off = vc.pack(docs)
    exp = [-6, -6, -6, -2, -6, 0, 0]
    b = enc.new_batch()
    b.encode_host(text, doc_off, ordinary=False, validate=True)
    assert b.fetch().status.tolist() == exp
    b.set_allowed_special([])                                                # the empty set: the call without the flag
    b.encode_host(text, doc_off, ordinary=False, validate=True, allow_special=True)
    assert b.fetch().status.tolist() == exp
    b.set_allowed_special(None)                                              # every literal allowed: no -2 is left
    b.encode_host(text, doc_off, ordinary=False, validate=True, allow_special=True)
    r = b.fetch()
    assert r.status.tolist() == [-6, -6, -6, 0, -6, 0, 0]
    assert r.doc(3).tolist() == _oracle(b"only ") + [oracle_lib.ENCODINGS[NAME]["specials"]["<|endoftext|>"]]
    b.close()


# ---- allow-special: the sub-documents are the validator's documents
@pytest.mark.parametrize("mode", ["host", "device"])
def test_allow_special_with_the_flag(enc, mode):
    specials = oracle_lib.ENCODINGS[NAME]["specials"]
    amap = {k.encode(): v for k, v in specials.items()}
    fim = b"<|fim_prefix|>"
    docs = [b"\xe4\xb8" + EOT + b"\xad", b"",                                # a character cut by a literal
            b"ab\x80 " + EOT + b" fine " + fim + b" fine", b"",              # bad bytes only before the first literal
            b"fine " + EOT + b" fine " + fim + b" \xf0\x9f\x98", b"",        # ... only after the last
            EOT, b"",                                                        # a document that is one literal
            "日本".encode() + EOT + "語\U0001F600".encode() + fim + "é".encode(), b"",   # literals between multi-byte characters
            b"", EOT + EOT, b"plain", "\U0001F600".encode() + EOT]
    exp = [0 if vr.well_formed(d) else vr.BAD_UTF8 for d in docs]
    assert exp == [-6, 0, -6, 0, -6, 0, 0, 0, 0, 0, 0, 0, 0, 0]
    text, doc_off = vc.pack(docs)
    b = enc.new_batch()
    b.set_allowed_special(None)
    if mode == "device":
        import torch
        d_text, d_off = torch.from_numpy(text.copy()).cuda(), torch.from_numpy(doc_off).cuda()
        torch.cuda.synchronize()
        b.encode_device(d_text.data_ptr(), d_off.data_ptr(), len(docs), len(text), False, allow_special=True, validate=True)
    else:
        b.encode_host(text, doc_off, ordinary=False, validate=True, allow_special=True)
    r = b.fetch()
    assert r.status.tolist() == exp
    for d, doc in enumerate(docs):
        if exp[d]:
            assert r.tok_off[d + 1] == r.tok_off[d], d                       # -6 and no tokens
        else:
            assert r.doc(d).tolist() == special_ref.encode(oracle_lib.get(NAME), doc, amap, list(amap)), (d, doc)
    b.close()


# ---- jtk_encode: one document, the flags forwarded
def test_single_document_entry_point(jt, enc):
    """jtk_encode without a token limit honours the flag: JTK_ERR_BAD_UTF8 as the return value and no tokens for a malformed
    document; with a token limit the flag is ignored (include/jtokkit_amd.h says both)."""
    N = jt._native
    b = enc.new_batch()

    def call(doc, flags, max_tokens=-1):
        out = np.full(len(doc) + 1, -1, dtype=np.int32)
        nt, tr = C.c_int64(-1), C.c_int(-1)
        rc = N.lib().jtk_encode(b._h, doc, len(doc), flags, max_tokens, out.ctypes.data, len(out), C.byref(nt), C.byref(tr))
        return rc, out[:max(nt.value, 0)].tolist(), nt.value

    flags = N.JTK_ENCODE_ORDINARY | N.JTK_ENCODE_VALIDATE_UTF8
    for doc in (b"plain", "café 中文 \U0001f355".encode(), b"\xf4\x8f\xbf\xbf", b"\xe0\xa0\x80", b""):
        assert call(doc, flags) == (N.JTK_OK, _oracle(doc), len(_oracle(doc)))
    for doc in (b"\xff", b"ab\x80", b"\xe4\xb8", b"\xf4\x90\x80\x80", b"\xe0\x9f\xbf", b"\xed\xa0\x80", b"\xf0\x8f\xbf\xbf", b"\xc1\xbf"):
        assert call(doc, flags) == (N.JTK_ERR_BAD_UTF8, [], 0), doc
        rc, toks, nt = call(doc, N.JTK_ENCODE_ORDINARY)                      # without the flag: the bytes as they are
        assert rc == N.JTK_OK and enc.decode_bytes(toks) == doc
        assert call(doc, flags, max_tokens=8)[0] == N.JTK_OK                 # with a token limit the flag is ignored
    b.close()
