"""JTK_ENCODE_FIM / fim=: fill-in-the-middle encodes on the device.  Every result is checked against the plain restatement
tests/fim_ref.py -- kind and cuts by the rule, the parts' ids by the CPU oracle's encode_ordinary -- for every document, through
host and device input.  (The oracle takes well-formed text only: an ill-formed part's ids are those of the device's own plain
encode of that part alone, which is what "encoded separately" means.)  Every test here needs a real MI355X (`-m gpu`)."""
import base64
import ctypes as C

import numpy as np
import pytest

import fim_cases as fc
import fim_ref as fr
import golden_util
import oracle_lib
import pack_ref

pytestmark = pytest.mark.gpu

HALF = fc.HALF
ALWAYS = fr.ALWAYS


@pytest.fixture(scope="module")
def jt():
    import jtokkit_amd
    return jtokkit_amd


def fim_ids(name):
    sp = oracle_lib.ENCODINGS[name]["specials"]
    return sp["<|fim_prefix|>"], sp["<|fim_middle|>"], sp["<|fim_suffix|>"]


def pack(docs):
    doc_off = np.zeros(len(docs) + 1, dtype=np.int64)
    if docs:
        np.cumsum([len(x) for x in docs], out=doc_off[1:])
    return (np.frombuffer(b"".join(docs), dtype=np.uint8) if doc_off[-1] else np.zeros(0, dtype=np.uint8)), doc_off


def closed(docs):
    """The documents, with a well-formed one behind them when there are ill-formed ones.  Without validation ill-formed text is
    encoded as the bytes it is, and what a character cut short at the very end of the BATCH counts as depends on the bytes behind
    the text, which are not the caller's: the comparisons here keep such an end out of the batch."""
    return list(docs) + ([b"the end"] if any(not fr.well_formed(x) for x in docs) else [])


def first_difference(got, ref):
    for d in range(len(ref.tok_off) - 1):
        if got.doc(d).tolist() != ref.doc(d).tolist() or got.status[d] != ref.status[d]:
            return d, got.doc(d).tolist()[:12], ref.doc(d).tolist()[:12], int(got.status[d]), int(ref.status[d])
    return None


def kept_where_ok(res):
    """A result without the tokens of the documents that have a negative status."""
    from jtokkit_amd import BatchResult
    docs = [res.doc(d) if res.status[d] >= 0 else res.tokens[:0] for d in range(len(res.status))]
    tok_off = np.zeros(len(docs) + 1, dtype=np.int64)
    np.cumsum([len(x) for x in docs], out=tok_off[1:])
    return BatchResult(np.concatenate(docs + [res.tokens[:0]]).astype(np.int32), tok_off, res.status.copy())


def set_fim(jt, b, seed, base, fim_rate, spm_rate, ids):
    """The parameters as the ABI takes them (rates in units of 2^-32)."""
    N = jt._native
    p = N.FimParamsStruct(seed, base, fim_rate, spm_rate, *ids)
    return N.lib().jtk_batch_set_fim(b._h, C.byref(p))


def device_copy(text, doc_off):
    import torch
    d_text = torch.zeros(len(text) + 32, dtype=torch.uint8, device="cuda")           # (16-byte aligned, readable past the end)
    if len(text):
        d_text[:len(text)].copy_(torch.from_numpy(text.copy()))
    return d_text, torch.from_numpy(doc_off).cuda()


def part_encoder(enc, o, docs, seed, base, fim_rate, spm_rate, unencodable=None):
    """encode(bytes) for fim_ref: the oracle for well-formed parts; for the ill-formed parts of these documents under these
    parameters, the device's plain encode_ordinary of each part as a document of its own (one batch)."""
    ill = set()
    for d, doc in enumerate(docs):
        kind, a, b = fr.transform(doc, seed, base + d, fim_rate, spm_rate)
        for part in ((doc,) if kind == fr.NONE else (doc[:a], doc[a:b], doc[b:])):
            if not fr.well_formed(part):
                ill.add(part)
    ill = sorted(ill)
    table = {}
    if ill:
        res = enc.encode_batch(closed(ill), ordinary=True)
        assert (res.status == 0).all()
        table = {part: res.doc(i).tolist() for i, part in enumerate(ill)}

    def encode(part):
        if part in table:
            return table[part]
        try:
            return o.encode_ordinary(part)
        except oracle_lib.OracleError:
            assert unencodable is not None
            return unencodable
    return encode


def same(got, fim, exp, what=""):
    kind, cut, part_tok = fim
    assert np.array_equal(kind, exp.kind), (what, np.flatnonzero(kind != exp.kind)[:10])
    assert np.array_equal(cut, exp.cut), (what, np.flatnonzero((cut != exp.cut).any(axis=1))[:10])
    assert np.array_equal(got.status, exp.status), (what, np.flatnonzero(got.status != exp.status)[:10])
    assert np.array_equal(part_tok, exp.part_tok), (what, np.flatnonzero((part_tok != exp.part_tok).any(axis=1))[:10])
    assert np.array_equal(got.tok_off, exp.tok_off), (what, np.flatnonzero(got.tok_off != exp.tok_off)[:10])
    assert np.array_equal(got.tokens, exp.tokens), (what, np.flatnonzero(got.tokens != exp.tokens)[:10] if len(got.tokens) == len(exp.tokens) else "length")


def run_both(jt, enc, b, docs, seed, base, fim_rate, spm_rate, ids, exp, what="", validate=False):
    """The same batch through encode_host and encode_device; every document compared."""
    text, doc_off = pack(docs)
    assert set_fim(jt, b, seed, base, fim_rate, spm_rate, ids) == 0
    b.encode_host(text, doc_off, ordinary=True, validate=validate, fim=True)
    same(b.fetch(), b.fim_result(), exp, what + " host")
    d_text, d_off = device_copy(text, doc_off)
    b.encode_device(d_text.data_ptr(), d_off.data_ptr(), len(docs), len(text), ordinary=True, validate=validate, fim=True)
    same(b.fetch(), b.fim_result(), exp, what + " device")


@pytest.mark.parametrize("name", ["cl100k_base", "p50k_edit"])
def test_golden_inputs_and_rule_cases(jt, name):
    enc, o, ids = jt.get_encoding(name), oracle_lib.get(name), fim_ids(name)
    docs = [r[0].encode("utf-8") for r in golden_util.load_rows("cl100k_base")]
    assert len(docs) == 423
    for c in fc.cases():
        docs += c.docs
    b = enc.new_batch()
    for spm_rate in (0, HALF, ALWAYS):
        encode = part_encoder(enc, o, docs, 5, 0, ALWAYS, spm_rate)
        exp = fr.encode_batch(encode, docs, 5, 0, ALWAYS, spm_rate, ids)
        run_both(jt, enc, b, docs, 5, 0, ALWAYS, spm_rate, ids, exp, "spm_rate %d" % spm_rate)
        assert set(exp.kind.tolist()) == ({0, 1}, {0, 1, 2}, {0, 2})[(0, HALF, ALWAYS).index(spm_rate)]
    # every case of the rule under its own parameters
    for c in fc.cases():
        cdocs = closed(c.docs)
        encode = part_encoder(enc, o, cdocs, c.seed, c.base, c.fim_rate, c.spm_rate)
        exp = fr.encode_batch(encode, cdocs, c.seed, c.base, c.fim_rate, c.spm_rate, ids)
        run_both(jt, enc, b, cdocs, c.seed, c.base, c.fim_rate, c.spm_rate, ids, exp, c.name)
    b.close()
    # the public call: floats for the rates, the encoding's own sentinel ids
    res = enc.encode_batch(docs[:60], ordinary=True, fim=jt.FimParams(1.0, 0.5, seed=5))
    exp = fr.encode_batch(part_encoder(enc, o, docs[:60], 5, 0, ALWAYS, HALF), docs[:60], 5, 0, ALWAYS, HALF, ids)
    same(res, (res.fim_kind, res.fim_cut, res.fim_part_tok), exp, "encode_batch")
    # the middle is the last part_tok[d][1] tokens in both layouts
    for d in np.flatnonzero((exp.kind != 0) & (exp.status == 0))[:40]:
        a, c = exp.cut[d]
        mid = res.doc(d)[len(res.doc(d)) - exp.part_tok[d, 1]:].tolist()
        assert mid == o.encode_ordinary(docs[:60][d][a:c])


def test_rate_0_is_the_plain_call(jt):
    """Bit-identical to the same call without the flag: ids, offsets, status.  With validation the statuses are the same and so
    are the tokens of every well-formed document; an offender has no tokens under JTK_ENCODE_FIM (as under
    JTK_ENCODE_ALLOW_SPECIAL), while the plain call leaves it those of its bytes."""
    enc, ids = jt.get_encoding("cl100k_base"), fim_ids("cl100k_base")
    docs = closed([r[0].encode("utf-8") for r in golden_util.load_rows("cl100k_base")] + fc.CONT_ONLY + fc.LONE_LEADS + [b""])
    text, doc_off = pack(docs)
    d_text, d_off = device_copy(text, doc_off)
    b = enc.new_batch()
    assert set_fim(jt, b, 3, 0, 0, HALF, ids) == 0
    for validate in (False, True):
        b.encode_host(text, doc_off, ordinary=True, validate=validate)
        ref = b.fetch()
        if validate:
            ref = kept_where_ok(ref)
        b.encode_host(text, doc_off, ordinary=True, validate=validate, fim=True)
        got = b.fetch()
        assert first_difference(got, ref) is None
        assert got.tokens.tobytes() == ref.tokens.tobytes() and got.tok_off.tobytes() == ref.tok_off.tobytes()
        assert got.status.tobytes() == ref.status.tobytes()
        assert not b.fim_result()[0].any()
        b.encode_device(d_text.data_ptr(), d_off.data_ptr(), len(docs), len(text), ordinary=True, validate=validate, fim=True)
        got = b.fetch()
        assert first_difference(got, ref) is None
        assert got.tokens.tobytes() == ref.tokens.tobytes() and got.tok_off.tobytes() == ref.tok_off.tobytes()
        assert got.status.tobytes() == ref.status.tobytes()
        assert (ref.status == -6).any() == validate
    b.close()


def test_gather_edges(jt):
    """Sentinels on either side of a tile boundary inside a document that crosses it; thousands of tiny documents (many per
    tile, empty parts everywhere); empty parts exactly at tile starts; more documents than one step of the scan takes."""
    enc, o, ids = jt.get_encoding("cl100k_base"), oracle_lib.get("cl100k_base"), fim_ids("cl100k_base")
    count = lambda part: len(o.encode_ordinary(part))
    todo = fc.gather_edge_cases(count) + [fc.tiny_documents(3000), fc.zero_token_parts_at_tile_starts(),
                                          fc.Case("past_one_scan_step", [b"a", b"b", b"\n"] * 5700, 8, 0, HALF, HALF)]
    b = enc.new_batch()
    for c in todo:
        encode = part_encoder(enc, o, c.docs, c.seed, c.base, c.fim_rate, c.spm_rate)
        exp = fr.encode_batch(encode, c.docs, c.seed, c.base, c.fim_rate, c.spm_rate, ids)
        run_both(jt, enc, b, c.docs, c.seed, c.base, c.fim_rate, c.spm_rate, ids, exp, c.name)
        if c.name.startswith("gather_"):
            cell = int(c.name.split("_")[2])
            assert exp.tokens[cell] == ids[2 if "suf" in c.name else 1] and len(exp.tokens) > fc.TILE + 1
    assert len(todo[-1].docs) > 16384 and len(exp.tokens) > 16 * fc.TILE
    b.close()


def test_multi_chunk_equals_single_chunk(jt):
    from jtokkit_amd import corpus
    enc, ids = jt.get_encoding("cl100k_base"), fim_ids("cl100k_base")
    N = jt._native
    text, doc_off = corpus.mixed(300, mean_bytes=1500, seed=12)
    text, doc_off = np.ascontiguousarray(text), np.ascontiguousarray(doc_off, dtype=np.int64)
    n = len(doc_off) - 1
    assert len(text) > 5 * (1 << 16)
    d_text, d_off = device_copy(text, doc_off)
    b = enc.new_batch()
    assert set_fim(jt, b, 17, 0, HALF + HALF // 2, HALF, ids) == 0
    b.encode_device(d_text.data_ptr(), d_off.data_ptr(), n, len(text), ordinary=True, fim=True)
    one, one_fim = b.fetch(), b.fim_result()
    assert set(one_fim[0].tolist()) == {0, 1, 2}
    b.set_option(N.JTK_OPT_CHUNK_BYTES, 1 << 16)
    b.encode_device(d_text.data_ptr(), d_off.data_ptr(), n, len(text), ordinary=True, fim=True)
    many, many_fim = b.fetch(), b.fim_result()
    b.encode_host(text, doc_off, ordinary=True, fim=True)
    host, host_fim = b.fetch(), b.fim_result()
    for got, got_fim in ((many, many_fim), (host, host_fim)):
        assert got.tokens.tobytes() == one.tokens.tobytes() and got.tok_off.tobytes() == one.tok_off.tobytes()
        assert got.status.tobytes() == one.status.tobytes()
        assert all(np.array_equal(x, y) for x, y in zip(got_fim, one_fim))
    b.close()
    # and the single-chunk result is the restatement's (the oracle encodes the parts)
    docs = [text[doc_off[d]:doc_off[d + 1]].tobytes() for d in range(n)]
    o = oracle_lib.get("cl100k_base")
    exp = fr.encode_batch(part_encoder(enc, o, docs, 17, 0, HALF + HALF // 2, HALF), docs, 17, 0, HALF + HALF // 2, HALF, ids)
    same(one, one_fim, exp, "single chunk")


def test_malformed_byte_in_each_part(jt):
    """validate=True judges the whole document: a malformed byte in the prefix, the middle or the suffix gives JTK_ERR_BAD_UTF8 and
    no tokens; the neighbours are unaffected."""
    enc, o, ids = jt.get_encoding("cl100k_base"), oracle_lib.get("cl100k_base"), fim_ids("cl100k_base")
    base_doc = b"The quick brown fox jumps over the lazy dog"
    docs, where = [], []
    for d in range(80):
        kind, a, c = fr.transform(base_doc, 41, d, ALWAYS, HALF)
        spans = (None, (0, a), (a, c), (c, len(base_doc)))[d % 4]
        if spans is None or spans[1] - spans[0] < 1:
            docs.append(base_doc)
            where.append(0)
            continue
        at = (spans[0] + spans[1]) // 2
        docs.append(base_doc[:at] + b"\xff" + base_doc[at + 1:])            # (0xFF is no continuation byte: the cuts stay)
        where.append(d % 4)
        assert fr.transform(docs[-1], 41, d, ALWAYS, HALF) == (kind, a, c)
    assert {1, 2, 3} <= set(where) and where.count(0) >= 20
    exp = fr.encode_batch(part_encoder(enc, o, docs, 41, 0, ALWAYS, HALF), docs, 41, 0, ALWAYS, HALF, ids, validate=True)
    assert [int(s) for s in exp.status] == [-6 if w else 0 for w in where]
    b = enc.new_batch()
    run_both(jt, enc, b, docs, 41, 0, ALWAYS, HALF, ids, exp, "validate", validate=True)
    assert b.result()[2] == -6
    b.close()


def test_byte_missing_from_the_rank_map_in_any_part(jt):
    """A custom rank map that lacks the single byte 'Q': JTK_ERR_UNENCODABLE when the byte is in any part."""
    ranks = {bytes([x]): i for i, x in enumerate(x for x in range(256) if x != ord("Q"))}
    for k, merged in enumerate((b"th", b"he", b" t", b"in", b"er", b"the", b" the")):
        ranks[merged] = 300 + k
    specials = {"<|fim_prefix|>": 1000, "<|fim_middle|>": 1001, "<|fim_suffix|>": 1002}
    enc = jt.new_custom_encoding("no_Q", 1, ranks, specials)
    data = b"\n".join(base64.b64encode(k) + b" " + str(v).encode() for k, v in sorted(ranks.items(), key=lambda kv: kv[1])) + b"\n"
    o = oracle_lib.OracleEncoding("no_Q", 1, data, specials)
    base_doc = b"in the thin ether the other then"
    docs, where = [], set()
    for d in range(60):
        at = (d * 7) % len(base_doc)
        docs.append(base_doc if d % 3 == 0 else base_doc[:at] + b"Q" + base_doc[at + 1:])
        if d % 3:
            kind, a, c = fr.transform(docs[-1], 6, d, ALWAYS, HALF)
            where.add(int(at >= a) + int(at >= c))
    assert where == {0, 1, 2}
    encode = part_encoder(enc, o, docs, 6, 0, ALWAYS, HALF, unencodable=jt._native.JTK_ERR_UNENCODABLE)
    exp = fr.encode_batch(encode, docs, 6, 0, ALWAYS, HALF, (1000, 1001, 1002))
    assert [int(s) for s in exp.status] == [0 if d % 3 == 0 else -12 for d in range(60)]
    res = enc.encode_batch(docs, ordinary=True, fim=jt.FimParams(1.0, 0.5, seed=6))
    same(res, (res.fim_kind, res.fim_cut, res.fim_part_tok), exp, "no_Q")
    enc.close()


def test_count_only_to_host_and_compact(jt):
    enc, ids = jt.get_encoding("cl100k_base"), fim_ids("cl100k_base")
    docs = [r[0].encode("utf-8") for r in golden_util.load_rows("cl100k_base")][:200] + [b"", b"x"]
    text, doc_off = pack(docs)
    d_text, d_off = device_copy(text, doc_off)
    b = enc.new_batch()
    assert set_fim(jt, b, 9, 100, ALWAYS - 1, HALF, ids) == 0
    b.encode_device(d_text.data_ptr(), d_off.data_ptr(), len(docs), len(text), ordinary=True, fim=True)
    full, full_fim = b.fetch(), b.fim_result()
    assert len(full.tokens) > len(docs) * 3
    for run in (lambda: b.encode_host(text, doc_off, ordinary=True, count_only=True, fim=True),
                lambda: b.encode_device(d_text.data_ptr(), d_off.data_ptr(), len(docs), len(text), ordinary=True, count_only=True, fim=True)):
        nt = run()
        counts, status = b.fetch_counts()
        assert nt == len(full.tokens) and np.array_equal(counts, np.diff(full.tok_off)) and np.array_equal(status, full.status)
        assert all(np.array_equal(x, y) for x, y in zip(b.fim_result(), full_fim))
        with pytest.raises(jt.EncodingError):
            b.fetch()
    b.encode_host(text, doc_off, ordinary=True, to_host=True, fim=True)
    h = b.host_result()
    assert h.tokens.tobytes() == full.tokens.tobytes() and h.tok_off.tobytes() == full.tok_off.tobytes()
    assert h.status.tobytes() == full.status.tobytes()
    b.encode_host(text, doc_off, ordinary=True, to_host=True, compact=True, fim=True)
    c = b.host_result_compact()
    assert np.array_equal(c.widen(), full.tokens) and np.array_equal(c.tok_off, full.tok_off) and np.array_equal(c.status, full.status)
    # jtk_batch_compact works on the result as on any other
    import torch
    lo = torch.zeros(len(full.tokens), dtype=torch.int16, device="cuda")
    hi = torch.zeros((len(full.tokens) * (enc.id_bits - 16) + 31) // 32 + 1, dtype=torch.int32, device="cuda")
    b.encode_device(d_text.data_ptr(), d_off.data_ptr(), len(docs), len(text), ordinary=True, fim=True)
    b.compact(lo.data_ptr(), hi.data_ptr())
    torch.cuda.synchronize()
    wide = jt.encoding.widen_ids(lo.cpu().numpy().view(np.uint16), hi.cpu().numpy().view(np.uint32), enc.id_bits, 0, len(full.tokens))
    assert np.array_equal(wide, full.tokens)
    b.close()


def test_refusals(jt):
    N = jt._native
    L = N.lib()
    enc, ids = jt.get_encoding("cl100k_base"), fim_ids("cl100k_base")
    docs = [b"hello world", b"fill in the middle"]
    text, doc_off = pack(docs)
    d_text, d_off = device_copy(text, doc_off)
    b = enc.new_batch()
    nt = C.c_int64(0)
    INV = N.JTK_ERR_INVALID_ARGUMENT
    ORD, FIM = N.JTK_ENCODE_ORDINARY, N.JTK_ENCODE_FIM

    def host(flags):
        return L.jtk_batch_encode(b._h, text.ctypes.data, doc_off.ctypes.data, 2, flags, C.byref(nt))

    def dev(flags):
        return L.jtk_batch_encode_device(b._h, d_text.data_ptr(), d_off.data_ptr(), 2, len(text), flags, None, C.byref(nt))
    # the flag without parameters
    assert host(ORD | FIM) == INV and "jtk_batch_set_fim" in N.last_error()
    assert dev(ORD | FIM) == INV
    # ids that are no specials of the encoding leave the parameters unset
    assert set_fim(jt, b, 1, 0, HALF, HALF, (ids[0], 5, ids[2])) == INV and "middle_id" in N.last_error()
    assert set_fim(jt, b, 1, 0, HALF, HALF, (-1, ids[1], ids[2])) == INV
    assert host(ORD | FIM) == INV
    assert set_fim(jt, b, 1, 0, ALWAYS, HALF, ids) == 0
    assert host(ORD | FIM) == 0
    # NULL clears them
    assert L.jtk_batch_set_fim(b._h, None) == 0 and host(ORD | FIM) == INV
    assert set_fim(jt, b, 1, 0, ALWAYS, HALF, ids) == 0
    # without JTK_ENCODE_ORDINARY, with JTK_ENCODE_ALLOW_SPECIAL
    assert host(FIM) == INV and "JTK_ENCODE_ORDINARY" in N.last_error()
    assert dev(FIM) == INV
    assert host(ORD | FIM | N.JTK_ENCODE_ALLOW_SPECIAL) == INV and dev(ORD | FIM | N.JTK_ENCODE_ALLOW_SPECIAL) == INV
    # a refused call leaves the last result alone
    assert host(ORD | FIM) == 0
    assert host(FIM) == INV and b.fim_result()[0].tolist() != []
    # every other entry point that takes flags
    pb, pe = np.array([0], dtype=np.int64), np.array([5], dtype=np.int64)
    assert L.jtk_batch_encode_pieces(b._h, text.ctypes.data, doc_off.ctypes.data, 2, pb.ctypes.data, pe.ctypes.data, 1, ORD | FIM, C.byref(nt)) == INV
    out = np.zeros(64, dtype=np.int32)
    assert L.jtk_encode(b._h, text.ctypes.data, 5, ORD | FIM, -1, out.ctypes.data, 64, C.byref(nt), None) == INV
    rows, kept, flag, status = np.zeros((2, 8), dtype=np.int32), np.zeros(2, dtype=np.int64), np.zeros(2, dtype=np.uint8), np.zeros(2, dtype=np.int32)
    assert L.jtk_batch_encode_max_tokens(b._h, text.ctypes.data, doc_off.ctypes.data, 2, ORD | FIM, 8, rows.ctypes.data, kept.ctypes.data,
                                         flag.ctypes.data, status.ctypes.data) == INV
    import torch
    d_rows, d_kept = torch.zeros((2, 8), dtype=torch.int32, device="cuda"), torch.zeros(2, dtype=torch.int64, device="cuda")
    d_flag, d_status = torch.zeros(2, dtype=torch.uint8, device="cuda"), torch.zeros(2, dtype=torch.int32, device="cuda")
    assert L.jtk_batch_encode_device_max_tokens(b._h, d_text.data_ptr(), d_off.data_ptr(), 2, len(text), ORD | FIM, 8, -1, d_rows.data_ptr(),
                                                d_kept.data_ptr(), d_flag.data_ptr(), d_status.data_ptr(), None) == INV
    units = np.frombuffer("hello".encode("utf-16-le"), dtype=np.uint16)
    unit_off = np.array([0, 5], dtype=np.int64)
    assert L.jtk_batch_encode_utf16(b._h, units.ctypes.data, unit_off.ctypes.data, 1, ORD | FIM, C.byref(nt)) == INV
    svc = C.c_void_p()
    assert L.jtk_service_create(enc._h, 1, C.byref(svc)) == 0
    trunc = C.c_int(0)
    assert L.jtk_service_encode(svc, text.ctypes.data, 5, ORD | FIM, -1, out.ctypes.data, 64, C.byref(nt), C.byref(trunc)) == INV
    L.jtk_service_destroy(svc)
    # after a FIM encode token positions are no positions in the text: the passes that need them refuse, each with a message
    assert host(ORD | FIM) == 0
    d_pos = torch.zeros(64, dtype=torch.int64, device="cuda")
    d_span = torch.zeros(64, dtype=torch.int32, device="cuda")
    nc = C.c_int64(0)
    for rc in (L.jtk_batch_chunk(b._h, 4, 0, None, C.byref(nc)),
               L.jtk_batch_chunk_prefer(b._h, 4, 0, 1, 15, None, C.byref(nc)),
               L.jtk_batch_token_offsets(b._h, d_pos.data_ptr(), None),
               L.jtk_batch_token_spans(b._h, d_pos.data_ptr(), d_pos.data_ptr(), 0, N.JTK_SPAN_WHOLE, d_span.data_ptr(), None),
               L.jtk_batch_char_index(b._h, N.JTK_UNIT_CODEPOINT, None, None),
               L.jtk_batch_token_char_offsets(b._h, N.JTK_UNIT_CODEPOINT, d_pos.data_ptr(), None, None),
               L.jtk_batch_truncate(b._h, 4)):
        assert rc == INV and "JTK_ENCODE_FIM" in N.last_error()
    # ... and work again after a plain encode; the FIM arrays are gone with the FIM result
    assert host(ORD) == 0
    assert L.jtk_batch_chunk(b._h, 4, 0, None, C.byref(nc)) == 0 and L.jtk_batch_truncate(b._h, 4) == 0
    a, c, e = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert L.jtk_batch_fim_result(b._h, C.byref(a), C.byref(c), C.byref(e)) == INV
    assert L.jtk_batch_fim_result_fetch(b._h, None, None, None) == INV
    b.close()
    # Python: no sentinels in the encoding, encode() instead of encode_ordinary(), spans
    with pytest.raises(ValueError):
        jt.get_encoding("r50k_base").encode_batch(["abc"], ordinary=True, fim=jt.FimParams(1.0))
    with pytest.raises(ValueError):
        enc.encode_batch(["abc"], ordinary=False, fim=jt.FimParams(1.0))
    with pytest.raises(ValueError):
        enc.encode_batch(["abc"], ordinary=True, allowed_special="all", fim=jt.FimParams(1.0))
    with pytest.raises(ValueError):
        enc.pack_batch(["abc"], 8, ordinary=True, fim=jt.FimParams(1.0), train_spans=[[(0, 1)]])
    # explicit ids for an encoding without the literals
    r = jt.get_encoding("r50k_base").encode_batch(["hello world"], ordinary=True, fim=jt.FimParams(1.0, 0.0, 1, prefix_id=50256, middle_id=50256, suffix_id=50256))
    assert r.fim_kind.tolist() == [1] and (r.tokens == 50256).sum() == 3


def test_pack_batch_with_fim(jt):
    """pack_batch(..., fim=) and pack_batch_device(..., fim=) equal tests/pack_ref.py applied to the restatement's ids."""
    import torch
    enc, o, ids = jt.get_encoding("cl100k_base"), oracle_lib.get("cl100k_base"), fim_ids("cl100k_base")
    docs = [r[0].encode("utf-8") for r in golden_util.load_rows("cl100k_base")][:150] + [b"", b"z"]
    fim = jt.FimParams(0.75, 0.5, seed=77, doc_index_base=1000)
    f_rate = fr.rate_u32(0.75)
    exp = fr.encode_batch(part_encoder(enc, o, docs, 77, 1000, f_rate, HALF), docs, 77, 1000, f_rate, HALF, ids)
    assert set(exp.kind.tolist()) == {0, 1, 2}
    eot = oracle_lib.ENCODINGS["cl100k_base"]["specials"]["<|endoftext|>"]
    text, doc_off = pack(docs)
    d_text, d_off = device_copy(text, doc_off)
    for whole in (False, True):
        want = pack_ref.pack(exp.docs, exp.status, 64, sep_id=eot, whole=whole, pad_id=-1)
        got = enc.pack_batch(docs, 64, sep="<|endoftext|>", whole_docs=whole, ordinary=True, fim=fim)
        dev = enc.pack_batch_device(d_text[:len(text)], d_off, 64, sep="<|endoftext|>", whole_docs=whole, ordinary=True, fim=fim)
        torch.cuda.synchronize()
        for key in ("rows", "positions", "cu_seqlens", "seg_doc"):
            assert np.array_equal(got[key], want[key]), (whole, key)
            assert np.array_equal(dev[key].cpu().numpy(), want[key]), (whole, key)
        assert got["max_seqlen"] == want["max_seqlen"] == dev["max_seqlen"]
        for key, e in (("fim_kind", exp.kind), ("fim_cut", exp.cut), ("fim_part_tok", exp.part_tok)):
            assert np.array_equal(got[key], e) and np.array_equal(dev[key].cpu().numpy(), e)


def test_determinism(jt):
    """The same call twice, and on a caller's stream, gives identical bytes."""
    import torch
    from jtokkit_amd import corpus
    enc, ids = jt.get_encoding("cl100k_base"), fim_ids("cl100k_base")
    text, doc_off = corpus.mixed(120, mean_bytes=800, seed=3)
    text, doc_off = np.ascontiguousarray(text), np.ascontiguousarray(doc_off, dtype=np.int64)
    n = len(doc_off) - 1
    d_text, d_off = device_copy(text, doc_off)
    b = enc.new_batch()
    assert set_fim(jt, b, 2024, 7, HALF, HALF, ids) == 0

    def snapshot():
        r = b.fetch()
        return (r.tokens.tobytes(), r.tok_off.tobytes(), r.status.tobytes()) + tuple(x.tobytes() for x in b.fim_result())
    b.encode_device(d_text.data_ptr(), d_off.data_ptr(), n, len(text), ordinary=True, fim=True)
    first = snapshot()
    b.encode_device(d_text.data_ptr(), d_off.data_ptr(), n, len(text), ordinary=True, fim=True)
    assert snapshot() == first
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        b.encode_device(d_text.data_ptr(), d_off.data_ptr(), n, len(text), ordinary=True, fim=True, stream=s.cuda_stream, sync=False)
    s.synchronize()
    assert snapshot() == first
    b.encode_host(text, doc_off, ordinary=True, fim=True)
    assert snapshot() == first
    b2 = enc.new_batch()                                           # another batch, the same parameters
    assert set_fim(jt, b2, 2024, 7, HALF, HALF, ids) == 0
    b2.encode_host(text, doc_off, ordinary=True, fim=True)
    r = b2.fetch()
    assert (r.tokens.tobytes(), r.tok_off.tobytes(), r.status.tobytes()) == first[:3]
    b.close()
    b2.close()
