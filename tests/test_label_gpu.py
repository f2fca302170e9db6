"""jtk_batch_token_spans / jtk_batch_pack_labels and HipEncoding.pack_batch(train_spans=...), pack_batch_device(span_begin=...,
span_end=...), token_spans_device: training labels for the packed rows from byte spans of the text.  Expected values come from
the plain restatement of the rule (tests/label_ref.py) applied to the CPU oracle's tokens and to token byte lengths taken from
the oracle's decode of single ids; nothing the device computes enters them.  Every entry of tok_span and of labels is compared.
Every test here needs a real MI355X (`-m gpu`)."""
import random

import numpy as np
import pytest

import golden_util
import label_ref
import oracle_lib
import pack_ref
import regex_crosscheck as rc
import special_ref

pytestmark = pytest.mark.gpu

EOT = "<|endoftext|>"
EOT_ID = 100257
PAD = -3
IGN = -100
RULES = (("whole", label_ref.WHOLE), ("start", label_ref.START), ("any", label_ref.ANY))
MODES = [(-1, False, False, False), (-1, False, False, True), (-1, False, True, False),
         (EOT_ID, False, False, False), (EOT_ID, False, False, True), (EOT_ID, False, True, False),
         (EOT_ID, True, False, False), (EOT_ID, True, False, True), (EOT_ID, True, True, False)]   # (sep, sep_first, whole, drop)


@pytest.fixture(scope="module")
def jt():
    import jtokkit_amd
    return jtokkit_amd


@pytest.fixture(scope="module")
def o():
    return oracle_lib.get("cl100k_base")


def _pack(texts):
    bs = [t if isinstance(t, (bytes, bytearray)) else t.encode("utf-8") for t in texts]
    doc_off = np.zeros(len(bs) + 1, dtype=np.int64)
    np.cumsum([len(x) for x in bs], out=doc_off[1:])
    text = np.frombuffer(b"".join(bs), dtype=np.uint8) if doc_off[-1] else np.zeros(0, dtype=np.uint8)
    return bs, text, doc_off


_len_cache = {}


def _tok_len(o, specials, t):
    """Decoded byte length of one id: the oracle's decode of the single id, a special id's literal."""
    if t not in _len_cache:
        _len_cache[t] = len(specials[t]) if t in specials else len(o.decode_bytes([t]))
    return _len_cache[t]


def _random_spans(rng, n_bytes, n_spans):
    """Sorted and disjoint; repeated cut points make empty and adjacent spans."""
    cuts = []
    for _ in range(2 * n_spans):
        cuts.append(rng.choice(cuts) if cuts and rng.random() < 0.1 else rng.randint(0, n_bytes))
    cuts.sort()
    return [(cuts[2 * i], cuts[2 * i + 1]) for i in range(n_spans)]


def _edge_spans(p, q, tok_off):
    """Spans that begin and end exactly at tokens 511 / 512 (the wave edge of the span pass), 2047 / 2048 (its tile edge), and at
    the first and the last token of documents that begin and end in the middle of a lane's 8 tokens; one ends a byte inside a
    token."""
    k = next(t for t in range(2049, 2100) if q[t] - p[t] >= 2)                  # a span will end one byte inside token k
    spans = [(p[505], q[511]), (p[512], q[515]), (p[2040], q[2047]), (p[2048], p[k] + 1)]
    mid = [d for d in range(len(tok_off) - 1)
           if tok_off[d] > 2100 and tok_off[d + 1] - tok_off[d] >= 2 and 1 <= tok_off[d] % 8 <= 6 and 1 <= (tok_off[d + 1] - 1) % 8 <= 6]
    assert len(mid) >= 4
    d1, d2, d3, d4 = mid[0], mid[1], mid[-2], mid[-1]
    spans += [(p[tok_off[d1]], q[tok_off[d1]]), (p[tok_off[d2 + 1] - 1], q[tok_off[d2 + 1] - 1]),
              (p[tok_off[d3]], q[tok_off[d3 + 1] - 1]), (p[tok_off[d4]], p[tok_off[d4 + 1] - 1])]
    spans = [(int(a), int(b)) for a, b in spans]
    assert all(a <= b for a, b in spans) and all(spans[i][1] <= spans[i + 1][0] for i in range(len(spans) - 1))
    return spans, k


@pytest.fixture(scope="module")
def batch(o):
    """About 5,000 tokens (more than two 2,048-token tiles): every third golden prompt, fuzz documents, empty documents, a
    3-byte-per-character script and an emoji run (tokens that split characters); the oracle's tokens and their byte lengths; the
    two span sets and the restatement's tok_span for every rule."""
    rng = random.Random(41)
    texts = [r[0] for r in golden_util.load_rows("cl100k_base")][::3]                # (all of them hold ~9,000 tokens)
    texts += ["", "日本語のテキストを書きます。" * 6, "", "\U0001F355\U0001F469‍\U0001F373" * 12, "", ""]
    bs, text, doc_off = _pack(texts)
    docs = [o.encode_ordinary(x) for x in bs]
    while sum(len(d) for d in docs) < 5000:
        t = rc.random_text(rng, rng.randint(0, 80)).encode("utf-8")
        bs.append(t)
        docs.append(o.encode_ordinary(t))
    bs, text, doc_off = _pack(bs)
    n_tok = sum(len(d) for d in docs)
    assert 2 * 2048 < n_tok < 8000
    doc_lens = [[_tok_len(o, {}, t) for t in d] for d in docs]
    assert all(sum(lens) == len(x) for lens, x in zip(doc_lens, bs))          # the tokens decode to the text
    assert any(n < 3 for x, lens in zip(bs, doc_lens) if "日本".encode() in x or "\U0001F355".encode() in x for n in lens)
    tok_off = np.concatenate([[0], np.cumsum([len(d) for d in docs])]).astype(np.int64)
    p, q = label_ref.token_positions(doc_lens, doc_off)
    edges, k = _edge_spans(p, q, tok_off)
    sets = {"edges": edges, "random": _random_spans(rng, int(doc_off[-1]), 300)}
    exp = {(name, rule): label_ref.token_spans(doc_lens, doc_off, spans, rule) for name, spans in sets.items() for _, rule in RULES}
    e = exp[("edges", label_ref.WHOLE)]
    assert e[511] == 0 and e[512] == 1 and e[2047] == 2 and e[2048] == 3 and e[k] == -1 and e[504] == -1 and e[516] == -1
    assert exp[("edges", label_ref.START)][k] == 3 and exp[("edges", label_ref.ANY)][k] == 3
    return dict(bs=bs, text=text, doc_off=doc_off, docs=docs, doc_lens=doc_lens, tok_off=tok_off, sets=sets, exp=exp,
                status=[0] * len(docs))


def _dev_spans(spans):
    import torch
    return (torch.tensor([s[0] for s in spans], dtype=torch.int64).cuda(), torch.tensor([s[1] for s in spans], dtype=torch.int64).cuda())


def test_token_spans_at_wave_tile_and_document_edges(jt, batch):
    """k_lb_spans on host-input and device-input encodes: all three rules, the edge spans and 300 random spans, zero spans."""
    import torch
    enc = jt.get_encoding("cl100k_base")
    n_tok = int(batch["tok_off"][-1])
    b = enc.new_batch()
    b.encode_host(batch["text"], batch["doc_off"], ordinary=True)
    assert b.result()[0] == n_tok
    d_text = torch.from_numpy(np.ascontiguousarray(batch["text"])).cuda()
    d_off = torch.from_numpy(batch["doc_off"]).cuda()
    for name, spans in batch["sets"].items():
        d_b, d_e = _dev_spans(spans)
        for rname, rule in RULES:
            exp = batch["exp"][(name, rule)]
            out = torch.full((n_tok + 1,), 12345, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()                                            # (the library's streams do not wait for torch's)
            b.token_spans(d_b.data_ptr(), d_e.data_ptr(), len(spans), rname, out.data_ptr())
            torch.cuda.synchronize()
            got = out.cpu().numpy()
            assert got[-1] == 12345                                             # nothing past the output
            assert np.array_equal(got[:-1], exp), ("host input", name, rname, np.flatnonzero(got[:-1] != exp)[:10])
            ts, t_off, st = enc.token_spans_device(d_text, d_off, d_b, d_e, rule=rname, ordinary=True)
            torch.cuda.synchronize()
            assert ts.dtype == torch.int32 and np.array_equal(ts.cpu().numpy(), exp), ("device input", name, rname)
            assert np.array_equal(t_off.cpu().numpy(), batch["tok_off"]) and (st.cpu().numpy() == 0).all()
    out = torch.full((n_tok,), 12345, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    b.token_spans(None, None, 0, "whole", out.data_ptr())
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == -1).all()
    # after a chunk plan and after token offsets the byte scan is reused: the same answer
    d_b, d_e = _dev_spans(batch["sets"]["random"])
    b.chunk(64)
    b.token_spans(d_b.data_ptr(), d_e.data_ptr(), d_b.numel(), "any", out.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), batch["exp"][("random", label_ref.ANY)])
    b.close()


def test_token_spans_with_special_tokens_as_ids(jt, o):
    """allowed_special="all": <|endoftext|> is one token that counts its literal; spans that end inside the literal, at its start
    and at its end separate the rules."""
    import torch
    enc = jt.get_encoding("cl100k_base")
    texts = ["head " + EOT + " tail", EOT + EOT, "plain text without one", "x" + EOT, ""]
    bs, text, doc_off = _pack(texts)
    amap = {k.encode(): v for k, v in enc._specials.items()}
    lits = {v: k for k, v in amap.items()}
    docs = [special_ref.encode(o, x, amap) for x in bs]
    assert sum(d.count(EOT_ID) for d in docs) == 4
    doc_lens = [[_tok_len(o, lits, t) for t in d] for d in docs]
    assert all(sum(lens) == len(x) for lens, x in zip(doc_lens, bs))
    a = bs[0].index(EOT.encode())
    z = int(doc_off[1])
    spans = [(0, a + 5), (a + 6, a + len(EOT) + 2), (z, z + len(EOT)), (z + len(EOT) + 3, z + 2 * len(EOT) + 4)]
    d_text, d_off = torch.from_numpy(text.copy()).cuda(), torch.from_numpy(doc_off).cuda()
    d_b, d_e = _dev_spans(spans)
    train = [[(0, a + 5), (a + 6, a + len(EOT) + 2)], [(0, len(EOT)), (len(EOT) + 3, 2 * len(EOT))], [], [], []]
    seen = set()
    for rname, rule in RULES:
        exp = label_ref.token_spans(doc_lens, doc_off, spans, rule)
        seen.add(tuple(exp.tolist()))
        ts, _, st = enc.token_spans_device(d_text, d_off, d_b, d_e, rule=rname, allowed_special="all")
        torch.cuda.synchronize()
        assert (st.cpu().numpy() == 0).all() and np.array_equal(ts.cpu().numpy(), exp), rname
        spans2 = [(0, a + 5), (a + 6, a + len(EOT) + 2), (z, z + len(EOT)), (z + len(EOT) + 3, z + 2 * len(EOT))]
        h = enc.pack_batch(texts, 7, sep=EOT, whole_docs=True, pad_id=PAD, allowed_special="all", train_spans=train, span_rule=rname)
        exp2 = label_ref.token_spans(doc_lens, doc_off, spans2, rule)
        assert np.array_equal(h["tok_span"], exp2), rname
        assert np.array_equal(h["labels"], label_ref.labels(docs, [0] * len(docs), 7, EOT_ID, whole=True, tok_span=exp2, ignore_index=IGN))
    assert len(seen) == 3                                                       # the three rules differ on this input


@pytest.mark.parametrize("L", [1, 7, 128])
def test_labels_every_mode(jt, batch, L):
    """k_lb_pack: the nine pack modes x shift x label_sep x tok_span given / NULL, labels compared whole."""
    import torch
    enc = jt.get_encoding("cl100k_base")
    docs, status = batch["docs"], batch["status"]
    tok_span = batch["exp"][("random", label_ref.WHOLE)]
    assert 0 < (tok_span >= 0).sum() < len(tok_span)
    d_ts = torch.from_numpy(tok_span).cuda()
    torch.cuda.synchronize()
    b = enc.new_batch()
    b.encode_host(batch["text"], batch["doc_off"], ordinary=True)
    for sep, sf, whole, drop in MODES:
        packed = pack_ref.pack(docs, status, L, sep, sf, whole, drop, PAD)
        cu = packed["cu_seqlens"]
        if L == 7:
            # the shapes keep covering the store path's edges: segment boundaries on every residue mod 4 of the flat cell index
            # (the lanes' groups of four cells) and a segment that lies across a 1,024-cell tile edge
            assert set((cu[1:-1] % 4).tolist()) == {0, 1, 2, 3}, (sep, sf, whole, drop)
            edges = np.arange(1024, int(cu[-1]), 1024)
            assert len(edges) >= 3 and np.isin(edges, cu).sum() < len(edges), (sep, sf, whole, drop)
        nr, _, _ = b.pack(L, sep, whole, sf, drop)
        assert nr == packed["rows"].shape[0]
        for ts, d_ptr in ((tok_span, d_ts.data_ptr()), (None, None)):
            for shift in (False, True):
                for label_sep in (False, True):
                    exp = label_ref.labels(docs, status, L, sep, sf, whole, drop, ts, IGN, shift, label_sep, packed=packed)
                    got = b.pack_labels_fetch(d_ptr, IGN, shift, label_sep)
                    what = (L, sep, sf, whole, drop, ts is None, shift, label_sep)
                    assert got.shape == exp.shape and np.array_equal(got, exp), (what, np.argwhere(got != exp)[:10].tolist())
        # the device-output call writes its cells and nothing after them
        out = torch.full((nr * L + 1,), 12345, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        b.pack_labels(d_ts.data_ptr(), IGN, out.data_ptr(), shift=True, label_sep=True)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        exp = label_ref.labels(docs, status, L, sep, sf, whole, drop, tok_span, IGN, True, True, packed=packed)
        assert got[-1] == 12345 and np.array_equal(got[:-1].reshape(exp.shape), exp)
    b.close()


def _doc_spans(rng, bs):
    """Per document up to three sorted byte ranges inside it; some documents get none."""
    out = []
    for x in bs:
        cuts = sorted(rng.randint(0, len(x)) for _ in range(2 * rng.randint(0, 3)))
        out.append([(cuts[2 * i], cuts[2 * i + 1]) for i in range(len(cuts) // 2)])
    return out


def test_public_methods(jt, batch):
    """pack_batch(train_spans=...) and pack_batch_device(span_begin=..., span_end=...): the same labels and tok_span, equal to
    the restatement; the other fields are those of the call without spans; default stream and a side stream."""
    import torch
    enc = jt.get_encoding("cl100k_base")
    bs, text, doc_off = batch["bs"], batch["text"], batch["doc_off"]
    docs, status = batch["docs"], batch["status"]
    train = _doc_spans(random.Random(8), bs)
    spans = [(int(doc_off[d]) + a, int(doc_off[d]) + e) for d, sp in enumerate(train) for a, e in sp]
    d_text, d_off = torch.from_numpy(np.ascontiguousarray(text)).cuda(), torch.from_numpy(doc_off).cuda()
    d_b, d_e = _dev_spans(spans)
    base_keys = {"rows", "positions", "cu_seqlens", "seg_doc", "status", "max_seqlen"}
    for L, whole, rname, rule, shift, label_sep in ((128, True, "whole", label_ref.WHOLE, False, True),
                                                    (7, False, "start", label_ref.START, True, False),
                                                    (128, False, "any", label_ref.ANY, True, True)):
        kw = dict(sep=EOT, whole_docs=whole, pad_id=PAD, ordinary=True)
        lab = dict(span_rule=rname, label_shift=shift, label_sep=label_sep, ignore_index=IGN)
        ts = label_ref.token_spans(batch["doc_lens"], doc_off, spans, rule)
        exp = label_ref.labels(docs, status, L, EOT_ID, False, whole, False, ts, IGN, shift, label_sep)
        plain = enc.pack_batch(bs, L, **kw)
        assert set(plain) == base_keys
        h = enc.pack_batch(bs, L, train_spans=train, **kw, **lab)
        assert set(h) == base_keys | {"labels", "tok_span"}
        assert h["labels"].dtype == np.int32 and h["tok_span"].dtype == np.int32
        assert np.array_equal(h["tok_span"], ts) and np.array_equal(h["labels"], exp), (L, whole, rname)
        for k in ("rows", "positions", "cu_seqlens", "seg_doc"):
            assert np.array_equal(h[k], plain[k]), k
        d_plain = enc.pack_batch_device(d_text, d_off, L, **kw)
        assert set(d_plain) == base_keys
        side = torch.cuda.Stream()
        for stream in (None, side):
            if stream is None:
                dev = enc.pack_batch_device(d_text, d_off, L, span_begin=d_b, span_end=d_e, **kw, **lab)
            else:
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    dev = enc.pack_batch_device(d_text, d_off, L, span_begin=d_b, span_end=d_e, **kw, **lab)
            torch.cuda.synchronize()
            assert set(dev) == base_keys | {"labels", "tok_span"}
            assert np.array_equal(dev["labels"].cpu().numpy(), h["labels"]) and np.array_equal(dev["tok_span"].cpu().numpy(), h["tok_span"])
            for k in ("rows", "positions", "cu_seqlens", "seg_doc"):
                assert np.array_equal(dev[k].cpu().numpy(), plain[k]) and torch.equal(dev[k], d_plain[k]), k
    # an empty list for every document: nothing is trained on
    none = enc.pack_batch(bs[:20], 16, sep=EOT, ordinary=True, train_spans=[[] for _ in range(20)], label_sep=True)
    assert (none["labels"] == IGN).all() and (none["tok_span"] == -1).all()


def test_invalid_arguments(jt, batch):
    """The host path validates the ranges and raises; the library refuses encodes whose tokens have no text positions.  No span
    out of order is ever sent to the device."""
    import torch
    N = jt._native
    enc = jt.get_encoding("cl100k_base")
    texts = ["hello world", "second document"]
    for bad in ([[(5, 3)], []], [[(0, 4), (3, 6)], []], [[(6, 8), (0, 2)], []], [[(0, 12)], []], [[(-1, 2)], []], [[(0, 1)]]):
        with pytest.raises(ValueError):
            enc.pack_batch(texts, 8, train_spans=bad)
    with pytest.raises(ValueError):
        enc.pack_batch(texts, 8, train_spans=[[], []], span_rule="most")
    bs, text, doc_off = _pack(texts)
    d_b, d_e = _dev_spans([(0, 4)])
    out = torch.zeros(64, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    b = enc.new_batch()

    def refused(fn):
        with pytest.raises(jt.EncodingError) as e:
            fn()
        assert e.value.code == N.JTK_ERR_INVALID_ARGUMENT

    b.encode_host(text, doc_off, ordinary=True, count_only=True)
    refused(lambda: b.token_spans(d_b.data_ptr(), d_e.data_ptr(), 1, "whole", out.data_ptr()))
    b.encode_pieces(text, doc_off, np.array([0, 6], dtype=np.int64), np.array([5, 11], dtype=np.int64))
    refused(lambda: b.token_spans(d_b.data_ptr(), d_e.data_ptr(), 1, "whole", out.data_ptr()))
    b.encode_host(text, doc_off, ordinary=True)
    refused(lambda: b.token_spans(d_b.data_ptr(), d_e.data_ptr(), 1, 3, out.data_ptr()))          # an unknown rule
    refused(lambda: b.token_spans(None, d_e.data_ptr(), 1, "whole", out.data_ptr()))             # NULL with a count
    refused(lambda: b.pack_labels(None, IGN, out.data_ptr()))                                    # no pack yet
    b.pack(8)
    rc_ = N.lib().jtk_batch_pack_labels(b._h, None, IGN, 4, out.data_ptr(), None)                 # an unknown flag bit
    assert rc_ == N.JTK_ERR_INVALID_ARGUMENT
    b.token_spans(d_b.data_ptr(), d_e.data_ptr(), 1, "whole", out.data_ptr())                    # and the valid call goes through
    b.pack_labels(out.data_ptr(), IGN, out.data_ptr() + 128)
    torch.cuda.synchronize()
    b.close()
    for args in ((d_b.cpu(), d_e), (d_b, d_e.to(torch.int32)), (d_b, torch.cat([d_e, d_e]))):
        with pytest.raises(ValueError):
            enc.pack_batch_device(torch.from_numpy(text.copy()).cuda(), torch.from_numpy(doc_off).cuda(), 8, span_begin=args[0],
                                  span_end=args[1])
