"""The shared device primitives of jtokkit_amd/csrc/jtk_device_prims.h at their size edges, through the calls built on them.
S = 16,384 items is one step of the one-workgroup array scan (jtk_block_scan_array: 1024 threads x 16 items); the cases put
S - 1, S, S + 1, 2S and 2S + 1 items through it from chunks, pack, allow-special and decode, put empty documents and sequence
boundaries on the step, tile and lane edges of the offset searches, and run the (count, bytes) pair prefix of the device
maxTokens plan over its blocks of 1024 items.  Every array is compared exactly, against numpy or the plain references
(chunk_ref, pack_ref, special_ref, label_ref) and the oracle.  Batches are drawn from a pool of about 50 short strings, each
encoded once by the oracle; the expected arrays are put together by numpy indexing and cumsum.  Needs a real MI355X (`-m gpu`)."""
import numpy as np
import pytest

import chunk_ref
import label_ref
import oracle_lib
import pack_ref
import special_ref

pytestmark = pytest.mark.gpu

S = 16384            # items per step of the shared scan
TILE = 2048          # tokens per tile of the byte scans (JTK_DEC_TILE)
BLOCK = 4096         # text bytes per find workgroup (JTK_SPECIAL_BLOCK)
PAD = -7
EOT = "<|endoftext|>"

_WORDS = ["a", "the", "hello", "world", "token", "GPU", "x1", "42", "naïve", "日本", "🍕", "été", "...", "I'm", "\n", "  ", "über",
          "한국", "data", "scan"]
# candidates; the pool is those with at most 7 tokens
_TEXTS = [""] + _WORDS + [a + " " + b for a, b in zip(_WORDS, _WORDS[3:])] + \
         [a + " " + b + " " + c for a, b, c in zip(_WORDS, _WORDS[5:], _WORDS[9:])] + \
         ["one two three four five six seven", "1234567890123", "🍕🍕", "a b c d e f g", "they'll say"]


def _expand(mat, cnt, idx):
    """The rows mat[idx[d], :cnt[idx[d]]], back to back."""
    if len(idx) == 0:
        return mat[:0, 0]
    return mat[idx][np.arange(mat.shape[1])[None, :] < cnt[idx][:, None]]


def _ex_cumsum(a):
    out = np.zeros(len(a) + 1, dtype=np.int64)
    np.cumsum(a, out=out[1:])
    return out


class Docs:
    """Distinct documents (bytes) with their expected token lists, and what batches of them are assembled from."""

    def __init__(self, o, docs, toks):
        self.o = o
        self.bytes = list(docs)
        self.toks = [list(t) for t in toks]
        self.blen = np.array([len(b) for b in self.bytes], dtype=np.int64)
        self.cnt = np.array([len(t) for t in self.toks], dtype=np.int64)
        w = max(1, int(self.cnt.max()))
        self.tokmat = np.zeros((len(docs), w), dtype=np.int32)
        self.tlen = np.zeros((len(docs), w), dtype=np.int64)          # byte length of every token
        self.first = np.zeros((len(docs), w), dtype=np.uint8)         # its first byte
        for p, t in enumerate(self.toks):
            self.tokmat[p, :len(t)] = t
            for k, i in enumerate(t):
                bts = o.decode_bytes([i])
                self.tlen[p, k] = len(bts)
                self.first[p, k] = bts[0]
        self.tpos = np.zeros((len(docs), w + 1), dtype=np.int64)      # bytes of the document's tokens before token k
        np.cumsum(self.tlen, axis=1, out=self.tpos[:, 1:])

    def batch(self, idx):
        """text, doc_off, tokens, tok_off of the documents idx[0], idx[1], ..."""
        idx = np.asarray(idx, dtype=np.int64)
        text = np.frombuffer(b"".join([self.bytes[i] for i in idx]), dtype=np.uint8)
        return text, _ex_cumsum(self.blen[idx]), _expand(self.tokmat, self.cnt, idx), _ex_cumsum(self.cnt[idx])

    def token_positions(self, idx, doc_off):
        """Byte position of every token of the batch in its text."""
        return np.repeat(doc_off[:-1], self.cnt[idx]) + _expand(self.tpos, self.cnt, idx)


@pytest.fixture(scope="module")
def jt():
    import jtokkit_amd
    return jtokkit_amd


@pytest.fixture(scope="module")
def enc(jt):
    return jt.get_encoding("cl100k_base")


@pytest.fixture(scope="module")
def pool():
    o = oracle_lib.get("cl100k_base")
    docs = [t.encode("utf-8") for t in _TEXTS]
    toks = [o.encode_ordinary(b) for b in docs]
    keep = [i for i, t in enumerate(toks) if len(t) <= 7]
    p = Docs(o, [docs[i] for i in keep], [toks[i] for i in keep])
    assert len(p.bytes) >= 40 and p.cnt[0] == 0 and p.cnt[1] == 1 and p.cnt.max() == 7
    return p


_IDX = {}


def _edge_idx(pool, n_docs):
    """n_docs documents of the pool (0 to 7 tokens), empty ones at 0, S - 1, S and n_docs - 1; the same for every test."""
    if n_docs not in _IDX:
        idx = np.random.default_rng(n_docs).integers(0, len(pool.bytes), n_docs)
        idx[[i for i in (0, S - 1, S, n_docs - 1) if i < n_docs]] = 0
        _IDX[n_docs] = idx
    return _IDX[n_docs]


def _encode(enc, text, doc_off, tokens, tok_off, b=None, **kw):
    """A batch holding the encode of the text, checked against the expected tokens."""
    b = b or enc.new_batch()
    b.encode_host(text, doc_off, **kw)
    res = b.fetch()
    assert np.array_equal(res.tok_off, tok_off) and np.array_equal(res.tokens, tokens) and (res.status == 0).all()
    return b


def _to_host(t, n):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()[:n]


# ---- chunks: the scan of the per-document counts over n_docs items -------------------------------------------------------
def _chunk_tables(pool, N, ov):
    """Per pool document the chunks of the restatement: count, and [pool, max chunks] s, e, split."""
    lists = [chunk_ref.chunks(pool.first[p, :pool.cnt[p]], N, ov) for p in range(len(pool.bytes))]
    cc = np.array([len(c) for c in lists], dtype=np.int64)
    s, e, sp = (np.zeros((len(lists), max(1, int(cc.max()))), dtype=np.int64) for _ in range(3))
    for p, c in enumerate(lists):
        for k, (cs, ce, csp) in enumerate(c):
            s[p, k], e[p, k], sp[p, k] = cs, ce, csp
    return cc, s, e, sp


@pytest.mark.parametrize("n_docs", [1, S - 1, S, S + 1, 2 * S, 2 * S + 1])
def test_chunk_counts_across_scan_steps(enc, pool, n_docs):
    """jtk_batch_chunk with N = 2, overlap 0 and 1: every field of the fetch, chunk_off in full."""
    idx = _edge_idx(pool, n_docs)
    text, doc_off, tokens, tok_off = pool.batch(idx)
    b = _encode(enc, text, doc_off, tokens, tok_off, ordinary=True)
    for ov in (0, 1):
        cc, s, e, sp = _chunk_tables(pool, 2, ov)
        doc = np.repeat(np.arange(n_docs), cc[idx])
        rows = np.repeat(idx, cc[idx])                                    # the pool document of every chunk
        cs, ce = _expand(s, cc, idx), _expand(e, cc, idx)
        exp = dict(chunk_off=_ex_cumsum(cc[idx]), doc=doc, tok_begin=tok_off[doc] + cs, n_tok=ce - cs,
                   byte_begin=doc_off[doc] + pool.tpos[rows, cs], byte_end=doc_off[doc] + pool.tpos[rows, ce],
                   split=_expand(sp, cc, idx))
        assert b.chunk(2, ov) == len(doc)
        f = b.chunk_fetch()
        for k, v in exp.items():
            assert np.array_equal(f[k], v), (k, ov, np.flatnonzero(f[k] != v)[:5])
    b.close()


# ---- pack: four scans over n_docs units -------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_docs", [S, S + 1])
def test_pack_across_scan_steps(enc, pool, n_docs):
    """Concat and whole rows of L = 8 of the chunk batches: rows, positions, cu_seqlens and seg_doc against pack_ref."""
    idx = _edge_idx(pool, n_docs)
    text, doc_off, tokens, tok_off = pool.batch(idx)
    b = _encode(enc, text, doc_off, tokens, tok_off, ordinary=True)
    docs = [pool.toks[i] for i in idx]
    for whole in (False, True):
        exp = pack_ref.pack(docs, np.zeros(n_docs, dtype=np.int32), 8, whole=whole, pad_id=PAD)
        nr, ns, mx = b.pack(8, whole_docs=whole)
        assert (nr, ns, mx) == (len(exp["rows"]), len(exp["seg_doc"]), exp["max_seqlen"])
        f = b.pack_fetch(PAD)
        for k in ("rows", "positions", "cu_seqlens", "seg_doc"):
            assert np.array_equal(f[k], exp[k]), (k, whole)
    b.close()


def test_token_offsets_on_the_chunk_batch(enc, pool):
    """jtk_batch_token_offsets on the S + 1 batch against numpy positions (28 tiles; empty documents at S - 1 and S)."""
    import torch
    idx = _edge_idx(pool, S + 1)
    text, doc_off, tokens, tok_off = pool.batch(idx)
    b = _encode(enc, text, doc_off, tokens, tok_off, ordinary=True)
    pos = torch.full((len(tokens) + 1,), -1, dtype=torch.int64, device="cuda")
    b.token_offsets(pos.data_ptr())
    got = _to_host(pos, len(tokens) + 1)
    assert got[-1] == -1 and np.array_equal(got[:-1], pool.token_positions(idx, doc_off))
    b.close()


# ---- token offsets and labels: the document search with duplicates at lane and tile edges ----------------------------------
def test_token_offsets_and_spans_on_tile_edges(enc, pool):
    """3 * 2048 + 5 tokens; runs of 1, 2 and 65 empty documents end exactly at token indices 8 (a lane's first token), 2048
    and 4096 (a tile's first token).  Token offsets against numpy positions, token spans against label_ref, three rules."""
    import torch
    rng = np.random.default_rng(7)
    live = np.flatnonzero(pool.cnt > 0)

    def fill(n):                                                        # documents with n tokens in all
        out = []
        while n >= 7:
            out.append(int(rng.choice(live)))
            n -= int(pool.cnt[out[-1]])
        return out + [1] * n                                            # (pool document 1 has one token)
    idx = np.array(fill(8) + [0] + fill(TILE - 8) + [0, 0] + fill(TILE) + [0] * 65 + fill(TILE + 5))
    text, doc_off, tokens, tok_off = pool.batch(idx)
    assert len(tokens) == 3 * TILE + 5
    for n_empty, at in ((1, 8), (2, TILE), (65, 2 * TILE)):
        d = np.flatnonzero((tok_off[:-1] == at) & (pool.cnt[idx] == 0))
        assert len(d) == n_empty and tok_off[d[-1] + 1] == at and pool.cnt[idx[d[-1] + 1]] > 0
    b = _encode(enc, text, doc_off, tokens, tok_off, ordinary=True)
    p = pool.token_positions(idx, doc_off)
    pos = torch.full((len(tokens),), -1, dtype=torch.int64, device="cuda")
    b.token_offsets(pos.data_ptr())
    assert np.array_equal(_to_host(pos, len(tokens)), p)
    end = int(doc_off[-1])
    spans = [(int(p[5]), int(p[9])), (int(p[9]) + 1, int(p[40])), (int(p[TILE - 3]), int(p[TILE + 1])), (int(p[TILE + 1]), int(p[TILE + 1])),
             (int(p[2 * TILE - 1]), int(p[2 * TILE + 2]) + 1), (int(p[3 * TILE]), end)]
    d_b = torch.tensor([s[0] for s in spans], dtype=torch.int64, device="cuda")
    d_e = torch.tensor([s[1] for s in spans], dtype=torch.int64, device="cuda")
    doc_lens = [pool.tlen[i, :pool.cnt[i]] for i in idx]
    for rule in (label_ref.WHOLE, label_ref.START, label_ref.ANY):
        out = torch.full((len(tokens),), -9, dtype=torch.int32, device="cuda")
        b.token_spans(d_b.data_ptr(), d_e.data_ptr(), len(spans), rule, out.data_ptr())
        assert np.array_equal(_to_host(out, len(tokens)), label_ref.token_spans(doc_lens, doc_off, spans, rule)), rule
    b.close()


# ---- allow-special ---------------------------------------------------------------------------------------------------------
def _with_specials(pool, extra):
    """The pool and, behind it, documents that hold special literals (all allowed), encoded by special_ref."""
    specials = oracle_lib.ENCODINGS["cl100k_base"]["specials"]
    amap = {k.encode(): v for k, v in specials.items()}
    docs = [x if isinstance(x, bytes) else x.encode("utf-8") for x in extra]
    toks = [special_ref.encode(pool.o, d, amap, list(amap), ordinary=False) for d in docs]
    return Docs(pool.o, pool.bytes + docs, pool.toks + toks), len(pool.bytes)


@pytest.mark.parametrize("n_sub", [S - 1, S, S + 1])
def test_allow_special_sub_document_scan(enc, pool, n_sub):
    """n_docs + 2 * candidates sub-documents = S - 1, S, S + 1: 100 documents with one allowed literal each (a candidate
    takes two slots), the rest from the pool.  Tokens, tok_off and status against special_ref."""
    n_cand = 100
    n_docs = n_sub - 2 * n_cand
    docs, first = _with_specials(pool, ["x" + EOT + " y", EOT, "hello <|fim_prefix|>world", "日本<|endofprompt|>"])
    idx = np.random.default_rng(n_sub).integers(0, first, n_docs)
    at = np.linspace(0, n_docs - 1, n_cand).astype(np.int64)              # (the first and the last document among them)
    assert len(np.unique(at)) == n_cand
    idx[at] = first + np.arange(n_cand) % 4
    text, doc_off, tokens, tok_off = docs.batch(idx)
    b = enc.new_batch()
    b.set_allowed_special("all")
    _encode(enc, text, doc_off, tokens, tok_off, b=b, allow_special=True).close()


def test_allow_special_block_scan(enc, pool):
    """One batch of S * 4096 + 1 bytes: 16,385 find blocks, the last of one byte.  A literal in the first block, one wholly in
    block S - 1, and one across the boundary between blocks S - 1 and S, whose last byte is the only byte of the last block.
    The text is tiled from eight pages of pool strings; the expected result is tiled per distinct document."""
    n_bytes = S * BLOCK + 1
    rng = np.random.default_rng(11)
    pages = []
    for k in range(8):
        page = b" ".join(pool.bytes[i] for i in rng.integers(1, len(pool.bytes), 700))
        pages.append(page[:3500 + 150 * k].decode("utf-8", "ignore").encode("utf-8"))
    head = EOT.encode() + b" " + pages[0]
    tail_text = b" tail " + EOT.encode() + b" and " + EOT.encode()
    idx, total = [8], len(head)
    while n_bytes - total - len(pages[len(idx) % 8]) > 2 * BLOCK:
        idx.append(len(idx) % 8)
        total += len(pages[idx[-1]])
    fill = n_bytes - total - len(tail_text)
    tail = (b"the cat sat on the mat, " * (fill // 24 + 1))[:fill] + tail_text
    specials = oracle_lib.ENCODINGS["cl100k_base"]["specials"]
    amap = {k.encode(): v for k, v in specials.items()}
    distinct = pages + [head, tail]
    docs = Docs(pool.o, distinct, [special_ref.encode(pool.o, d, amap, list(amap)) for d in distinct])
    idx = np.array(idx + [9])
    text, doc_off, tokens, tok_off = docs.batch(idx)
    assert len(text) == n_bytes and bytes(text[-len(EOT):]) == EOT.encode() and tokens[-1] == specials[EOT]
    b = enc.new_batch()
    b.set_allowed_special("all")
    _encode(enc, text, doc_off, tokens, tok_off, b=b, allow_special=True).close()


# ---- decode: the scan of the tile sizes over S and S + 1 tiles ---------------------------------------------------------------
@pytest.mark.parametrize("extra", [0, 1])
def test_decode_across_scan_steps(enc, pool, extra):
    """n_tok = S * 2048 (+ 1): S (+ 1) tiles.  Ids drawn from the pool's tokens of at most 3 bytes (a block of 2^20 ids, tiled),
    sequence boundaries at token S * 2048 - 1, S * 2048 and n_tok, one unknown id in the last tile.  Expected by numpy: lengths
    by table lookup, cumsum for byte_off, indexing for the bytes."""
    n_tok = S * TILE + extra
    ids_pool = np.unique(pool.tokmat[(pool.tlen > 0) & (pool.tlen <= 3)])
    blen = np.array([len(pool.o.decode_bytes([int(i)])) for i in ids_pool], dtype=np.int64)
    bmat = np.zeros((len(ids_pool), 3), dtype=np.uint8)
    for k, i in enumerate(ids_pool):
        bmat[k, :blen[k]] = np.frombuffer(pool.o.decode_bytes([int(i)]), dtype=np.uint8)
    reps = S * TILE >> 20
    pick = np.random.default_rng(5).integers(0, len(ids_pool), 1 << 20)
    ids = np.tile(ids_pool[pick].astype(np.int32), reps)
    lens = np.tile(blen[pick], reps)
    out = np.tile(_expand(bmat, blen, pick), reps)
    if extra:
        unknown = n_tok - 1                                            # the only token of the last tile; a negative id
        ids = np.append(ids, np.int32(-1))
        lens = np.append(lens, 0)
    else:
        unknown = n_tok - 5                                            # in tile S - 1; an id past the table
        ids[unknown] = 2_000_000
        before = int(lens[:unknown].sum())
        out = np.concatenate([out[:before], out[before + int(lens[unknown]):]])
        lens[unknown] = 0
    seq_off = np.array([0, S * TILE - 1, S * TILE, n_tok], dtype=np.int64)
    byte_off = _ex_cumsum(lens)[seq_off]
    status = np.zeros(3, dtype=np.int32)
    status[np.searchsorted(seq_off, unknown, side="right") - 1] = oracle_lib.ERR_UNKNOWN_TOKEN
    b = enc.new_batch()
    assert b.decode_host(ids, seq_off) == len(out)
    got, got_off, got_status = b.decode_fetch()
    b.close()
    assert np.array_equal(got_off, byte_off) and np.array_equal(got_status, status)
    assert np.array_equal(got, out)


# ---- device maxTokens plan: the (count, bytes) pair prefix and its blocks of 1024 items ---------------------------------------
@pytest.mark.parametrize("n_docs", [1023, 1024, 1025, 4097])
def test_device_max_tokens_plan_blocks(enc, pool, n_docs):
    """maxTokens 3 under encode(): every seventh document empty, a few with a special literal (refused).  Rows, kept, truncated
    and status against the host call jtk_batch_encode_max_tokens on the same input.  (The second step of the scan inside the
    plan would need more than 16.7 M documents; it is the function the chunk cases above take through two steps.)"""
    import torch
    docs, first = _with_specials(pool, ["x" + EOT + " y", EOT])
    idx = np.random.default_rng(n_docs).integers(1, first, n_docs)
    idx[::7] = 0
    idx[[5, n_docs // 2, n_docs - 2]] = [first, first + 1, first]
    text, doc_off, _, _ = docs.batch(idx)
    d_text = torch.from_numpy(np.ascontiguousarray(text)).cuda()
    d_off = torch.from_numpy(doc_off).cuda()
    rows, kept, tr, st = (x.cpu().numpy() for x in enc.encode_batch_max_tokens_device(d_text, d_off, 3, ordinary=False, pad_id=PAD))
    b = enc.new_batch()
    h_rows, h_kept, h_tr, h_st = b.encode_max_tokens(text, doc_off, 3, ordinary=False)
    b.close()
    assert np.array_equal(st, h_st) and (st[[5, n_docs // 2, n_docs - 2]] == oracle_lib.ERR_UNSUPPORTED_SPECIAL).all()
    assert np.array_equal(kept, h_kept) and np.array_equal(tr.astype(np.uint8), h_tr)
    live = np.arange(3)[None, :] < kept[:, None]
    assert np.array_equal(np.where(live, rows, 0), np.where(live, h_rows, 0)) and (rows[~live] == PAD).all()
    assert (kept[::7] == 0).all() and kept.max() == 3
