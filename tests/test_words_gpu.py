"""jtk_batch_word_stats and the Python surface on it (Batch.word_stats, word_stats_batch, word_stats_batch_device,
quality_signals): a table of small cases, each on an edge of the kernels' partition (the constants jtokkit_amd._native exports),
every output equal to the plain restatement tests/words_ref.py exactly -- the pass is integer arithmetic only -- through host
input, device input and a count-only encode, with and without JTK_WORDS_FOLD_ASCII.  Every test needs a real MI355X (`-m gpu`).
The characters are code points assigned long before the library's Unicode 13 tables: U+00AA (Lo), U+00E9, U+4E2D (CJK) and
U+10400 as letters of 2, 3 and 4 bytes, U+2160 (Nl) and U+0660 (Nd), U+0301 (Mn: no letter), U+1F600 (an emoji)."""
import collections

import numpy as np
import pytest

import words_ref as wr
from jtokkit_amd import _native as N

pytestmark = pytest.mark.gpu

G, WAVE, TILE, STEP = N.JTK_WD_GRANULE, N.JTK_WD_WAVE_BYTES, N.JTK_WD_TILE, N.JTK_WD_TILE * N.JTK_WD_SCAN_STEP
EDGES = (3 * G, WAVE, TILE, TILE + WAVE, 2 * TILE)               # a granule's, a wave's, a tile's, a wave's inside a tile, a tile's
GOPHER = tuple(w.encode() for w in ("the", "be", "to", "of", "and", "that", "have", "with"))
STOP32 = tuple(("w%d" % i + "xyzxy"[:i % 6]).encode() for i in range(32))          # 2 .. 8 bytes
SHORT = 10
GUARD = 0x5A
Case = collections.namedtuple("Case", "name docs status route stops")


def layout(items, fill=b"ab "):
    """One document: every (position, bytes) item at its byte position, filler words (ending in a blank) in between."""
    out = bytearray()
    for pos, s in sorted(items):
        gap = pos - len(out)
        assert gap >= 0, (pos, len(out))
        out += (fill * (gap // len(fill) + 1))[:gap - 1] + b" " if gap else b""
        out += s
    return bytes(out)


def case(name, docs, status=None, route="ordinary", stops=GOPHER):
    docs = [d.encode() if isinstance(d, str) else d for d in docs]
    return Case(name, docs, status or [0] * len(docs), route, stops)


def cases():
    L4, long_run = "\U00010400".encode(), b"-" * (3 * TILE)
    out = [
        # words across edges: one begins on the last byte before each edge and ends on the first behind it; one ends before, one starts at it
        case("word_straddles", [layout([(e - 1, b"to be ") for e in EDGES])]),
        case("word_ends_before", [layout([(e - 3, b"of and ") for e in EDGES])]),
        # dot runs: lengths 1..7; a run of 3k + 1 across every edge; whole granules, a whole wave and whole tiles of dots
        case("dot_lengths", [" ".join("." * n for n in range(1, 8)), "….. ..… ...…... .…."]),
        case("dot_run_over_edges", [layout([(e - 5, b"." * 10 + b" ") for e in EDGES])]),
        case("dot_granules_wave_tiles", [layout([(G - 1, b"." * (3 * G + 3) + b" x"), (WAVE - 20, b"." * (WAVE + 41) + b" x"), (2 * TILE - 3, b"." * (2 * TILE + 8))])]),
        case("dot_run_cut_by_document", ["..", ".", "....", "..", "a...", "...b"]),
        # stop words
        case("stop_at_document_ends", [w + b" x" for w in GOPHER] + [b"x " + w for w in GOPHER] + list(GOPHER)),
        case("stop_across_edges", [layout([(G * (3 + 2 * i) - 1, w + b" ") for i, w in enumerate(GOPHER)] + [(TILE * (1 + i) - 2, w + b" ") for i, w in enumerate(GOPHER)])]),
        case("stop_8_and_9_bytes", [layout([(1, b"totototo totototot xtotototo totototo"), (3 * G - 7, b"totototo "), (TILE - 7, b"totototot "), (2 * TILE - 4, b"totototo")])],
             stops=GOPHER + (b"totototo", "été".encode(), b"the")),
        case("stop_lookalikes", ["the, bathe then The THE the the. été Été tHe"], stops=GOPHER + (b"totototo", "été".encode(), b"the")),
        case("stop_list_of_32", [b" ".join(STOP32[::3]) + b" w1 W2xy w31xyz w31x W31x w27xyz", b" ".join(STOP32)], stops=STOP32),
        case("stop_list_empty", ["the and of"], stops=()),
        # documents
        case("document_edge_inside_granule", ["the", "the", "#", "#a", "1", "-"]),
        case("empty_documents", ["", "", "to be", "", "", "of", ""]),
        case("refused_by_validate", [b"the cat", b"the \xff and of # ... that", b"to be"], [0, -1, 0], "validate"),
        case("refused_by_special", ["the <|endoftext|> of # ...", "and that", layout([(TILE - 1, b"to be")]), "with <|endoftext|>"], [-1, 0, 0, -1], "encode"),
        # lines
        case("lines", ["  - item\n\t• item\r\n-\n•\nplain...   \r\nend…\t\nsaid \"hi.\"  \nwhy?\r\nno\n \t \n..\nwow!\n" +
                       "abcdefghij\nabcdefghi\n" + "é" * 10 + "\n  " + "é" * 9 + " \n", "", "one line", "\n\n"]),
        # classes: letters of 2, 3 and 4 bytes, a letter number, a digit outside ASCII, a mark, an emoji
        case("classes", ["ª Ⅰ ́ ٠ \U0001F600 中文 é \U00010400 -́- 1́ #\U0001F600# x…y Ⅰ́"]),
    ]
    # a word over three tiles whose only letter (digit) is its first byte, its last byte, or absent
    for what, c in (("letter", b"a"), ("digit", b"7")):
        out += [case("long_word_%s_first" % what, [b"ab , " + c + long_run + b" the"]), case("long_word_%s_last" % what, [b"ab , " + long_run + c + b" the"])]
    out.append(case("long_word_symbols", [b"ab , " + long_run + b" the"]))
    # White_Space of 2 and 3 bytes and a 4-byte letter, split by each edge after each of their bytes
    for name, ch in (("nbsp", "\u00a0"), ("nel", "\u0085"), ("ls", "\u2028"), ("ideographic", "\u3000"), ("letter4", "\U00010400")):
        ch = ch.encode()
        for k in range(1, len(ch)):
            out.append(case("%s_split_%d" % (name, k), [layout([(e - k - 1, b"#" + ch + b"# ") for e in EDGES])]))
    # the edge of a scan step: what is carried from one step of pass B to the next.  The filler is long words of letters and a word
    # of "1-" pairs: a run of digits or of symbols of this size is one the encoder walks slowly or refuses (JTK_MAX_PIECE_BYTES)
    long_fill = b"abcdefghijklmnopqrstuvwxyz" * 2 + b"abcdefghijk "
    for name, probe in (("fwd", b"1---- x"), ("bwd", b"----1 x"), ("dots", b"....... x")):
        out.append(case("scan_step_" + name, [layout([(STEP - 2, probe)], fill=long_fill)]))
    out.append(case("scan_step_letter_behind", [b"1-" * (STEP // 2 + 25) + b"a", b"1-" * 20]))
    return out


CASES = {c.name: c for c in cases()}
_REF = {}


@pytest.fixture(scope="module")
def enc():
    import jtokkit_amd
    return jtokkit_amd.get_encoding("cl100k_base")


def ref(c, fold, short=SHORT):
    """The restatement's result of a case, computed once, shared and left unchanged."""
    key = (c.name, fold, short)
    if key not in _REF:
        _REF[key] = wr.stats(c.docs, c.status, c.stops, fold, short)
        for a in _REF[key].values():
            a.setflags(write=False)
    return _REF[key]


def pack(docs):
    doc_off = np.zeros(len(docs) + 1, dtype=np.int64)
    np.cumsum([len(x) for x in docs], out=doc_off[1:])
    return np.frombuffer(b"".join(docs) + b"\0", dtype=np.uint8)[:-1], doc_off


def encode(enc, c, via, b=None):
    """A batch holding the encode of the case's documents by its route, through host input, device input, or a count-only encode
    of device input.  The statuses the device leaves have the signs the case expects."""
    import torch
    b = b or enc.new_batch()
    kw = dict(ordinary=c.route != "encode", validate=c.route == "validate", count_only=via == "count_only")
    text, doc_off = pack(c.docs)
    if via == "host":
        b.encode_host(text, doc_off, **kw)
    else:
        d_text = torch.zeros(len(text) + 32, dtype=torch.uint8, device="cuda")       # (16-byte aligned, readable past the end)
        d_text[:len(text)].copy_(torch.from_numpy(text.copy()))
        b._keep = (d_text, torch.from_numpy(doc_off).cuda())
        torch.cuda.synchronize()
        b.encode_device(b._keep[0].data_ptr(), b._keep[1].data_ptr(), len(c.docs), len(text), **kw)
    assert (np.sign(b.fetch_counts()[1]) == np.sign(c.status)).all(), (c.name, via)
    return b


def run(b, nd, stops, fold, short=SHORT, want=None, pad=4):
    """word_stats into torch buffers with guard cells around every output; one that was not asked for is checked untouched."""
    import torch
    names = [name for name, _ in wr.OUTS]
    want = names if want is None else want
    bufs = {name: torch.full(((nd + 2 * pad) * np.dtype(dt).itemsize,), GUARD, dtype=torch.uint8, device="cuda") for name, dt in wr.OUTS}
    torch.cuda.synchronize()                 # (the fills run on torch's stream, the pass on the batch's)
    b.word_stats(stops, fold, short, **{name: bufs[name].data_ptr() + pad * np.dtype(dict(wr.OUTS)[name]).itemsize for name in want})
    torch.cuda.synchronize()
    out = {}
    for name, dt in wr.OUTS:
        a = bufs[name].cpu().numpy().view(dt)
        guard = np.frombuffer(bytes([GUARD]) * 8, dtype=dt)[0]
        assert (a[:pad] == guard).all() and (a[pad + nd:] == guard).all() and (name in want or (a == guard).all()), name
        out[name] = a[pad:pad + nd]
    return out


@pytest.mark.parametrize("via", ["host", "device", "count_only"])
@pytest.mark.parametrize("name", list(CASES))
def test_case_equals_restatement(enc, name, via):
    c = CASES[name]
    b = encode(enc, c, via)
    b.line_units("line", True)
    for fold in (False, True):
        got, exp = run(b, len(c.docs), c.stops, fold), ref(c, fold)
        for out, _ in wr.OUTS:
            assert np.array_equal(got[out], exp[out]), (name, via, fold, out, got[out], exp[out])


def test_output_subsets_leave_the_rest_untouched(enc):
    c = CASES["lines"]
    b = encode(enc, c, "host")
    b.line_units("line", True)
    names = [name for name, _ in wr.OUTS]
    for want in ([n] for n in names):
        got = run(b, len(c.docs), c.stops, False, want=want)
        assert np.array_equal(got[want[0]], ref(c, False)[want[0]]), want
    got = run(b, len(c.docs), c.stops, False, short=0, want=["n_short_lines", "n_words", "stop_mask"])
    assert not got["n_short_lines"].any() and np.array_equal(got["n_words"], ref(c, False)["n_words"])
    run(b, len(c.docs), c.stops, False, want=[])


def test_invalid_arguments_write_nothing(enc):
    import jtokkit_amd as jt
    import torch
    c = CASES["lines"]
    nd = len(c.docs)
    b = encode(enc, c, "host")
    buf = torch.full((nd * 8 + 64,), GUARD, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    p = buf.data_ptr() + 16

    def refused(**kw):
        args = dict(stop_words=GOPHER, n_words=p)
        args.update(kw)
        with pytest.raises(jt.EncodingError) as e:
            b.word_stats(**args)
        assert e.value.code == N.JTK_ERR_INVALID_ARGUMENT, kw
    refused(n_words=None, n_lines=p)                             # no line list is held yet
    refused(n_words=None, n_short_lines=p)
    b.line_units("line", False)
    refused(n_words=None, n_lines=p)                             # ... nor is the untrimmed list one
    b.line_units("paragraph", True)
    refused(n_words=None, n_bullet_lines=p)
    for bad in ((b"",), (b"ninebytes",), (b"a b",), ("a b".encode(),), ("　".encode(),), (b"\xff",), (b"\xc3",), (b"x",) * 33):
        refused(stop_words=bad)
    refused(n_words=p + 2)
    refused(n_words=None, word_chars=p + 4)
    refused(n_words=None, n_hash=p + 4)
    refused(n_words=None, stop_mask=p + 1)
    text, doc_off = pack(c.docs)
    b.set_fim(jt.FimParams(0.5, 0.5, seed=1, doc_index_base=0))
    b.encode_host(text, doc_off, ordinary=True, fim=True)
    refused()
    full = doc_off[1:] > doc_off[:-1]
    b.encode_pieces(text, doc_off, doc_off[:-1][full], doc_off[1:][full])
    refused()
    b.encode_host(text, doc_off, ordinary=True)
    b.word_stats(GOPHER, n_words=None)                           # (nothing asked for: nothing to do)
    d_text, d_off = torch.from_numpy(np.concatenate([text, np.zeros(32, np.uint8)])).cuda(), torch.from_numpy(doc_off).cuda()
    rows = torch.zeros(nd * 8, dtype=torch.int32, device="cuda")
    kept, trunc, st = (torch.zeros(nd, dtype=dt, device="cuda") for dt in (torch.int64, torch.uint8, torch.int32))
    torch.cuda.synchronize()
    b.encode_device_max_tokens(d_text.data_ptr(), d_off.data_ptr(), nd, len(text), 8, rows.data_ptr(), kept.data_ptr(), trunc.data_ptr(),
                               st.data_ptr(), ordinary=True)
    refused()
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == GUARD).all()


def test_quality_signals(enc):
    pool = [d for c in CASES.values() if c.route == "ordinary" and not c.name.startswith(("scan_step", "long_word")) for d in c.docs]
    docs = [d for d in pool if len(d) < 3 * TILE][:40]
    assert len(docs) >= 36
    exp = wr.stats(docs, [0] * len(docs), GOPHER, True, 0)
    got = enc.quality_signals(docs, fold_ascii=True)
    frac = lambda num, den: np.where(den > 0, num.astype(np.float64) / np.maximum(den, 1), 0.0)
    nw, nl = exp["n_words"].astype(np.int64), exp["n_lines"].astype(np.int64)
    want = {"n_words": nw, "mean_word_length": frac(exp["word_chars"] - exp["symbol_word_chars"], nw - exp["n_symbol_words"]),
            "hash_to_word": frac(exp["n_hash"], nw), "ellipsis_to_word": frac(exp["n_ellipsis"], nw),
            "bullet_line_fraction": frac(exp["n_bullet_lines"], nl), "ellipsis_line_fraction": frac(exp["n_ellipsis_lines"], nl),
            "terminal_line_fraction": frac(exp["n_terminal_lines"], nl), "alpha_word_fraction": frac(exp["n_alpha_words"], nw),
            "n_stop_words": np.array([bin(int(m)).count("1") for m in exp["stop_mask"]]), "status": np.zeros(len(docs), dtype=np.int32)}
    assert set(got) == set(want)
    for name in want:
        assert np.array_equal(got[name], want[name]), name
    batch = enc.word_stats_batch(docs, fold_ascii=True)
    for name, _ in wr.OUTS:
        assert np.array_equal(batch[name], exp[name]), name
