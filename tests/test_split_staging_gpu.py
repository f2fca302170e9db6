"""pretok_split's staging on the device: which waves copy the Unicode class table into LDS, lanes of one wave with unequal
numbers of characters to decode, characters that straddle block, wave and workgroup edges and end the text, and the
all-letters shortcut that stages nothing -- through Batch.encode_device with torch-owned buffers, bit-exact against the
CPU oracle.  A workgroup of the kernel spans 31,744 bytes of the text and each of its 8 waves 3,968.
"""
import numpy as np
import pytest

import oracle_lib

pytestmark = pytest.mark.gpu

NAMES = ["cl100k_base", "r50k_base"]
WAVE, WG = 3968, 31744
ALPHA, HIRA, CJK4E, EMOJI = "α", "あ", "一", "\U0001F600"     # lead bytes CE, E3, E4, F0: all are decoded
PROSE = ("The quick brown fox doesn't jump over 12 lazy dogs; it's 3,968 bytes to the next wave, they said. "
         "Numbers like 1234567 and words like we'll, I'M and you'd keep every rule busy.\n").encode("ascii")


def _prose(n):
    return (PROSE * (n // len(PROSE) + 1))[:n]


def _put(buf, pos, s):
    """Overwrite bytes of an ASCII text with the UTF-8 form of s at pos (the length stays)."""
    b = s.encode("utf-8")
    assert all(c < 0x80 for c in buf[pos:pos + len(b)])
    buf[pos:pos + len(b)] = b


@pytest.fixture(scope="module")
def jt():
    import jtokkit_amd
    return jtokkit_amd


@pytest.fixture(scope="module", params=NAMES)
def enc_batch(request, jt):
    name = request.param
    return name, jt.get_encoding(name).new_batch()


def _encode(b, raw):
    import torch
    dev = torch.device("cuda:0")
    text = np.frombuffer(bytes(raw), dtype=np.uint8)
    doc_off = np.array([0, len(text)], dtype=np.int64)
    d_text = torch.from_numpy(np.concatenate([text, np.zeros(16, dtype=np.uint8)])).to(dev)
    d_off = torch.from_numpy(doc_off).to(dev)
    torch.cuda.synchronize()
    b.encode_device(d_text.data_ptr(), d_off.data_ptr(), 1, len(text), ordinary=True)
    return b.fetch(), text, doc_off


def _check(enc_batch, raw, what):
    name, b = enc_batch
    bytes(raw).decode("utf-8")                                    # the cases are valid UTF-8
    res, text, doc_off = _encode(b, raw)
    exp_tok, exp_off = oracle_lib.get(name).encode_batch(text, doc_off, threads=4)
    assert np.array_equal(res.tok_off, exp_off), (name, what)
    if not np.array_equal(res.tokens, exp_tok):
        j = int(np.nonzero(res.tokens != exp_tok)[0][0])
        p = len(oracle_lib.get(name).decode_bytes(exp_tok[:j]))
        raise AssertionError("%s %s: token %d differs at byte %d (mod 64: %d, wave %d of workgroup %d)"
                             % (name, what, j, p, p % 64, p % WG // WAVE, p // WG))
    assert int(res.status[0]) == 0, (name, what)


# ---- a. who copies the table

@pytest.mark.parametrize("ch", [ALPHA, HIRA, CJK4E, EMOJI], ids=["U+03B1", "U+3042", "U+4E00", "U+1F600"])
def test_one_wave_needs_the_table(enc_batch, ch):
    """Two workgroups plus 17 bytes of ASCII prose with one character to decode in exactly one wave's span: each of the 8
    waves of the first workgroup, and wave 0 of the last, partial one.  Only that wave (and no other of its workgroup)
    stages the class table; then all 8 waves of the first workgroup carry one."""
    n = 2 * WG + 17
    spots = [wv * WAVE + WAVE // 2 + 5 for wv in range(8)] + [2 * WG + 3]
    for pos in spots:
        raw = bytearray(_prose(n))
        _put(raw, pos, ch)
        _check(enc_batch, raw, "one %r at byte %d" % (ch, pos))
    raw = bytearray(_prose(n))
    for pos in spots[:8]:
        _put(raw, pos, ch)
    _check(enc_batch, raw, "one %r in each of 8 waves" % ch)


# ---- b. unequal trips

def _block(n_chars, ch):
    b = ch.encode("utf-8") * n_chars
    assert len(b) <= 64
    return b + _prose(64 - len(b))


def test_lanes_with_unequal_trips(enc_batch):
    """Adjacent lanes (64-byte blocks) with 0, 1, 2, 21 three-byte, 32 two-byte and 16 four-byte characters to decode, in
    that order and reversed, inside one wave."""
    blocks = [_block(0, HIRA), _block(1, HIRA), _block(2, ALPHA), _block(21, HIRA), _block(32, ALPHA), _block(16, EMOJI)]
    for order, seq in (("up", blocks), ("down", blocks[::-1])):
        raw = bytearray(_prose(WAVE + 640))
        at = 64 * 7
        raw[at:at + 64 * len(seq)] = b"".join(seq)
        _check(enc_batch, raw, "blocks with 0, 1, 2, 21, 32, 16 characters, " + order)


SPLITS = [(ALPHA, 1), (HIRA, 1), (HIRA, 2), (EMOJI, 1), (EMOJI, 2), (EMOJI, 3)]     # 1|1, 1|2, 2|1, 1|3, 2|2, 3|1


def _straddle(raw, edge, ch, before):
    _put(raw, edge - before, ch)


def test_characters_straddle_block_edges(enc_batch):
    """A character over a block edge at every split of its bytes, the six splits at six block edges of one wave."""
    raw = bytearray(_prose(WAVE))
    for i, (ch, before) in enumerate(SPLITS):
        _straddle(raw, 64 * (5 + 4 * i), ch, before)
    _check(enc_batch, raw, "block edges")


def test_characters_straddle_wave_edges(enc_batch):
    """The same over wave edges: the first bytes in the last emitting lane of one wave (and the halo lane of the next), the
    rest in the next wave's first."""
    raw = bytearray(_prose(WG))
    for i, (ch, before) in enumerate(SPLITS):
        _straddle(raw, WAVE * (1 + i), ch, before)
    _check(enc_batch, raw, "wave edges")


def test_characters_straddle_workgroup_edges(enc_batch):
    """The same over workgroup edges: no lane of the character's second workgroup sees its lead outside a halo block."""
    raw = bytearray(_prose(6 * WG + 100))
    for i, (ch, before) in enumerate(SPLITS):
        _straddle(raw, WG * (1 + i), ch, before)
    _check(enc_batch, raw, "workgroup edges")


@pytest.mark.parametrize("edge", [64 * 3, WAVE, WG], ids=["block", "wave", "workgroup"])
def test_character_straddles_the_last_edge_of_the_text(enc_batch, edge):
    """The same with the text ending at the character's last byte: 1, 2 or 3 bytes into the last block."""
    for ch, before in SPLITS:
        raw = bytearray(_prose(edge - before)) + ch.encode("utf-8")
        _check(enc_batch, raw, "text end after %r split %d|%d at %d" % (ch, before, len(ch.encode("utf-8")) - before, edge))


# ---- c. the all-letters shortcut

def test_all_letter_leads_stage_nothing(enc_batch):
    """A text whose only characters outside ASCII have lead bytes whose characters are all letters (U+5000...: E5), so no
    wave stages the table or decodes anything; next to it the same text with one U+3042, which one wave decodes."""
    raw = bytearray(_prose(WG + 2 * WAVE + 29))
    for i, pos in enumerate(range(40, len(raw) - 8, 331)):
        _put(raw, pos, chr(0x5000 + 37 * i) * (1 + i % 3))
    assert not any(b in raw for b in (0xCE, 0xE3, 0xE4, 0xF0))
    _check(enc_batch, raw, "all-letter leads only")
    _put(raw, WAVE * 3 + 100, HIRA)
    _check(enc_batch, raw, "all-letter leads and one U+3042")
