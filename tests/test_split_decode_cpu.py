"""pretok_split's per-character loop on the CPU (jtk_block_classify.h): the branch-free decode of a lead byte's 4-byte word
against the three-way branch it replaced, for every word, and the block classification (two characters per trip) through
the host simulator on every code point at every shift, on text ends inside a 4-byte character, and on neighbouring blocks
with 0, 1, 2, 3, 21 and 32 decoded characters.
"""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DECODE_SWEEP = r"""
#include <cstdint>
#include <cstdio>
#include "jtk_common.h"
#include "jtk_split_masks.h"
#include "jtk_block_classify.h"
#include "jtk_unicode_tables.h"

// the decode that jtk_block_fix_nonascii had before jtk_decode_lead_word: the reference
static inline uint32_t decode_three_way(uint32_t w) {
    const uint32_t b0 = w & 255u, b1 = (w >> 8) & 0x3Fu, b2 = (w >> 16) & 0x3Fu, b3 = (w >> 24) & 0x3Fu;
    uint32_t cp;
    if (b0 < 0xE0u) cp = ((b0 & 0x1Fu) << 6) | b1;
    else if (b0 < 0xF0u) cp = ((b0 & 0x0Fu) << 12) | (b1 << 6) | b2;
    else cp = ((b0 & 0x07u) << 18) | (b1 << 12) | (b2 << 6) | b3;
    return cp;
}

int main() {
    uint64_t words = 0, bad = 0;
    uint32_t first_bad = 0;
    for (uint32_t b0 = 0xC0u; b0 <= 0xFFu; b0++) {
        for (uint32_t rest = 0; rest < (1u << 24); rest++) {
            const uint32_t w = b0 | rest << 8;
            if (jtk_decode_lead_word(w) != decode_three_way(w)) { if (!bad) first_bad = w; bad++; }
            words++;
        }
    }
    // the loop looks values past U+10FFFF up as U+10FFFF: that has to be class O, as jtk_class_of_cp says of them
    const JtkUcTables u{jtk_uc_stage1_init, jtk_uc_stage2_init};
    const unsigned top = jtk_class_of_cp(u, 0x10FFFFu);
    printf("%llu %llu %08x %u\n", (unsigned long long)words, (unsigned long long)bad, first_bad, top);
    return bad || top != JTK_CLS_O ? 1 : 0;
}
"""


def test_branch_free_decode_equals_three_way_branch(tmp_path):
    """jtk_decode_lead_word(w) == the old if / else-if / else decode for all 64 x 2^24 words whose first byte is
    0xC0..0xFF: malformed continuation bytes, overlong forms, surrogates and leads >= 0xF8 included."""
    src = tmp_path / "decode_sweep.cpp"
    src.write_text(DECODE_SWEEP)
    exe = tmp_path / "decode_sweep"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "jtokkit_amd", "csrc"), "-o", str(exe), str(src)])
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, universal_newlines=True)
    words, bad, first, class_of_top = r.stdout.split()
    assert int(words) == 64 << 24
    assert int(class_of_top) == 0, "U+10FFFF is not class O: the loop's clamp of malformed values needs that"
    assert int(bad) == 0 and r.returncode == 0, "first differing word: " + first


@pytest.fixture(scope="module")
def sim():
    d = os.path.join(ROOT, "tests", "hostsim")
    subprocess.check_call(["make", "-C", d, "-s"])
    L = C.CDLL(os.path.join(d, "libjtk_hostsim.so"))
    L.sim_block_classify_check.restype = C.c_int64
    L.sim_block_classify_check.argtypes = [C.c_int, C.c_char_p, C.c_int64]
    return L


def _differing_blocks(sim, kind, b):
    return sim.sim_block_classify_check(kind, b, len(b))


_EVERY = "".join(chr(c) for c in range(1, 0x110000) if not 0xD800 <= c < 0xE000)


@pytest.mark.parametrize("kind", [1, 0])
def test_every_code_point_at_every_shift(sim, kind):
    """Every code point except the surrogates, with 0..6 ASCII bytes in front: 1-, 2-, 3- and 4-byte characters meet every
    position of their block, and the pairs of one trip are made of every neighbouring two."""
    every = _EVERY.encode("utf-8")
    for shift in range(7):
        assert _differing_blocks(sim, kind, b"abcdef"[:shift] + every) == 0, shift


@pytest.mark.parametrize("kind", [1, 0])
def test_text_ends_inside_a_four_byte_character(sim, kind):
    """The text ends 1, 2 and 3 bytes into a 4-byte character (the words past the end are zero), at every place of the
    character's lead in the last block and the one before."""
    four = "\U0001F600".encode("utf-8")
    for fill in range(0, 130):
        head = (b"word \xce\xb1 " * 20)[:fill]
        if head and head[-1] == 0xCE:
            head = head[:-1] + b" "
        for cut in (1, 2, 3):
            assert _differing_blocks(sim, kind, head + four[:cut]) == 0, (fill, cut)


def _block(n_chars, ch):
    """64 bytes: n_chars copies of ch, then ASCII."""
    b = ch.encode("utf-8") * n_chars
    assert len(b) <= 64
    return b + (b"filler text of plain ASCII words, 64 bytes and more of it ......" * 2)[:64 - len(b)]


@pytest.mark.parametrize("kind", [1, 0])
def test_neighbouring_blocks_with_unequal_character_counts(sim, kind):
    """Blocks with 0, 1, 2, 3, 21 (three-byte) and 32 (two-byte) decoded characters next to each other, in both orders
    and with every kind of character in the short ones: the odd and the even tail of the pair loop."""
    two, three, four = "α", "あ", "\U0001F600"          # none under an all-letters lead byte: all are decoded
    for ch in (two, three, four, "٣", "　"):               # a digit and a space, too: classes N and W
        blocks = [_block(0, ch), _block(1, ch), _block(2, ch), _block(3, ch), _block(21, three), _block(32, two)]
        text = b"".join(blocks)
        assert len(text) == 64 * 6
        assert _differing_blocks(sim, kind, text) == 0
        assert _differing_blocks(sim, kind, b"".join(reversed(blocks))) == 0
        assert _differing_blocks(sim, kind, b"".join(blocks[i] for i in (4, 0, 5, 1, 3, 2))) == 0
    # 16 four-byte characters fill a block; 21 three-byte ones after one ASCII byte end on its last byte
    assert _differing_blocks(sim, kind, _block(16, four) + b"x" + three.encode("utf-8") * 21 + _block(3, two)) == 0
