"""Plain restatement of the two transcoding rules of jtokkit_amd/csrc/jtk_utf16_rules.h, in loops over units and bytes: no codec
calls, no windows packed into words, no tiles.  E is String.getBytes(UTF_8) per document of UTF-16 units; D is
new String(bytes, UTF_8) per sequence of bytes.  Used by the CPU tier (against the CPython codecs, and against the header
through tests/utf16_sim) and by the GPU tier."""
import numpy as np


def _is_high(u):
    return 0xD800 <= u <= 0xDBFF


def _is_low(u):
    return 0xDC00 <= u <= 0xDFFF


def encode_doc(units):
    """One document's units (a sequence of ints) -> its bytes."""
    out = bytearray()
    n = len(units)
    i = 0
    while i < n:
        u = int(units[i])
        if u < 0x80:
            out.append(u)
        elif u < 0x800:
            out += bytes((0xC0 | u >> 6, 0x80 | u & 0x3F))
        elif _is_high(u) and i + 1 < n and _is_low(int(units[i + 1])):
            c = 0x10000 + ((u - 0xD800) << 10) + (int(units[i + 1]) - 0xDC00)
            out += bytes((0xF0 | c >> 18, 0x80 | c >> 12 & 0x3F, 0x80 | c >> 6 & 0x3F, 0x80 | c & 0x3F))
            i += 1                                                       # the low surrogate of the pair: no bytes
        elif _is_high(u) or _is_low(u):
            out.append(0x3F)
        else:
            out += bytes((0xE0 | u >> 12, 0x80 | u >> 6 & 0x3F, 0x80 | u & 0x3F))
        i += 1
    return bytes(out)


def encode(units, unit_off):
    """E over a batch: (utf8 uint8 array, doc_off int64 [n_docs + 1]).  Units outside [unit_off[0], unit_off[-1]) give nothing."""
    docs = [encode_doc(units[int(unit_off[d]):int(unit_off[d + 1])]) for d in range(len(unit_off) - 1)]
    doc_off = np.zeros(len(unit_off), dtype=np.int64)
    if docs:
        np.cumsum([len(x) for x in docs], out=doc_off[1:])
    return np.frombuffer(b"".join(docs), dtype=np.uint8).copy(), doc_off


def _second_range(b0):
    """(character length, lowest and highest second byte) of the lead b0 by Unicode Table 3-7; None for a byte that leads nothing."""
    if 0xC2 <= b0 <= 0xDF:
        return 2, 0x80, 0xBF
    if 0xE0 <= b0 <= 0xEF:
        return 3, 0xA0 if b0 == 0xE0 else 0x80, 0x9F if b0 == 0xED else 0xBF
    if 0xF0 <= b0 <= 0xF4:
        return 4, 0x90 if b0 == 0xF0 else 0x80, 0x8F if b0 == 0xF4 else 0xBF
    return None


def decode_seq(seq):
    """One sequence's bytes -> its UTF-16 units (a list of ints): a walk that takes one maximal subpart at a time."""
    out = []
    n = len(seq)
    i = 0
    while i < n:
        b0 = seq[i]
        if b0 < 0x80:
            out.append(b0)
            i += 1
            continue
        r = _second_range(b0)
        if r is None:                                                    # a continuation byte on its own, C0, C1, F5..FF
            out.append(0xFFFD)
            i += 1
            continue
        need, lo2, hi2 = r
        got = 1
        while got < need and i + got < n:
            x = seq[i + got]
            if not ((lo2 <= x <= hi2) if got == 1 else (0x80 <= x <= 0xBF)):
                break
            got += 1
        if got < need:
            out.append(0xFFFD)
        else:
            c = b0 & (0x1F if need == 2 else 0x0F if need == 3 else 0x07)
            for x in seq[i + 1:i + need]:
                c = c << 6 | x & 0x3F
            if c >= 0x10000:
                c -= 0x10000
                out += [0xD800 | c >> 10, 0xDC00 | c & 0x3FF]
            else:
                out.append(c)
        i += got
    return out


def decode(text, byte_off):
    """D over a batch: (units uint16 array, unit_off int64 [n_seqs + 1])."""
    raw = bytes(bytearray(text))
    seqs = [decode_seq(raw[int(byte_off[q]):int(byte_off[q + 1])]) for q in range(len(byte_off) - 1)]
    unit_off = np.zeros(len(byte_off), dtype=np.int64)
    if seqs:
        np.cumsum([len(x) for x in seqs], out=unit_off[1:])
    return np.array([u for s in seqs for u in s], dtype=np.uint16), unit_off


def batch_units(docs):
    """Lists of units -> (units uint16, unit_off int64)."""
    unit_off = np.zeros(len(docs) + 1, dtype=np.int64)
    if docs:
        np.cumsum([len(d) for d in docs], out=unit_off[1:])
    return np.array([u for d in docs for u in d], dtype=np.uint16), unit_off


def batch_bytes(seqs):
    """Byte strings -> (text uint8, byte_off int64)."""
    byte_off = np.zeros(len(seqs) + 1, dtype=np.int64)
    if seqs:
        np.cumsum([len(s) for s in seqs], out=byte_off[1:])
    return np.frombuffer(b"".join(seqs), dtype=np.uint8).copy(), byte_off


def str_units(s):
    """A Python str (lone surrogates allowed) -> its UTF-16 units."""
    return np.frombuffer(s.encode("utf-16-le", "surrogatepass"), dtype=np.uint16).tolist()
