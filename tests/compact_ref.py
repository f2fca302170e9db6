"""A plain restatement of the compact-ids format (include/jtokkit_amd.h, "compact token ids"), written independently of
jtokkit_amd/csrc/jtk_compact_rules.h: lo = ids & 0xFFFF; hi = the hb bits above of every token, laid out as one bit stream
(token i at bits [i * hb, (i + 1) * hb), least significant bit first) and cut into little-endian 32-bit words."""
import numpy as np

HB_CHOICES = (0, 1, 2, 4, 8, 16)


def hb_for(max_id):
    """The smallest allowed number of high bits that holds max_id."""
    need = max(int(max_id).bit_length() - 16, 0)
    return next(h for h in HB_CHOICES if h >= need)


def hi_words(n, hb):
    return -(-n * hb // 32)


def compact(ids, hb):
    """(lo uint16 [n], hi uint32 [ceil(n * hb / 32)] or None)."""
    ids = np.asarray(ids, dtype=np.int64)
    assert ids.size == 0 or (ids.min() >= 0 and ids.max() < 1 << (16 + hb))
    lo = (ids % 65536).astype(np.uint16)
    if hb == 0:
        return lo, None
    high = ids // 65536
    bits = ((high[:, None] >> np.arange(hb)) & 1).astype(np.uint8).reshape(-1)        # the bit stream, LSB first per token
    pad = hi_words(len(ids), hb) * 32 - bits.size
    bits = np.concatenate([bits, np.zeros(pad, dtype=np.uint8)])
    by = np.packbits(bits, bitorder="little")                                           # bytes of the stream
    return lo, by.view("<u4").astype(np.uint32)


def widen(lo, hi, hb):
    lo = np.asarray(lo, dtype=np.int64)
    if hb == 0:
        return lo.astype(np.int32)
    bits = np.unpackbits(np.asarray(hi, dtype="<u4").view(np.uint8), bitorder="little")[:len(lo) * hb].reshape(len(lo), hb)
    high = (bits.astype(np.int64) << np.arange(hb)).sum(axis=1)
    return (lo + high * 65536).astype(np.int32)
