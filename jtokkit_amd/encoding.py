"""Host-side mirror of the reference's Encoding interface on top of the C ABI.

Mirrors `com.knuddels.jtokkit.api.Encoding` (reference api/Encoding.java:29-189) method for method
so that parity tests read like the reference's own (reference/Cl100kBaseTestTest.java), plus the
batch entry points that are the reason this library exists.  The JVM is absent from the build image,
so this Python class (and the C++ header jtokkit_amd/csrc/jtk_encoding.hpp) stand where the Java
`HipEncoding implements Encoding` of INTEGRATION.md would.
"""
import contextlib
import ctypes as C
import threading

import numpy as np

from . import _native as N


class UnsupportedOperationError(Exception):
    """java.lang.UnsupportedOperationException (GptBytePairEncoding.java:54)."""


class EncodingError(Exception):
    def __init__(self, code, msg):
        super().__init__("jtokkit_amd error %d: %s" % (code, msg))
        self.code = code


def _check(rc):
    if rc == N.JTK_OK:
        return
    msg = N.last_error()
    if rc == N.JTK_ERR_UNSUPPORTED_SPECIAL:
        raise UnsupportedOperationError("Encoding special tokens is not supported yet.")
    if rc == N.JTK_ERR_UNKNOWN_TOKEN:
        raise ValueError("Unknown token for decoding: " + msg)     # IllegalArgumentException
    if rc == N.JTK_ERR_UNENCODABLE:
        raise ValueError("Unknown token for encoding: " + msg)     # IllegalArgumentException (TokenEncoder.java:66-68)
    if rc == N.JTK_ERR_BAD_RANK_FILE:
        raise RuntimeError(msg)                                    # IllegalStateException
    raise EncodingError(rc, msg)


_hip_memcpy_async = None


def _copy_d2d(dst, src, n_bytes, stream):
    """hipMemcpyAsync(dst, src, n, DeviceToDevice, stream) of the HIP runtime the library is bound to."""
    global _hip_memcpy_async
    if _hip_memcpy_async is None:
        f = N.lib().hipMemcpyAsync                                  # (found through the library's own dependencies)
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
        _hip_memcpy_async = f
    rc = _hip_memcpy_async(dst, src, n_bytes, 3, stream)
    if rc != 0:
        raise EncodingError(N.JTK_ERR_HIP, "hipMemcpyAsync failed (%d)" % rc)


def _device_copy(src_ptr, shape, dtype, device, stream):
    """A new CUDA tensor of the elements at device pointer src_ptr, copied on `stream`; an empty one reads nothing."""
    import torch
    t = torch.empty(shape, dtype=dtype, device=device)
    if t.numel():
        _copy_d2d(t.data_ptr(), src_ptr, t.numel() * t.element_size(), stream)
    return t


def _join_texts(texts):
    """List of str/bytes -> (the documents' bytes, text uint8, doc_off int64 [n + 1]): the documents back to back."""
    bs = [t if isinstance(t, (bytes, bytearray)) else t.encode("utf-8") for t in texts]
    doc_off = np.zeros(len(bs) + 1, dtype=np.int64)
    if bs:
        np.cumsum([len(b) for b in bs], out=doc_off[1:])
    text = np.frombuffer(b"".join(bs), dtype=np.uint8) if doc_off[-1] else np.zeros(0, dtype=np.uint8)
    return bs, text, doc_off


def _join_ids(token_lists):
    """List of token-id lists -> (ids int32, seq_off int64 [n + 1]): the lists back to back."""
    seq_off = np.zeros(len(token_lists) + 1, dtype=np.int64)
    if token_lists:
        np.cumsum([len(t) for t in token_lists], out=seq_off[1:])
    return np.fromiter((i for t in token_lists for i in t), dtype=np.int32, count=int(seq_off[-1])), seq_off


def _view(ptr, n, ctype, dtype):
    """Zero-copy numpy view of n elements at a host pointer (an empty array for none)."""
    if not ptr or n == 0:
        return np.zeros(0, dtype=dtype)
    return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(ctype)), shape=(n,))


def _encode_flags(ordinary=False, validate=False, count_only=False, to_host=False, allow_special=False, compact=False, fim=False):
    """The JTK_ENCODE_* flag word of an encode call."""
    return ((N.JTK_ENCODE_ORDINARY if ordinary else 0) | (N.JTK_ENCODE_VALIDATE_UTF8 if validate else 0)
            | (N.JTK_ENCODE_COUNT_ONLY if count_only else 0) | (N.JTK_ENCODE_TO_HOST if to_host else 0)
            | (N.JTK_ENCODE_ALLOW_SPECIAL if allow_special else 0) | (N.JTK_ENCODE_COMPACT_IDS if compact else 0)
            | (N.JTK_ENCODE_FIM if fim else 0))


_SPAN_RULES = {"whole": N.JTK_SPAN_WHOLE, "start": N.JTK_SPAN_START, "any": N.JTK_SPAN_ANY}


def _span_rule(rule):
    """"whole" / "start" / "any" -> JTK_SPAN_*; an int goes through (the library checks it)."""
    if isinstance(rule, str):
        if rule not in _SPAN_RULES:
            raise ValueError("span rule must be 'whole', 'start' or 'any', not %r" % (rule,))
        return _SPAN_RULES[rule]
    return int(rule)


_UNITS = {"byte": N.JTK_UNIT_BYTE, "utf16": N.JTK_UNIT_UTF16, "char": N.JTK_UNIT_CODEPOINT}
_ROUNDS = {"floor": N.JTK_CHAR_FLOOR, "ceil": N.JTK_CHAR_CEIL}


def _unit(unit):
    """"byte" / "utf16" (indices into a Java String) / "char" (code points: indices into a Python str) -> JTK_UNIT_*; an int
    goes through (the library checks it)."""
    if isinstance(unit, str):
        if unit not in _UNITS:
            raise ValueError("unit must be 'byte', 'utf16' or 'char', not %r" % (unit,))
        return _UNITS[unit]
    return int(unit)


_CUTS = {"word": N.JTK_CUT_WORD, "sentence": N.JTK_CUT_SENTENCE, "line": N.JTK_CUT_LINE, "paragraph": N.JTK_CUT_PARAGRAPH}


def prefer_mask(prefer):
    """An iterable of "word" / "sentence" / "line" / "paragraph", the string "all", or an int mask -> JTK_CUT_* bits (the
    library checks an int)."""
    if isinstance(prefer, str):
        if prefer == "all":
            return 15
        prefer = (prefer,)
    if isinstance(prefer, int):
        return prefer & 0xFFFFFFFF
    mask = 0
    for name in prefer:
        if name not in _CUTS:
            raise ValueError("prefer takes 'word', 'sentence', 'line', 'paragraph' or 'all', not %r" % (name,))
        mask |= _CUTS[name]
    return mask


def _round(rnd):
    if isinstance(rnd, str):
        if rnd not in _ROUNDS:
            raise ValueError("round must be 'floor' or 'ceil', not %r" % (rnd,))
        return _ROUNDS[rnd]
    return int(rnd)


def _stream_sync(stream):
    """hipStreamSynchronize of the HIP runtime the library is bound to."""
    f = N.lib().hipStreamSynchronize
    f.restype, f.argtypes = C.c_int, [C.c_void_p]
    rc = f(stream)
    if rc != 0:
        raise EncodingError(N.JTK_ERR_HIP, "hipStreamSynchronize failed (%d)" % rc)


def _lines_params(unit, trim, mark_first, seed, doc_index_base):
    """jtk_lines_params; unit: "line", "paragraph" or a JTK_LINES_* value."""
    u = {"line": N.JTK_LINES_LINE, "paragraph": N.JTK_LINES_PARAGRAPH}.get(unit, unit)
    if not isinstance(u, int):
        raise ValueError('unit must be "line" or "paragraph"')
    return N.LinesParamsStruct(seed & 0xFFFFFFFFFFFFFFFF, doc_index_base & 0xFFFFFFFFFFFFFFFF, u,
                               (N.JTK_LINES_MARK_FIRST if mark_first else 0) | (N.JTK_LINES_TRIM if trim else 0))


# jtk_lines_out: the arrays per unit, per document + 1 and per document, with their element types
_LINES_PER_UNIT = (("unit_begin", np.int64), ("unit_end", np.int64), ("unit_flags", np.uint8))
_LINES_PER_DOC = (("n_dup", np.int32), ("dup_bytes", np.int64), ("dup_chars", np.int64), ("unit_bytes", np.int64), ("unit_chars", np.int64),
                  ("doc_chars", np.int64), ("top_count", np.int32), ("top_first", np.int64))


def _stop_blob(stop_strings):
    """Stop strings (bytes or str, a str as its UTF-8 bytes; one alone is a list of one) -> (blob uint8, str_off uint32
    [n + 1]).  The library checks counts and lengths."""
    if isinstance(stop_strings, (str, bytes, bytearray)):
        stop_strings = (stop_strings,)
    bs = [s.encode("utf-8") if isinstance(s, str) else bytes(s) for s in stop_strings]
    str_off = np.zeros(len(bs) + 1, dtype=np.uint32)
    if bs:
        np.cumsum([len(x) for x in bs], out=str_off[1:])
    return np.frombuffer(b"".join(bs), dtype=np.uint8), str_off


def fim_rate_u32(rate):
    """A probability as the ABI takes it: units of 2^-32, 0xFFFFFFFF = always."""
    rate = float(rate)
    if not 0.0 <= rate <= 1.0:
        raise ValueError("a FIM rate must be in [0, 1]")
    return min(int(rate * 2 ** 32), 2 ** 32 - 1)


class FimParams:
    """Fill-in-the-middle parameters (jtk_fim_params; the rule is in include/jtokkit_amd.h): rate = the probability that a
    document is cut into prefix, middle and suffix, spm_rate = the probability that a cut document is emitted in SPM order
    (else PSM), seed, and doc_index_base = the corpus index of the batch's first document (a shard then draws what the whole
    corpus would).  prefix_id / middle_id / suffix_id: None = the encoding's <|fim_prefix|> / <|fim_middle|> / <|fim_suffix|>."""

    def __init__(self, rate, spm_rate=0.5, seed=0, doc_index_base=0, prefix_id=None, middle_id=None, suffix_id=None):
        self.rate, self.spm_rate, self.seed, self.doc_index_base = rate, spm_rate, seed, doc_index_base
        self.prefix_id, self.middle_id, self.suffix_id = prefix_id, middle_id, suffix_id
        fim_rate_u32(rate), fim_rate_u32(spm_rate)

    def __repr__(self):
        return "FimParams(rate=%r, spm_rate=%r, seed=%r, doc_index_base=%r)" % (self.rate, self.spm_rate, self.seed, self.doc_index_base)


class _DeviceArray:
    """A numpy array's bytes in device memory of the HIP runtime the library is bound to, for host-input calls whose C entry
    point takes device arrays (no torch needed).  fetch() copies back."""

    def __init__(self, arr):
        self._arr = np.ascontiguousarray(arr)
        self.ptr = C.c_void_p()
        L = N.lib()
        for f, args in ((L.hipMalloc, [C.POINTER(C.c_void_p), C.c_size_t]), (L.hipFree, [C.c_void_p]),
                        (L.hipMemcpy, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int])):
            f.restype, f.argtypes = C.c_int, args
        self._check(L.hipMalloc(C.byref(self.ptr), max(self._arr.nbytes, 16)), "hipMalloc")
        if self._arr.nbytes:
            self._check(L.hipMemcpy(self.ptr, self._arr.ctypes.data, self._arr.nbytes, 1), "hipMemcpy")

    @staticmethod
    def _check(rc, what):
        if rc != 0:
            raise EncodingError(N.JTK_ERR_HIP, "%s failed (%d)" % (what, rc))

    def fetch(self):
        out = np.empty_like(self._arr)
        if out.nbytes:
            self._check(N.lib().hipMemcpy(out.ctypes.data, self.ptr, out.nbytes, 2), "hipMemcpy")
        return out

    def free(self):
        if self.ptr:
            N.lib().hipFree(self.ptr)
            self.ptr = C.c_void_p()


@contextlib.contextmanager
def _device_arrays():
    """Scratch of a host-input method: yields put(arr) -> _DeviceArray; every array put is freed on exit."""
    held = []

    def put(arr):
        held.append(_DeviceArray(arr))
        return held[-1]
    try:
        yield put
    finally:
        for x in held:
            x.free()


class EncodingResult:
    """api/EncodingResult.java"""

    def __init__(self, tokens, truncated):
        self.tokens = tokens
        self.truncated = truncated

    def get_tokens(self):
        return self.tokens

    def is_truncated(self):
        return self.truncated

    getTokens = get_tokens
    isTruncated = is_truncated

    def __repr__(self):
        return "EncodingResult{tokens=%r, truncated=%s}" % (self.tokens, str(self.truncated).lower())


class BatchResult:
    """Packed result of a batch encode: tokens[int32], tok_off[int64, n_docs+1], status[int32, n_docs]."""

    def __init__(self, tokens, tok_off, status):
        self.tokens = tokens
        self.tok_off = tok_off
        self.status = status

    def doc(self, d):
        return self.tokens[self.tok_off[d]:self.tok_off[d + 1]]

    def __len__(self):
        return len(self.tok_off) - 1


def widen_ids(lo, hi, id_bits, first=0, n=None):
    """jtk_widen_ids: int32 ids of tokens [first, first + n) from the planes of a compact result (jtk_compact_rules.h)."""
    if n is None:
        n = len(lo) - first
    out = np.empty(max(n, 1), dtype=np.int32)
    _check(N.lib().jtk_widen_ids(lo.ctypes.data if len(lo) else None, hi.ctypes.data if hi is not None and len(hi) else None,
                                 int(id_bits), int(first), int(n), out.ctypes.data))
    return out[:n]


class CompactBatchResult:
    """Packed result of a batch encode with compact ids: lo[uint16, n_tokens] holds id & 0xFFFF, hi[uint32] the id_bits - 16
    bits above of every token back to back (None when id_bits == 16); tok_off and status as in BatchResult.  doc(d) widens
    that document to int32, widen() the whole batch."""

    def __init__(self, lo, hi, id_bits, tok_off, status):
        self.lo = lo
        self.hi = hi
        self.id_bits = id_bits
        self.tok_off = tok_off
        self.status = status

    def doc(self, d):
        first = int(self.tok_off[d])
        return widen_ids(self.lo, self.hi, self.id_bits, first, int(self.tok_off[d + 1]) - first)

    def widen(self):
        return widen_ids(self.lo, self.hi, self.id_bits, 0, len(self.lo))

    @property
    def tokens(self):
        return self.widen()

    def __len__(self):
        return len(self.tok_off) - 1


class HostBuffer:
    """Page-locked host memory (jtk_host_alloc) as a numpy array: input buffers the device reads by DMA."""

    def __init__(self, n_bytes):
        p = C.c_void_p()
        _check(N.lib().jtk_host_alloc(int(n_bytes), C.byref(p)))
        self._p = p
        self.array = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(max(int(n_bytes), 1),))[:int(n_bytes)]

    def close(self):
        if getattr(self, "_p", None):
            self.array = None
            N.lib().jtk_host_free(self._p)
            self._p = None

    def __del__(self):
        try:
            self.close()
        except Exception:          # (interpreter shutdown: the module's globals may be gone)
            pass


class Batch:
    """One caller thread's stream + device scratch (jtk_batch)."""

    def __init__(self, encoding):
        self.encoding = encoding
        h = C.c_void_p()
        _check(N.lib().jtk_batch_create(encoding._h, C.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            N.lib().jtk_batch_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:          # (interpreter shutdown: the module's globals may be gone)
            pass

    def set_option(self, option, value):
        """jtk_batch_set_option: N.JTK_OPT_CHUNK_BYTES, N.JTK_OPT_CHUNKS_IN_FLIGHT, ..., N.JTK_OPT_REPEAT_TABLE_BYTES."""
        _check(N.lib().jtk_batch_set_option(self._h, int(option), int(value)))

    def set_allowed_special(self, ids):
        """jtk_batch_set_allowed_special: the special ids that encodes with allow_special=True take as ids.  None or "all":
        every special of the encoding; an iterable of ids (empty: none)."""
        if ids is None or (isinstance(ids, str) and ids == "all"):
            _check(N.lib().jtk_batch_set_allowed_special(self._h, None, -1))
            return
        arr = np.ascontiguousarray(list(ids), dtype=np.int32)
        _check(N.lib().jtk_batch_set_allowed_special(self._h, arr.ctypes.data if len(arr) else None, len(arr)))

    def set_fim(self, fim, prefix_id=None, middle_id=None, suffix_id=None):
        """jtk_batch_set_fim: the parameters of later encodes with fim=True.  fim: a FimParams (None clears them); the ids default
        to fim's own, then to the encoding's <|fim_prefix|>, <|fim_middle|>, <|fim_suffix|>."""
        if fim is None:
            _check(N.lib().jtk_batch_set_fim(self._h, None))
            return
        ids = self.encoding.fim_ids(fim, prefix_id, middle_id, suffix_id)
        p = N.FimParamsStruct(int(fim.seed) & (2 ** 64 - 1), int(fim.doc_index_base), fim_rate_u32(fim.rate), fim_rate_u32(fim.spm_rate), *ids)
        _check(N.lib().jtk_batch_set_fim(self._h, C.byref(p)))

    def fim_result(self):
        """After an encode with fim=True: (kind uint8 [n_docs] -- 0 untouched, 1 PSM, 2 SPM --, cut int64 [n_docs, 2] -- byte
        positions relative to the document --, part_tok int64 [n_docs, 3] -- tokens of prefix, middle, suffix)."""
        _, nd, _ = self.result()
        kind, cut = np.zeros(max(nd, 1), dtype=np.uint8), np.zeros((max(nd, 1), 2), dtype=np.int64)
        part = np.zeros((max(nd, 1), 3), dtype=np.int64)
        _check(N.lib().jtk_batch_fim_result_fetch(self._h, kind.ctypes.data, cut.ctypes.data, part.ctypes.data))
        return kind[:nd], cut[:nd], part[:nd]

    def fim_device_result(self):
        """Device pointers (kind, cut, part_tok) of the last fim=True encode, valid until the next encode."""
        a, b, c = C.c_void_p(), C.c_void_p(), C.c_void_p()
        _check(N.lib().jtk_batch_fim_result(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def encode_host(self, text_u8, doc_off, ordinary=False, validate=False, count_only=False, to_host=False, allow_special=False,
                    compact=False, fim=False):
        """Host buffers in (numpy arrays, or anything with .ctypes.data such as a pinned HostBuffer view).  to_host: the result
        is streamed to the batch's pinned host memory while later chunks are encoded (read it with host_result()).
        allow_special: the batch's allowed special-token literals become their ids (JTK_ENCODE_ALLOW_SPECIAL).
        compact (with to_host): the ids go up as a 16-bit plane and a plane of the bits above (JTK_ENCODE_COMPACT_IDS; read
        them with host_result_compact()).  fim: the fill-in-the-middle transformation by the parameters of set_fim()
        (JTK_ENCODE_FIM; needs ordinary)."""
        text_u8 = np.ascontiguousarray(text_u8, dtype=np.uint8)
        doc_off = np.ascontiguousarray(doc_off, dtype=np.int64)
        nt = C.c_int64(0)
        flags = _encode_flags(ordinary, validate, count_only, to_host, allow_special, compact, fim)
        self._count_only = count_only
        _check(N.lib().jtk_batch_encode(self._h, text_u8.ctypes.data, doc_off.ctypes.data, len(doc_off) - 1,
                                        flags, C.byref(nt)))
        return nt.value

    def encode_pieces(self, text_u8, doc_off, piece_begin, piece_end, ordinary=True, to_host=False, compact=False):
        """jtk_batch_encode_pieces: the caller's own pattern has been matched on the host; piece i is
        text[piece_begin[i]:piece_end[i]] (positions in the whole batch).  Returns the token total."""
        text_u8 = np.ascontiguousarray(text_u8, dtype=np.uint8)
        doc_off = np.ascontiguousarray(doc_off, dtype=np.int64)
        pb = np.ascontiguousarray(piece_begin, dtype=np.int64)
        pe = np.ascontiguousarray(piece_end, dtype=np.int64)
        nt = C.c_int64(0)
        flags = _encode_flags(ordinary, to_host=to_host, compact=compact)
        self._count_only = False
        _check(N.lib().jtk_batch_encode_pieces(self._h, text_u8.ctypes.data, doc_off.ctypes.data, len(doc_off) - 1,
                                               pb.ctypes.data, pe.ctypes.data, len(pb), flags, C.byref(nt)))
        return nt.value

    def host_result(self):
        """After encode_host(to_host=True): zero-copy numpy views of the batch's pinned result buffers (valid until the
        next encode on this batch)."""
        nt, nd, _ = self.result()
        a, b, c = C.c_void_p(), C.c_void_p(), C.c_void_p()
        _check(N.lib().jtk_batch_host_result(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return BatchResult(_view(a.value, nt, C.c_int32, np.int32), _view(b.value, nd + 1, C.c_int64, np.int64),
                           _view(c.value, nd, C.c_int32, np.int32))

    def host_result_compact(self):
        """After encode_host(to_host=True, compact=True): zero-copy numpy views of the pinned planes as a CompactBatchResult
        (valid until the next encode on this batch)."""
        nt, nd, _ = self.result()
        lo, hi, t, s = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        bits = C.c_int(0)
        _check(N.lib().jtk_batch_host_result_compact(self._h, C.byref(lo), C.byref(hi), C.byref(bits), C.byref(t), C.byref(s)))
        hb = bits.value - 16
        n_lo = nt if lo.value else 0
        return CompactBatchResult(_view(lo.value, n_lo, C.c_uint16, np.uint16),
                                  _view(hi.value, (n_lo * hb + 31) // 32, C.c_uint32, np.uint32) if hb else None, bits.value,
                                  _view(t.value, nd + 1, C.c_int64, np.int64), _view(s.value, nd, C.c_int32, np.int32))

    def compact(self, d_lo_ptr, d_hi_ptr, stream=None):
        """jtk_batch_compact on the last encode: uint16 [n_tokens] at d_lo_ptr and uint32 [ceil(n_tokens * (id_bits - 16) / 32)]
        at d_hi_ptr (None when id_bits == 16), device pointers; waits for the token count, not for the pass."""
        _check(N.lib().jtk_batch_compact(self._h, d_lo_ptr, d_hi_ptr, stream))

    def minhash(self, d_sig_ptr, ngram=5, num_hashes=128, bands=0, seed=0, d_n_shingles_ptr=None, d_band_keys_ptr=None, stream=None):
        """jtk_batch_minhash on the last encode: uint32 [n_docs * num_hashes] at d_sig_ptr, int32 [n_docs] at d_n_shingles_ptr
        (or None), uint64 [n_docs * bands] at d_band_keys_ptr (or None: no keys), device pointers; waits for the token count, not
        for the pass."""
        p = N.MinhashParamsStruct(seed & 0xFFFFFFFFFFFFFFFF, ngram, num_hashes, bands, 0)
        _check(N.lib().jtk_batch_minhash(self._h, C.byref(p), d_sig_ptr, d_n_shingles_ptr, d_band_keys_ptr, stream))

    def minhash_agree(self, d_sig_ptr, n_sig, num_hashes, d_pair_a_ptr, d_pair_b_ptr, n_pairs, d_agree_ptr, stream=None):
        """jtk_batch_minhash_agree: int32 [n_pairs] at d_agree_ptr, per pair (int64 indices at d_pair_a_ptr, d_pair_b_ptr) the
        words on which the two rows of uint32 [n_sig * num_hashes] at d_sig_ptr agree, -1 for an index outside [0, n_sig).
        Needs no encode on the batch; does not wait."""
        _check(N.lib().jtk_batch_minhash_agree(self._h, d_sig_ptr, n_sig, num_hashes, d_pair_a_ptr, d_pair_b_ptr, n_pairs,
                                               d_agree_ptr, stream))

    def ngram_overlap(self, ngram_set, d_tok_flags_ptr=None, d_n_hit_ptr=None, d_n_covered_ptr=None, d_first_hit_ptr=None, stream=None):
        """jtk_batch_ngram_overlap of the last encode against an NgramSet: uint8 [n_tokens] at d_tok_flags_ptr, int32 [n_docs] at
        d_n_hit_ptr and d_n_covered_ptr, int64 [n_docs] at d_first_hit_ptr, device pointers, each may be None and is then not
        written; waits for the token count, not for the pass."""
        _check(N.lib().jtk_batch_ngram_overlap(self._h, ngram_set._h, d_tok_flags_ptr, d_n_hit_ptr, d_n_covered_ptr, d_first_hit_ptr, stream))

    def ngram_repeats(self, ngram, d_tok_flags_ptr=None, d_n_repeat_ptr=None, d_n_covered_ptr=None, d_top_count_ptr=None,
                      d_top_first_ptr=None, seed=0, mark_first=False, doc_index_base=0, stream=None):
        """jtk_batch_ngram_repeats of the last encode: uint8 [n_tokens] at d_tok_flags_ptr (JTK_RP_START | JTK_RP_COVERED per
        token), int32 [n_docs] at d_n_repeat_ptr, d_n_covered_ptr and d_top_count_ptr, int64 [n_docs] at d_top_first_ptr, device
        pointers, each may be None and is then not written; waits for the token count and for the documents' token counts (the
        groups that share a table are planned from them), not for the pass."""
        p = N.RepeatParamsStruct(seed & 0xFFFFFFFFFFFFFFFF, doc_index_base & 0xFFFFFFFFFFFFFFFF, ngram,
                                 N.JTK_REPEAT_MARK_FIRST if mark_first else 0)
        _check(N.lib().jtk_batch_ngram_repeats(self._h, C.byref(p), d_tok_flags_ptr, d_n_repeat_ptr, d_n_covered_ptr, d_top_count_ptr,
                                               d_top_first_ptr, stream))

    def line_units(self, unit="line", trim=False, seed=0, doc_index_base=0, stream=None):
        """jtk_batch_line_units of the last encode's text: finds and hashes the lines (unit="line") or paragraphs ("paragraph"),
        keeps the list in the batch and returns the number of units; waits once, for that number."""
        n = C.c_int64(0)
        _check(N.lib().jtk_batch_line_units(self._h, C.byref(_lines_params(unit, trim, False, seed, doc_index_base)), stream, C.byref(n)))
        return n.value

    def line_repeats(self, unit="line", trim=False, mark_first=False, seed=0, doc_index_base=0, stream=None, **ptrs):
        """jtk_batch_line_repeats over the list of a line_units call with the same unit, trim, seed and doc_index_base: device
        pointers by the field names of jtk_lines_out (unit_begin=, unit_end=, unit_flags=, unit_off=, n_dup=, dup_bytes=,
        dup_chars=, unit_bytes=, unit_chars=, doc_chars=, top_count=, top_first=), each may be left out or None and is then not
        written; waits for the documents' unit counts, not for the pass."""
        unknown = set(ptrs) - set(N.LINES_OUT_FIELDS)
        if unknown:
            raise TypeError("line_repeats: no output named %s" % ", ".join(sorted(unknown)))
        out = N.LinesOutStruct(**{k: v for k, v in ptrs.items() if v})
        _check(N.lib().jtk_batch_line_repeats(self._h, C.byref(_lines_params(unit, trim, mark_first, seed, doc_index_base)), C.byref(out), stream))

    def encode_device(self, d_text_ptr, d_doc_off_ptr, n_docs, n_bytes, ordinary=False, stream=None, sync=True,
                      allow_special=False, validate=False, count_only=False, fim=False):
        nt = C.c_int64(0)
        flags = _encode_flags(ordinary, validate, count_only, allow_special=allow_special, fim=fim)
        _check(N.lib().jtk_batch_encode_device(self._h, d_text_ptr, d_doc_off_ptr, n_docs, n_bytes, flags, stream,
                                               C.byref(nt) if sync else None))
        return nt.value if sync else None

    def stream(self):
        """The batch's own HIP stream handle (int)."""
        return N.lib().jtk_batch_stream(self._h)

    def result(self):
        nt, nd, ws = C.c_int64(0), C.c_int64(0), C.c_int32(0)
        _check(N.lib().jtk_batch_result(self._h, C.byref(nt), C.byref(nd), C.byref(ws)))
        return nt.value, nd.value, ws.value

    def fetch_counts(self):
        """Token count per document and status (works after any encode; the only fetch after a count-only one)."""
        _, nd, _ = self.result()
        tok_off = np.empty(nd + 1, dtype=np.int64)
        status = np.zeros(max(nd, 1), dtype=np.int32)
        _check(N.lib().jtk_batch_fetch(self._h, None, 0, tok_off.ctypes.data, status.ctypes.data))
        return np.diff(tok_off), status[:nd]

    def fetch(self):
        nt, nd, _ = self.result()
        tokens = np.empty(max(nt, 1), dtype=np.int32)
        tok_off = np.empty(nd + 1, dtype=np.int64)
        status = np.zeros(max(nd, 1), dtype=np.int32)
        _check(N.lib().jtk_batch_fetch(self._h, tokens.ctypes.data, nt, tok_off.ctypes.data, status.ctypes.data))
        return BatchResult(tokens[:nt], tok_off, status[:nd])

    def device_result(self):
        a, b, c = C.c_void_p(), C.c_void_p(), C.c_void_p()
        _check(N.lib().jtk_batch_device_result(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    # ---- maxTokens for the whole batch (device) ---------------------------------------------------------
    def encode_max_tokens(self, text_u8, doc_off, max_tokens, ordinary=False):
        """jtk_batch_encode_max_tokens: (tokens [n_docs, max_tokens], kept [n_docs], truncated [n_docs], status [n_docs])."""
        text_u8 = np.ascontiguousarray(text_u8, dtype=np.uint8)
        doc_off = np.ascontiguousarray(doc_off, dtype=np.int64)
        nd, mt = len(doc_off) - 1, max(0, int(max_tokens))
        toks = np.zeros((nd, mt), dtype=np.int32)
        kept = np.zeros(nd, dtype=np.int64)
        flag = np.zeros(nd, dtype=np.uint8)
        status = np.zeros(nd, dtype=np.int32)
        _check(N.lib().jtk_batch_encode_max_tokens(self._h, text_u8.ctypes.data, doc_off.ctypes.data, nd,
                                                   N.JTK_ENCODE_ORDINARY if ordinary else 0, mt, toks.ctypes.data,
                                                   kept.ctypes.data, flag.ctypes.data, status.ctypes.data))
        return toks, kept, flag, status

    def encode_device_max_tokens(self, d_text_ptr, d_doc_off_ptr, n_docs, n_bytes, max_tokens, d_tokens_ptr, d_kept_ptr,
                                 d_trunc_ptr, d_status_ptr, ordinary=False, pad_id=-1, stream=None):
        """jtk_batch_encode_device_max_tokens: device text and offsets in, rows [n_docs, max_tokens] (int32, pad_id after the
        kept ids), kept (int64), truncated (uint8) and status (int32) out, all device pointers; ordered on `stream`."""
        _check(N.lib().jtk_batch_encode_device_max_tokens(self._h, d_text_ptr, d_doc_off_ptr, int(n_docs), int(n_bytes),
                                                          N.JTK_ENCODE_ORDINARY if ordinary else 0, int(max_tokens), int(pad_id),
                                                          d_tokens_ptr, d_kept_ptr, d_trunc_ptr, d_status_ptr, stream))

    def truncate(self, max_tokens):
        """Encoding.encode(text, maxTokens) for every document of the last encode -> (kept int64[n], truncated bool[n])."""
        _check(N.lib().jtk_batch_truncate(self._h, int(max_tokens)))
        _, nd, _ = self.result()
        kept = np.zeros(max(nd, 1), dtype=np.int64)
        flag = np.zeros(max(nd, 1), dtype=np.uint8)
        _check(N.lib().jtk_batch_fetch_truncated(self._h, kept.ctypes.data, flag.ctypes.data))
        return kept[:nd], flag[:nd].astype(bool)

    # ---- chunks of a token budget (device) ---------------------------------------------------------------
    def chunk(self, chunk_tokens, overlap=0, stream=None):
        """jtk_batch_chunk on the last encode: chunks of at most chunk_tokens tokens (jtk_chunk_rules.h).  Returns n_chunks."""
        n = C.c_int64(0)
        _check(N.lib().jtk_batch_chunk(self._h, int(chunk_tokens), int(overlap), stream, C.byref(n)))
        self._n_chunks = n.value
        return n.value

    def chunk_fetch(self):
        """The last chunk call's arrays on the host: dict of chunk_off [n_docs + 1], doc, tok_begin, n_tok, byte_begin,
        byte_end, split [n_chunks]."""
        _, nd, _ = self.result()
        nc = self._n_chunks
        f = dict(chunk_off=np.zeros(nd + 1, dtype=np.int64), doc=np.zeros(max(nc, 1), dtype=np.int64),
                 tok_begin=np.zeros(max(nc, 1), dtype=np.int64), n_tok=np.zeros(max(nc, 1), dtype=np.int32),
                 byte_begin=np.zeros(max(nc, 1), dtype=np.int64), byte_end=np.zeros(max(nc, 1), dtype=np.int64),
                 split=np.zeros(max(nc, 1), dtype=np.uint8))
        _check(N.lib().jtk_batch_chunk_fetch(self._h, *(f[k].ctypes.data for k in ("chunk_off", "doc", "tok_begin", "n_tok",
                                                                                   "byte_begin", "byte_end", "split"))))
        return {k: (v if k == "chunk_off" else v[:nc]) for k, v in f.items()}

    def chunk_device_result(self):
        """Device pointers (chunk_off, doc, tok_begin, n_tok, byte_begin, byte_end, split) of the last chunk call."""
        ps = [C.c_void_p() for _ in range(7)]
        _check(N.lib().jtk_batch_chunk_device_result(self._h, *(C.byref(p) for p in ps)))
        return tuple(p.value for p in ps)

    def chunk_rows(self, pad_id, d_rows_ptr, stream=None):
        """jtk_batch_chunk_rows: [n_chunks, chunk_tokens] int32 at d_rows_ptr, the chunk's ids then pad_id."""
        _check(N.lib().jtk_batch_chunk_rows(self._h, int(pad_id), d_rows_ptr, stream))

    def token_offsets(self, d_byte_pos_ptr, stream=None):
        """jtk_batch_token_offsets: int64 [n_tokens] at d_byte_pos_ptr, each token's byte position in the batch text."""
        _check(N.lib().jtk_batch_token_offsets(self._h, d_byte_pos_ptr, stream))

    def chunk_prefer(self, chunk_tokens, overlap=0, min_tokens=None, prefer="all", stream=None):
        """jtk_batch_chunk_prefer on the last encode: chunks of at most chunk_tokens tokens that end at the best paragraph, line,
        sentence or word boundary in [min_tokens, chunk_tokens] (jtk_chunk_prefer_rules.h).  min_tokens defaults to
        (chunk_tokens + 1) // 2.  The result replaces chunk()'s: chunk_fetch, chunk_device_result and chunk_rows read it.
        Returns n_chunks."""
        n = C.c_int64(0)
        mt = (int(chunk_tokens) + 1) // 2 if min_tokens is None else int(min_tokens)
        _check(N.lib().jtk_batch_chunk_prefer(self._h, int(chunk_tokens), int(overlap), mt, prefer_mask(prefer), stream, C.byref(n)))
        self._n_chunks = n.value
        return n.value

    def chunk_levels(self):
        """(end_level uint8 [n_chunks] on the host, its device pointer) of the last chunk_prefer call (JTK_LEVEL_*)."""
        nc = self._n_chunks
        lv = np.zeros(max(nc, 1), dtype=np.uint8)
        p = C.c_void_p()
        _check(N.lib().jtk_batch_chunk_levels(self._h, lv.ctypes.data, C.byref(p)))
        return lv[:nc], p.value

    def chunk_levels_device(self):
        """Device pointer of end_level uint8 [n_chunks] of the last chunk_prefer call (does not wait)."""
        p = C.c_void_p()
        _check(N.lib().jtk_batch_chunk_levels(self._h, None, C.byref(p)))
        return p.value

    def token_cut_levels(self, prefer, d_level_ptr, stream=None):
        """jtk_batch_token_cut_levels: uint8 [n_tokens] at d_level_ptr, the level of the cut before every token under `prefer`
        (6 for the first token of a document)."""
        _check(N.lib().jtk_batch_token_cut_levels(self._h, prefer_mask(prefer), d_level_ptr, stream))

    # ---- packed training rows (device) -------------------------------------------------------------------
    def pack(self, seq_len, sep_id=-1, whole_docs=False, sep_first=False, drop_last=False, stream=None):
        """jtk_batch_pack on the last encode (the rule is in jtk_pack_rules.h).  Returns (n_rows, n_segments, max_seqlen)."""
        flags = ((N.JTK_PACK_WHOLE_DOCS if whole_docs else 0) | (N.JTK_PACK_SEP_FIRST if sep_first else 0)
                 | (N.JTK_PACK_DROP_LAST if drop_last else 0))
        nr, ns, mx = C.c_int64(0), C.c_int64(0), C.c_int32(0)
        _check(N.lib().jtk_batch_pack(self._h, int(seq_len), int(sep_id), flags, stream, C.byref(nr), C.byref(ns), C.byref(mx)))
        self._pack = (nr.value, int(seq_len), ns.value)
        return nr.value, ns.value, mx.value

    def pack_write(self, pad_id, d_rows_ptr, d_positions_ptr=None, d_cu_seqlens_ptr=None, d_seg_doc_ptr=None, stream=None):
        """jtk_batch_pack_write: rows / positions int32 [n_rows, seq_len], cu_seqlens int32 [n_segments + 1], seg_doc int64
        [n_segments] at the given device pointers (all but the rows may be None); does not wait."""
        _check(N.lib().jtk_batch_pack_write(self._h, int(pad_id), d_rows_ptr, d_positions_ptr, d_cu_seqlens_ptr, d_seg_doc_ptr,
                                            stream))

    def pack_fetch(self, pad_id=-1):
        """The last pack call's result on the host: dict of rows, positions [n_rows, seq_len] int32, cu_seqlens int32,
        seg_doc int64."""
        nr, L, ns = self._pack
        f = dict(rows=np.zeros((nr, L), dtype=np.int32), positions=np.zeros((nr, L), dtype=np.int32),
                 cu_seqlens=np.zeros(ns + 1, dtype=np.int32), seg_doc=np.zeros(max(ns, 1), dtype=np.int64))
        _check(N.lib().jtk_batch_pack_fetch(self._h, int(pad_id), *(f[k].ctypes.data for k in ("rows", "positions", "cu_seqlens",
                                                                                               "seg_doc"))))
        f["seg_doc"] = f["seg_doc"][:ns]
        return f

    # ---- labels of the packed rows from byte spans (device) ----------------------------------------------
    def token_spans(self, d_begin, d_end, n_spans, rule, d_tok_span, stream=None):
        """jtk_batch_token_spans on the last encode: int32 [n_tokens] at d_tok_span, per token the lowest of the n_spans spans
        [begin[i], end[i]) (int64 device arrays, batch positions, sorted and disjoint) that holds it by `rule` ("whole",
        "start", "any" or a JTK_SPAN_* value), or -1 (the rule is in jtk_label_rules.h)."""
        _check(N.lib().jtk_batch_token_spans(self._h, d_begin, d_end, int(n_spans), _span_rule(rule), d_tok_span, stream))

    def pack_labels(self, d_tok_span, ignore_index, d_labels, shift=False, label_sep=False, stream=None):
        """jtk_batch_pack_labels on the last pack: int32 [n_rows, seq_len] at d_labels from d_tok_span (None: every token is
        trainable); does not wait."""
        flags = (N.JTK_LABEL_SHIFT if shift else 0) | (N.JTK_LABEL_SEP if label_sep else 0)
        _check(N.lib().jtk_batch_pack_labels(self._h, d_tok_span, int(ignore_index), flags, d_labels, stream))

    def pack_labels_fetch(self, d_tok_span, ignore_index=-100, shift=False, label_sep=False):
        """The same on the host: labels int32 [n_rows, seq_len] (d_tok_span stays a device pointer, or None)."""
        nr, L, _ = self._pack
        out = np.zeros((nr, L), dtype=np.int32)
        flags = (N.JTK_LABEL_SHIFT if shift else 0) | (N.JTK_LABEL_SEP if label_sep else 0)
        _check(N.lib().jtk_batch_pack_labels_fetch(self._h, d_tok_span, int(ignore_index), flags, out.ctypes.data))
        return out

    # ---- character positions of the last encode's text (device) ------------------------------------------
    def char_index(self, unit, d_doc_units_ptr=None, stream=None):
        """jtk_batch_char_index: builds the index of the last encode's text for `unit` ("utf16", "char", "byte" or a
        JTK_UNIT_* value); int64 [n_docs] at d_doc_units_ptr (may be None): every document's length in that unit."""
        _check(N.lib().jtk_batch_char_index(self._h, _unit(unit), d_doc_units_ptr, stream))

    def char_positions(self, unit, d_byte_pos_ptr, n, d_char_pos_ptr, round="floor", d_doc_ptr=None, stream=None):
        """jtk_batch_char_positions: int64 [n] at d_char_pos_ptr, the index in its document of each of the n batch byte
        positions at d_byte_pos_ptr, rounded down ("floor") or up ("ceil") to a character; d_doc_ptr (int64 [n], or None: the
        document that holds the position) names the documents.  -1 outside the document."""
        _check(N.lib().jtk_batch_char_positions(self._h, _unit(unit), _round(round), d_doc_ptr, d_byte_pos_ptr, int(n), d_char_pos_ptr,
                                                stream))

    def byte_positions(self, unit, d_doc_ptr, d_char_pos_ptr, n, d_byte_pos_ptr, stream=None):
        """jtk_batch_byte_positions: int64 [n] at d_byte_pos_ptr, the batch byte position of index d_char_pos[i] of document
        d_doc[i] (an index past the document: its end; a negative one: -1)."""
        _check(N.lib().jtk_batch_byte_positions(self._h, _unit(unit), d_doc_ptr, d_char_pos_ptr, int(n), d_byte_pos_ptr, stream))

    def token_char_offsets(self, unit, d_begin_ptr, d_end_ptr=None, stream=None):
        """jtk_batch_token_char_offsets: int64 [n_tokens] at d_begin_ptr and d_end_ptr (may be None): every token's range
        [begin, end) in its document, in `unit`."""
        _check(N.lib().jtk_batch_token_char_offsets(self._h, _unit(unit), d_begin_ptr, d_end_ptr, stream))

    # ---- batch decode (device) -------------------------------------------------------------------------
    def decode_host(self, ids, seq_off):
        """ids int32[n], seq_off int64[n_seqs+1] -> total byte count (result stays on the device)."""
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        seq_off = np.ascontiguousarray(seq_off, dtype=np.int64)
        nb = C.c_int64(0)
        _check(N.lib().jtk_batch_decode(self._h, ids.ctypes.data, seq_off.ctypes.data, len(seq_off) - 1, C.byref(nb)))
        self._dec_shape = (nb.value, len(seq_off) - 1)
        return nb.value

    def decode_device(self, d_ids_ptr, d_seq_off_ptr, n_seqs, n_ids, stream=None):
        nb = C.c_int64(0)
        _check(N.lib().jtk_batch_decode_device(self._h, d_ids_ptr, d_seq_off_ptr, n_seqs, n_ids, stream, C.byref(nb)))
        self._dec_shape = (nb.value, n_seqs)
        return nb.value

    def decode_fetch(self):
        nb, ns = self._dec_shape
        out = np.empty(max(nb, 1), dtype=np.uint8)
        byte_off = np.empty(ns + 1, dtype=np.int64)
        status = np.zeros(max(ns, 1), dtype=np.int32)
        _check(N.lib().jtk_batch_decode_fetch(self._h, out.ctypes.data, nb, byte_off.ctypes.data, status.ctypes.data))
        return out[:nb], byte_off, status[:ns]

    # ---- decode of an id matrix (device); the result is read with decode_fetch ----------------------------
    @staticmethod
    def _rows_options(stop_ids, skip_pad, keep_stop):
        stop = np.ascontiguousarray(list(stop_ids), dtype=np.int64)
        flags = (N.JTK_DECODE_SKIP_PAD if skip_pad else 0) | (N.JTK_DECODE_KEEP_STOP if keep_stop else 0)
        return stop, flags

    def decode_rows_device(self, d_rows_ptr, id_bytes, n_rows, width, row_stride=None, d_begin_ptr=None, d_end_ptr=None, pad_id=-1,
                           stop_ids=(), skip_pad=False, keep_stop=False, d_cell_byte_ptr=None, stream=None):
        """jtk_batch_decode_rows_device: n_rows x width ids of id_bytes bytes at d_rows_ptr -> total byte count (result on the
        device)."""
        stop, flags = self._rows_options(stop_ids, skip_pad, keep_stop)
        nb = C.c_int64(0)
        _check(N.lib().jtk_batch_decode_rows_device(self._h, d_rows_ptr, id_bytes, n_rows, width, width if row_stride is None else row_stride,
                                                    d_begin_ptr, d_end_ptr, int(pad_id), stop.ctypes.data if len(stop) else None,
                                                    len(stop), flags, d_cell_byte_ptr, stream, C.byref(nb)))
        self._dec_shape = (nb.value, n_rows)
        return nb.value

    def decode_rows_host(self, rows, begin=None, end=None, pad_id=-1, stop_ids=(), skip_pad=False, keep_stop=False, cell_byte=False):
        """jtk_batch_decode_rows: rows is a 2-d numpy int32 / int64 matrix whose rows are contiguous (a row-strided view is passed
        as it is) -> total byte count, or (total, cell_byte int64 [n_rows, width]) when cell_byte is asked for."""
        rows = np.asarray(rows)
        if rows.ndim != 2 or rows.dtype not in (np.dtype(np.int32), np.dtype(np.int64)):
            raise ValueError("rows must be a 2-d int32 or int64 array")
        nr, width = rows.shape
        isz = rows.itemsize
        if nr > 1 and width > 0 and rows.strides[1] == isz and rows.strides[0] % isz == 0 and rows.strides[0] >= width * isz:
            stride = rows.strides[0] // isz
        else:
            rows, stride = np.ascontiguousarray(rows), width
        win = [None if a is None else np.ascontiguousarray(a, dtype=np.int64) for a in (begin, end)]
        for a in win:
            if a is not None and a.shape != (nr,):
                raise ValueError("begin / end need one entry per row")
        stop, flags = self._rows_options(stop_ids, skip_pad, keep_stop)
        cells = np.zeros((nr, width), dtype=np.int64) if cell_byte else None
        nb = C.c_int64(0)
        _check(N.lib().jtk_batch_decode_rows(self._h, rows.ctypes.data if rows.size else None, isz, nr, width, stride,
                                             None if win[0] is None else win[0].ctypes.data, None if win[1] is None else win[1].ctypes.data,
                                             int(pad_id), stop.ctypes.data if len(stop) else None, len(stop), flags,
                                             cells.ctypes.data if cell_byte else None, C.byref(nb)))
        self._dec_shape = (nb.value, nr)
        return (nb.value, cells) if cell_byte else nb.value

    def decode_device_result(self):
        """jtk_batch_decode_device_result: device pointers (out, byte_off, status) of the last decode."""
        p = [C.c_void_p() for _ in range(3)]
        _check(N.lib().jtk_batch_decode_device_result(self._h, *(C.byref(x) for x in p)))
        return tuple(x.value for x in p)

    # ---- UTF-16 in and out (device; the rules are jtk_utf16_rules.h) --------------------------------------
    def transcode_utf16_device(self, d_units_ptr, d_unit_off_ptr, n_docs, n_units, stream=None):
        """jtk_batch_transcode_utf16_device: uint16 units and int64 offsets on the device -> the byte count of the UTF-8 text the
        batch now owns (utf8_device_result)."""
        nb = C.c_int64(0)
        _check(N.lib().jtk_batch_transcode_utf16_device(self._h, d_units_ptr, d_unit_off_ptr, n_docs, n_units, stream, C.byref(nb)))
        return nb.value

    def utf8_device_result(self):
        """jtk_batch_utf8_device_result: (device pointer of the UTF-8 text, of doc_off int64 [n_docs + 1], n_bytes) of the last
        transcode."""
        a, o, nb = C.c_void_p(), C.c_void_p(), C.c_int64(0)
        _check(N.lib().jtk_batch_utf8_device_result(self._h, C.byref(a), C.byref(o), C.byref(nb)))
        return a.value, o.value, nb.value

    def encode_utf16_device(self, d_units_ptr, d_unit_off_ptr, n_docs, n_units, ordinary=False, stream=None, sync=True,
                            allow_special=False, validate=False, count_only=False, to_host=False):
        """jtk_batch_encode_utf16_device: the transcode, then the encode of the owned text (to_host: the library refuses it)."""
        nt = C.c_int64(0)
        flags = _encode_flags(ordinary, validate, count_only, to_host, allow_special)
        self._count_only = count_only
        _check(N.lib().jtk_batch_encode_utf16_device(self._h, d_units_ptr, d_unit_off_ptr, n_docs, n_units, flags, stream,
                                                     C.byref(nt) if sync else None))
        return nt.value if sync else None

    def encode_utf16_host(self, units, unit_off, ordinary=False, allow_special=False, validate=False, count_only=False, to_host=False):
        """jtk_batch_encode_utf16: numpy uint16 units and int64 offsets in host memory -> the token total."""
        units = np.ascontiguousarray(units, dtype=np.uint16)
        unit_off = np.ascontiguousarray(unit_off, dtype=np.int64)
        if len(unit_off) < 1 or unit_off[-1] > len(units):
            # (the C entry takes n_units = unit_off[n_docs]: only here is the length of the array known)
            raise ValueError("unit_off needs n_docs + 1 entries and must end at or below len(units)")
        nt = C.c_int64(0)
        flags = _encode_flags(ordinary, validate, count_only, to_host, allow_special)
        self._count_only = count_only
        _check(N.lib().jtk_batch_encode_utf16(self._h, units.ctypes.data if len(units) else None, unit_off.ctypes.data, len(unit_off) - 1,
                                              flags, C.byref(nt)))
        return nt.value

    def decode_utf16(self, stream=None):
        """jtk_batch_decode_utf16 over the last decode (flat or rows) -> the unit total (result on the device)."""
        nu = C.c_int64(0)
        _check(N.lib().jtk_batch_decode_utf16(self._h, stream, C.byref(nu)))
        self._dec16_shape = (nu.value, self._dec_shape[1])
        return nu.value

    def decode_utf16_fetch(self):
        nu, ns = self._dec16_shape
        units = np.empty(max(nu, 1), dtype=np.uint16)
        unit_off = np.empty(ns + 1, dtype=np.int64)
        status = np.zeros(max(ns, 1), dtype=np.int32)
        _check(N.lib().jtk_batch_decode_utf16_fetch(self._h, units.ctypes.data, nu, unit_off.ctypes.data, status.ctypes.data))
        return units[:nu], unit_off, status[:ns]

    def decode_utf16_device_result(self):
        """jtk_batch_decode_utf16_device_result: device pointers (units, unit_off, status)."""
        p = [C.c_void_p() for _ in range(3)]
        _check(N.lib().jtk_batch_decode_utf16_device_result(self._h, *(C.byref(x) for x in p)))
        return tuple(x.value for x in p)

    # ---- stop strings over the last decode (device; the rule is jtk_stop_rules.h) --------------------------
    def decode_find_stops(self, stop_strings, d_from_ptr=None, d_cell_byte_ptr=None, width=0, stream=None):
        """jtk_batch_decode_find_stops over the last decode (flat or rows): stop_strings is a sequence of bytes / str (a str
        is its UTF-8 bytes) in order of preference; d_from_ptr int64 [n_seqs] and d_cell_byte_ptr int64 [n_rows, width] are
        device pointers or None.  Queued on stream (None: the batch's); does not wait."""
        blob, str_off = _stop_blob(stop_strings)
        _check(N.lib().jtk_batch_decode_find_stops(self._h, blob.ctypes.data if len(blob) else None, str_off.ctypes.data, len(str_off) - 1,
                                                   d_from_ptr, d_cell_byte_ptr, width, stream))

    def decode_stops_fetch(self):
        """jtk_batch_decode_stops_fetch -> (stop_pos int64, stop_which int32, hold int32, stop_col int64), each [n_seqs]."""
        ns = self._dec_shape[1]
        pos, col = np.zeros(max(ns, 1), dtype=np.int64), np.zeros(max(ns, 1), dtype=np.int64)
        which, hold = np.zeros(max(ns, 1), dtype=np.int32), np.zeros(max(ns, 1), dtype=np.int32)
        _check(N.lib().jtk_batch_decode_stops_fetch(self._h, pos.ctypes.data, which.ctypes.data, hold.ctypes.data, col.ctypes.data))
        return pos[:ns], which[:ns], hold[:ns], col[:ns]

    def decode_stops_device_result(self):
        """jtk_batch_decode_stops_device_result: device pointers (stop_pos, stop_which, hold, stop_col)."""
        p = [C.c_void_p() for _ in range(4)]
        _check(N.lib().jtk_batch_decode_stops_device_result(self._h, *(C.byref(x) for x in p)))
        return tuple(x.value for x in p)

    def set_profiling(self, on=True):
        _check(N.lib().jtk_batch_set_profiling(self._h, 1 if on else 0))

    def kernel_times(self):
        names = (C.c_char_p * 16)()
        ms = (C.c_float * 16)()
        n = C.c_int(0)
        _check(N.lib().jtk_batch_kernel_times(self._h, names, ms, 16, C.byref(n)))
        return {names[i].decode(): float(ms[i]) for i in range(n.value)}

    def encode_one(self, text, ordinary, max_tokens):
        if text is None:
            return [], False
        b = text if isinstance(text, (bytes, bytearray)) else text.encode("utf-8")
        cap = len(b) + 1
        out = np.empty(cap, dtype=np.int32)
        nt = C.c_int64(0)
        tr = C.c_int(0)
        _check(N.lib().jtk_encode(self._h, bytes(b), len(b), N.JTK_ENCODE_ORDINARY if ordinary else 0,
                                  -1 if max_tokens is None else max(0, int(max_tokens)), out.ctypes.data, cap,
                                  C.byref(nt), C.byref(tr)))
        return out[:nt.value].tolist(), bool(tr.value)


class NgramSet:
    """A device-resident set of token n-grams of held-out texts (jtk_ngram_set; the rule is in include/jtokkit_amd.h), for
    decontamination: HipEncoding.ngram_overlap_batch marks where corpus documents share an n-gram with it.  It belongs to its
    encoding, which must stay open while the set is used, and keeps no reference to any batch."""

    def __init__(self, encoding, ngram, seed=0):
        self.encoding = encoding
        self.ngram = int(ngram)
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        p = N.NgramParamsStruct(self.seed, self.ngram, 0)
        h = C.c_void_p()
        _check(N.lib().jtk_ngram_set_create(encoding._h, C.byref(p), C.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            N.lib().jtk_ngram_set_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:          # (interpreter shutdown: the module's globals may be gone)
            pass

    def add_last_encode(self, batch, stream=None):
        """jtk_ngram_set_add_batch: every n-gram of the last encode on `batch` (a Batch of the same encoding)."""
        _check(N.lib().jtk_ngram_set_add_batch(self._h, batch._h, stream))

    def add_texts(self, texts, ordinary=True, **encode_kwargs):
        """Encodes a list of str/bytes (encode_batch's keywords: ordinary, validate, allowed_special, fim) and inserts every
        n-gram of the result; a refused document (status < 0) adds nothing.  Returns the encode's BatchResult."""
        res = self.encoding.encode_batch(texts, ordinary=ordinary, **encode_kwargs)
        self.add_last_encode(self.encoding._b())
        return res

    def add_keys(self, keys):
        """jtk_ngram_set_add_keys: the keys() of a saved set, or of another shard's (uint64; a 0 is refused)."""
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        _check(N.lib().jtk_ngram_set_add_keys(self._h, keys.ctypes.data if keys.size else None, keys.size))

    def _size(self):
        n, cap = C.c_int64(0), C.c_int64(0)
        _check(N.lib().jtk_ngram_set_size(self._h, C.byref(n), C.byref(cap)))
        return n.value, cap.value

    def __len__(self):
        return self._size()[0]

    @property
    def capacity(self):
        """Slots of the device table: the smallest power of two >= max(64, 2 (keys + what the largest insert could add))."""
        return self._size()[1]

    def keys(self):
        """The distinct keys, uint64 [len(self)], in no particular order."""
        out = np.zeros(len(self), dtype=np.uint64)
        _check(N.lib().jtk_ngram_set_keys(self._h, out.ctypes.data if out.size else None, out.size))
        return out


class HipEncoding:
    """GPU-backed `Encoding` (reference GptBytePairEncoding.java:18 is the class this replaces)."""

    def __init__(self, name, pattern_kind, tiktoken_bytes, special_tokens, device=0, host_pattern=None):
        """host_pattern: a compiled pattern object with finditer() over str (e.g. the `regex` module with the Java
        pattern's text) for encodings whose split pattern is neither of the two the device evaluates; the batch methods
        then match on the host and encode the matches through jtk_batch_encode_pieces."""
        self._host_pattern = host_pattern
        self._specials = dict(special_tokens)
        lits = [k.encode("utf-8") for k in special_tokens]
        arr = (C.c_char_p * max(len(lits), 1))(*lits)
        ids = (C.c_int32 * max(len(lits), 1))(*special_tokens.values())
        h = C.c_void_p()
        _check(N.lib().jtk_encoding_create(name.encode("utf-8"), pattern_kind, tiktoken_bytes, len(tiktoken_bytes),
                                           arr, ids, len(lits), device, C.byref(h)))
        self._h = h
        self._name = name
        self._batch = None
        self._svc = None
        self._svc_lock = threading.Lock()
        # close() against per-call methods in progress on other threads: calls are counted, close() waits for them to leave
        # and later ones raise instead of touching freed handles
        self._life = threading.Condition()
        self._calls = 0
        self._closed = False

    def close(self):
        life = getattr(self, "_life", None)
        if life is not None:
            with life:
                self._closed = True
                while self._calls:
                    life.wait()
        if self._batch is not None:
            self._batch.close()
            self._batch = None
        if getattr(self, "_svc", None):
            N.lib().jtk_service_destroy(self._svc)
            self._svc = None
        if getattr(self, "_h", None):
            N.lib().jtk_encoding_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def new_batch(self):
        return Batch(self)

    def _b(self):
        if self._batch is None:
            self._batch = Batch(self)
        return self._batch

    # ---- api/Encoding.java ---------------------------------------------------------------------------
    # "The encoding must be thread-safe" (api/EncodingRegistry.java:51,61): the per-call methods go through the
    # encoding's jtk_service, which coalesces concurrent callers into device batches.
    def _service(self):
        if self._svc is None:
            with self._svc_lock:
                if self._svc is None:
                    h = C.c_void_p()
                    _check(N.lib().jtk_service_create(self._h, 2, C.byref(h)))
                    self._svc = h
        return self._svc

    def _encode_one(self, text, ordinary, max_tokens):
        if text is None:
            return [], False
        b = text if isinstance(text, (bytes, bytearray)) else text.encode("utf-8")
        cap = len(b) + 1
        out = np.empty(cap, dtype=np.int32)
        nt = C.c_int64(0)
        tr = C.c_int(0)
        with self._life:
            if self._closed:
                raise RuntimeError("encoding is closed")
            self._calls += 1
        try:
            _check(N.lib().jtk_service_encode(self._service(), bytes(b), len(b), N.JTK_ENCODE_ORDINARY if ordinary else 0,
                                              -1 if max_tokens is None else max(0, int(max_tokens)), out.ctypes.data, cap,
                                              C.byref(nt), C.byref(tr)))
        finally:
            with self._life:
                self._calls -= 1
                if not self._calls:
                    self._life.notify_all()
        return out[:nt.value].tolist(), bool(tr.value)

    def encode(self, text, max_tokens=None):                       # Encoding.java:29,61
        toks, tr = self._encode_one(text, False, max_tokens)
        return toks if max_tokens is None else EncodingResult(toks, tr)

    def encode_ordinary(self, text, max_tokens=None):              # :80,107
        toks, tr = self._encode_one(text, True, max_tokens)
        return toks if max_tokens is None else EncodingResult(toks, tr)

    def count_tokens(self, text):                                  # :127
        return len(self.encode(text))

    def count_tokens_ordinary(self, text):                         # :147
        return len(self.encode_ordinary(text))

    def decode_bytes(self, tokens):                                # :181
        ids = np.ascontiguousarray(tokens, dtype=np.int32)
        n = C.c_int64(0)
        _check(N.lib().jtk_decode(self._h, ids.ctypes.data, len(ids), None, 0, C.byref(n)))
        out = np.empty(max(n.value, 1), dtype=np.uint8)
        _check(N.lib().jtk_decode(self._h, ids.ctypes.data, len(ids), out.ctypes.data, n.value, C.byref(n)))
        return out[:n.value].tobytes()

    def decode(self, tokens):                                      # :164  new String(bytes, UTF_8)
        return self.decode_bytes(tokens).decode("utf-8", errors="replace")

    def get_name(self):                                            # :189
        return self._name

    encodeOrdinary = encode_ordinary
    countTokens = count_tokens
    countTokensOrdinary = count_tokens_ordinary
    decodeBytes = decode_bytes
    getName = get_name

    # ---- batch -----------------------------------------------------------------------------------------
    def fim_ids(self, fim, prefix_id=None, middle_id=None, suffix_id=None):
        """(prefix_id, middle_id, suffix_id) of a FimParams: the arguments, else its own, else the encoding's <|fim_*|> ids
        (ValueError when the encoding has none and none is given)."""
        out = []
        for given, own, lit in ((prefix_id, fim.prefix_id, "<|fim_prefix|>"), (middle_id, fim.middle_id, "<|fim_middle|>"),
                                (suffix_id, fim.suffix_id, "<|fim_suffix|>")):
            v = given if given is not None else own
            if v is None:
                if lit not in self._specials:
                    raise ValueError("%s has no %s: give FimParams the three sentinel ids" % (self._name, lit))
                v = self._specials[lit]
            out.append(int(v))
        return tuple(out)

    def _fim(self, b, fim, ordinary, allowed_special=None):
        """Sets the batch's FIM parameters for fim (not None); returns whether the encode takes the flag."""
        if fim is None:
            return False
        if not ordinary:
            raise ValueError("fim= needs ordinary=True: encode()'s special-token check would have to look across the cuts")
        if allowed_special is not None:
            raise ValueError("fim= does not combine with allowed_special=")
        if self._host_pattern is not None:
            raise ValueError("fim=: the device cannot run this encoding's custom split pattern")
        b.set_fim(fim)
        return True

    def encode_batch(self, texts, ordinary=False, validate=False, allowed_special=None, fim=None):
        """List of str/bytes -> BatchResult (one jtk_batch_encode call).  allowed_special: None (the literals are refused by
        encode() and ordinary text to encodeOrdinary()), "all", or an iterable of literals that are encoded as their ids
        (JTK_ENCODE_ALLOW_SPECIAL; the rule is in include/jtokkit_amd.h).  fim: a FimParams -- the fill-in-the-middle
        transformation of every document it draws (JTK_ENCODE_FIM; with ordinary=True); the result then also has .fim_kind,
        .fim_cut and .fim_part_tok (Batch.fim_result)."""
        _, text, doc_off = _join_texts(texts)
        return self.encode_batch_packed(text, doc_off, ordinary, validate, allowed_special, fim=fim)

    def encode_batch_packed(self, text_u8, doc_off, ordinary=False, validate=False, allowed_special=None, compact=False, fim=None):
        """compact: the ids cross the link as two planes (JTK_ENCODE_COMPACT_IDS) and come back as a CompactBatchResult that
        owns copies of them."""
        b = self._b()
        if self._fim(b, fim, ordinary, allowed_special):
            b.encode_host(text_u8, doc_off, ordinary, validate, to_host=compact, compact=compact, fim=True)
        elif self._allow(b, allowed_special):
            b.encode_host(text_u8, doc_off, ordinary, validate, allow_special=True, to_host=compact, compact=compact)
        elif self._host_pattern is not None:
            pb, pe = self._match_on_host(text_u8, doc_off)
            b.encode_pieces(text_u8, doc_off, pb, pe, ordinary, to_host=compact, compact=compact)
        else:
            b.encode_host(text_u8, doc_off, ordinary, validate, to_host=compact, compact=compact)
        if compact:
            r = b.host_result_compact()
            res = CompactBatchResult(r.lo.copy(), None if r.hi is None else r.hi.copy(), r.id_bits, r.tok_off.copy(), r.status.copy())
        else:
            res = b.fetch()
        if fim is not None:
            res.fim_kind, res.fim_cut, res.fim_part_tok = b.fim_result()
        return res

    def _char_unit(self, unit, what):
        """JTK_UNIT_* of `unit`; None for bytes.  A custom split pattern has no positions in the text to convert."""
        u = _unit(unit)
        if u == N.JTK_UNIT_BYTE:
            return None
        if self._host_pattern is not None:
            raise ValueError("%s: character positions are not defined for this encoding's custom split pattern" % what)
        return u

    def encode_batch_with_offsets(self, texts, unit="char", ordinary=False, allowed_special=None):
        """encode_batch plus every token's range in its text: (BatchResult, begin int64 [n_tokens], end int64 [n_tokens]).
        unit "char": indices into the Python str (text[begin:end] holds the token's characters; a token that starts inside a
        character begins at that character, one that ends inside a character ends after it -- tiktoken's decode_with_offsets
        convention for begin); "utf16": indices into a Java String; "byte": the token's own bytes, unrounded."""
        bs, text, doc_off = _join_texts(texts)
        u = self._char_unit(unit, "encode_batch_with_offsets")
        res = self.encode_batch_packed(text, doc_off, ordinary, False, allowed_special)
        nt = len(res.tokens)
        b = self._b()
        with _device_arrays() as put:
            d_begin, d_end = put(np.zeros(nt, dtype=np.int64)), put(np.zeros(nt, dtype=np.int64))
            if u is None:
                b.token_offsets(d_begin.ptr)
                _stream_sync(b.stream())
                pos = d_begin.fetch()
                counts = np.diff(res.tok_off)
                doc = np.repeat(np.arange(len(bs)), counts)
                begin = pos - doc_off[doc]
                end = np.empty_like(begin)
                end[:-1] = pos[1:] - doc_off[doc[:-1]]                          # a token ends where the next one begins ...
                last = res.tok_off[1:][counts > 0] - 1
                end[last] = (doc_off[1:] - doc_off[:-1])[doc[last]]             # ... a document's last token at its end
                return res, begin, end
            b.token_char_offsets(u, d_begin.ptr, d_end.ptr)
            _stream_sync(b.stream())
            return res, d_begin.fetch(), d_end.fetch()

    @property
    def id_bits(self):
        """Bits per id of the compact format: 16 + the high bits per token (jtk_encoding_id_bits)."""
        return N.lib().jtk_encoding_id_bits(self._h)

    # ---- what the *_device methods share ---------------------------------------------------------------
    def _check_device_inputs(self, what, *inputs):
        """Every (name, tensor, dtype) of `inputs` is a contiguous 1-d CUDA tensor of that dtype on this encoding's device."""
        import torch
        if self._host_pattern is not None:
            raise ValueError("%s: the device cannot run this encoding's custom split pattern" % what)
        dev = N.lib().jtk_encoding_device(self._h)
        for name, t, dt in inputs:
            if not isinstance(t, torch.Tensor) or t.device.type != "cuda" or t.dtype != dt or t.dim() != 1:
                raise ValueError("%s must be a 1-d CUDA tensor of %s" % (name, dt))
            if t.device.index != dev:
                raise ValueError("%s is on cuda:%s, the encoding on cuda:%d" % (name, t.device.index, dev))
            if not t.is_contiguous():
                raise ValueError("%s must be contiguous" % name)

    @staticmethod
    def _n_docs(doc_off):
        nd = doc_off.numel() - 1
        if nd < 0:
            raise ValueError("doc_off needs n_docs + 1 entries")
        return nd

    @contextlib.contextmanager
    def _on_current_stream(self, b, device):
        """Yields the raw handle of the stream a *_device method queues its work on: torch's current stream.  When that is the
        legacy default stream, whose NULL handle means "the batch's own stream" to the library -- a non-blocking stream that
        does not order against it --, the work goes to the batch's own stream explicitly, forked from the current stream on
        entry and joined into it on exit, also when the body raises: what it has queued by then still orders before the
        caller's next work."""
        import torch
        cur = torch.cuda.current_stream(device)
        if cur.cuda_stream != 0:
            yield cur.cuda_stream
            return
        side = torch.cuda.ExternalStream(b.stream(), device=device)
        side.wait_stream(cur)
        try:
            yield side.cuda_stream
        finally:
            cur.wait_stream(side)

    @contextlib.contextmanager
    def _encode_device_batch(self, text, doc_off, ordinary, allow, fim=False):
        """The encode of a checked device-resident batch, queued without a wait for its token count; yields (batch, n_docs,
        device, stream) with _on_current_stream held for the method's post-passes and copies.  The staged text lives until the
        block is left."""
        import torch
        nd = self._n_docs(doc_off)
        device, n = text.device, text.numel()
        st = text.untyped_storage()
        if text.data_ptr() % 16 or st.data_ptr() + st.nbytes() < text.data_ptr() + (n + 15) // 16 * 16:
            # (the encode reads whole aligned 16-byte blocks; the copy runs on the current stream, so before the fork below)
            buf = torch.zeros((n + 15) // 16 * 16 + 16, dtype=torch.uint8, device=device)
            buf[:n].copy_(text)
            text = buf
        b = self._b()
        with self._on_current_stream(b, device) as stream:
            b.encode_device(text.data_ptr(), doc_off.data_ptr(), nd, n, ordinary, stream=stream, sync=False, allow_special=allow, fim=fim)
            yield b, nd, device, stream

    @staticmethod
    def _tok_off_and_status(b, nd, device, stream):
        """(tok_off int64 [n_docs + 1], status int32 [n_docs]) of the batch's last encode as new CUDA tensors."""
        import torch
        _, p_off, p_status = b.device_result()
        return _device_copy(p_off, nd + 1, torch.int64, device, stream), _device_copy(p_status, nd, torch.int32, device, stream)

    def compact_batch_device(self, text, doc_off, ordinary=False, allowed_special=None):
        """Encodes a device-resident batch and returns its ids compact, as CUDA tensors written on torch.cuda.current_stream():
        (lo uint16 [n_tokens], hi int32 [ceil(n_tokens * (id_bits - 16) / 32)] or None when id_bits == 16 -- the bit pattern of
        the format's uint32 words --, tok_off int64 [n_docs + 1], status int32 [n_docs]).  text: CUDA torch.uint8 tensor, doc_off:
        CUDA torch.int64 tensor [n_docs + 1], on this encoding's device.  Waits once, for the token count (and, with
        allowed_special -- as for encode_batch --, once more for the encode's count of literal candidates)."""
        import torch
        self._check_device_inputs("compact_batch_device", ("text", text, torch.uint8), ("doc_off", doc_off, torch.int64))
        allow = self._allow(self._b(), allowed_special)
        with self._encode_device_batch(text, doc_off, ordinary, allow) as (b, nd, device, stream):
            nt = b.result()[0]
            hb = self.id_bits - 16
            lo = torch.empty(nt, dtype=torch.uint16, device=device)
            hi = torch.empty((nt * hb + 31) // 32, dtype=torch.int32, device=device) if hb else None
            b.compact(lo.data_ptr() if nt else None, hi.data_ptr() if hb and nt else None, stream)
            tok_off, status = self._tok_off_and_status(b, nd, device, stream)
        return lo, hi, tok_off, status

    def minhash_batch(self, texts, ngram=5, num_hashes=128, bands=0, seed=0, ordinary=True, allowed_special=None):
        """MinHash signatures of a list of str/bytes over their token n-grams (jtk_batch_minhash; the rule is in
        include/jtokkit_amd.h): (sig uint32 [n, num_hashes], n_shingles int32 [n], band_keys uint64 [n, bands] or None when
        bands == 0).  The fraction of columns on which two rows agree estimates the Jaccard similarity of the two documents'
        n-gram sets; a refused document (status < 0) has no shingles and a row of 0xFFFFFFFF."""
        bs, text, doc_off = _join_texts(texts)
        self.encode_batch_packed(text, doc_off, ordinary, False, allowed_special)
        n = len(bs)
        b = self._b()
        with _device_arrays() as put:
            sig, n_shingles = put(np.zeros((n, num_hashes), dtype=np.uint32)), put(np.zeros(n, dtype=np.int32))
            keys = put(np.zeros((n, bands), dtype=np.uint64)) if bands else None
            b.minhash(sig.ptr, ngram, num_hashes, bands, seed, n_shingles.ptr, keys.ptr if bands else None)
            _stream_sync(b.stream())
            return sig.fetch(), n_shingles.fetch(), keys.fetch() if bands else None

    def minhash_batch_device(self, text, doc_off, ngram=5, num_hashes=128, bands=0, seed=0, ordinary=True, allowed_special=None):
        """Encodes a device-resident batch (text CUDA torch.uint8, doc_off CUDA torch.int64 [n_docs + 1]) and returns its MinHash
        signatures as CUDA tensors written on torch.cuda.current_stream(): (sig int32 [n_docs, num_hashes] -- the bit patterns of
        the uint32 minima --, n_shingles int32 [n_docs], band_keys int64 [n_docs, bands] -- bit patterns of the uint64 keys -- or
        None when bands == 0, tok_off int64 [n_docs + 1], status int32 [n_docs]).  The ids stay in the batch (device_result).
        Waits once, for the token count (and, with allowed_special, once more for the encode's count of literal candidates)."""
        import torch
        self._check_device_inputs("minhash_batch_device", ("text", text, torch.uint8), ("doc_off", doc_off, torch.int64))
        allow = self._allow(self._b(), allowed_special)
        with self._encode_device_batch(text, doc_off, ordinary, allow) as (b, nd, device, stream):
            sig = torch.empty((nd, num_hashes), dtype=torch.int32, device=device)
            n_shingles = torch.empty(nd, dtype=torch.int32, device=device)
            band_keys = torch.empty((nd, bands), dtype=torch.int64, device=device) if bands else None
            b.minhash(sig.data_ptr() if nd else None, ngram, num_hashes, bands, seed, n_shingles.data_ptr() if nd else None,
                      band_keys.data_ptr() if bands and nd else None, stream)
            tok_off, status = self._tok_off_and_status(b, nd, device, stream)
        return sig, n_shingles, band_keys, tok_off, status

    def ngram_set(self, ngram, seed=0):
        """An empty NgramSet of this encoding: token n-grams of held-out texts, for ngram_overlap_batch (decontamination)."""
        return NgramSet(self, ngram, seed)

    def ngram_overlap_batch(self, texts, ngram_set, ordinary=True, allowed_special=None):
        """Where a list of str/bytes shares a token n-gram with `ngram_set` (jtk_batch_ngram_overlap; the rule is in
        include/jtokkit_amd.h): (flags uint8 [n_tokens] -- JTK_NG_START | JTK_NG_COVERED per token --, n_hit int32 [n],
        n_covered int32 [n], first_hit int64 [n] -- the document-relative index of the first start, or -1 --, tok_off int64
        [n + 1]).  The covered tokens of document d are the set bits of flags[tok_off[d]:tok_off[d + 1]] & JTK_NG_COVERED."""
        bs, text, doc_off = _join_texts(texts)
        res = self.encode_batch_packed(text, doc_off, ordinary, False, allowed_special)
        n = len(bs)
        b = self._b()
        with _device_arrays() as put:
            outs = [put(np.zeros(len(res.tokens), dtype=np.uint8)), put(np.zeros(n, dtype=np.int32)), put(np.zeros(n, dtype=np.int32)),
                    put(np.zeros(n, dtype=np.int64))]
            b.ngram_overlap(ngram_set, *[x.ptr for x in outs])
            _stream_sync(b.stream())
            return tuple(x.fetch() for x in outs) + (res.tok_off.copy(),)

    def ngram_overlap_batch_device(self, text, doc_off, ngram_set, ordinary=True, allowed_special=None):
        """Encodes a device-resident batch (text CUDA torch.uint8, doc_off CUDA torch.int64 [n_docs + 1]) and returns its
        overlap with `ngram_set` as CUDA tensors written on torch.cuda.current_stream(): (flags uint8 [n_tokens], n_hit int32
        [n_docs], n_covered int32 [n_docs], first_hit int64 [n_docs], tok_off int64 [n_docs + 1], status int32 [n_docs]).  The
        ids stay in the batch (device_result).  Waits once, for the token count (and, with allowed_special, once more for the
        encode's count of literal candidates)."""
        import torch
        self._check_device_inputs("ngram_overlap_batch_device", ("text", text, torch.uint8), ("doc_off", doc_off, torch.int64))
        allow = self._allow(self._b(), allowed_special)
        with self._encode_device_batch(text, doc_off, ordinary, allow) as (b, nd, device, stream):
            nt = b.result()[0]
            flags = torch.empty(nt, dtype=torch.uint8, device=device)
            n_hit = torch.empty(nd, dtype=torch.int32, device=device)
            n_covered = torch.empty(nd, dtype=torch.int32, device=device)
            first_hit = torch.empty(nd, dtype=torch.int64, device=device)
            b.ngram_overlap(ngram_set, flags.data_ptr() if nt else None, n_hit.data_ptr() if nd else None,
                            n_covered.data_ptr() if nd else None, first_hit.data_ptr() if nd else None, stream)
            tok_off, status = self._tok_off_and_status(b, nd, device, stream)
        return flags, n_hit, n_covered, first_hit, tok_off, status

    def ngram_repeats_batch(self, texts, ngram, seed=0, mark_first=False, doc_index_base=0, ordinary=True, allowed_special=None):
        """Repeated token n-grams inside each of a list of str/bytes (jtk_batch_ngram_repeats; the rule is in
        include/jtokkit_amd.h): (flags uint8 [n_tokens] -- JTK_RP_START | JTK_RP_COVERED per token --, n_repeat int32 [n],
        n_covered int32 [n], top_count int32 [n], top_first int64 [n] -- the document-relative first position of the most
        frequent n-gram, or -1 --, tok_off int64 [n + 1]).  mark_first: the first occurrence of a repeated n-gram is marked as
        well (RedPajama-v2's count); otherwise only the later ones."""
        bs, text, doc_off = _join_texts(texts)
        res = self.encode_batch_packed(text, doc_off, ordinary, False, allowed_special)
        n = len(bs)
        b = self._b()
        with _device_arrays() as put:
            outs = [put(np.zeros(len(res.tokens), dtype=np.uint8)), put(np.zeros(n, dtype=np.int32)), put(np.zeros(n, dtype=np.int32)),
                    put(np.zeros(n, dtype=np.int32)), put(np.zeros(n, dtype=np.int64))]
            b.ngram_repeats(ngram, *[x.ptr for x in outs], seed=seed, mark_first=mark_first, doc_index_base=doc_index_base)
            _stream_sync(b.stream())
            return tuple(x.fetch() for x in outs) + (res.tok_off.copy(),)

    def ngram_repeats_batch_device(self, text, doc_off, ngram, seed=0, mark_first=False, doc_index_base=0, ordinary=True, allowed_special=None):
        """Encodes a device-resident batch (text CUDA torch.uint8, doc_off CUDA torch.int64 [n_docs + 1]) and returns the repeated
        n-grams inside its documents as CUDA tensors written on torch.cuda.current_stream(): (flags uint8 [n_tokens], n_repeat
        int32 [n_docs], n_covered int32 [n_docs], top_count int32 [n_docs], top_first int64 [n_docs], tok_off int64 [n_docs + 1],
        status int32 [n_docs]).  The ids stay in the batch (device_result).  Waits for the token count and for the documents'
        token counts (and, with allowed_special, once more for the encode's count of literal candidates)."""
        import torch
        self._check_device_inputs("ngram_repeats_batch_device", ("text", text, torch.uint8), ("doc_off", doc_off, torch.int64))
        allow = self._allow(self._b(), allowed_special)
        with self._encode_device_batch(text, doc_off, ordinary, allow) as (b, nd, device, stream):
            nt = b.result()[0]
            flags = torch.empty(nt, dtype=torch.uint8, device=device)
            rows = [torch.empty(nd, dtype=torch.int32, device=device) for _ in range(3)] + [torch.empty(nd, dtype=torch.int64, device=device)]
            b.ngram_repeats(ngram, flags.data_ptr() if nt else None, *[t.data_ptr() if nd else None for t in rows], seed=seed,
                            mark_first=mark_first, doc_index_base=doc_index_base, stream=stream)
            tok_off, status = self._tok_off_and_status(b, nd, device, stream)
        return (flags,) + tuple(rows) + (tok_off, status)

    def line_repeats_batch(self, texts, unit="line", trim=False, mark_first=False, seed=0, doc_index_base=0):
        """Duplicate lines (unit="line") or paragraphs ("paragraph") inside each of a list of str/bytes (jtk_batch_line_units and
        jtk_batch_line_repeats; the rule is in include/jtokkit_amd.h): a dict of numpy arrays by the field names of jtk_lines_out
        -- unit_begin, unit_end int64 [n_units] (byte positions in the documents back to back), unit_flags uint8 [n_units] (1: a
        repeat), unit_off int64 [n + 1], n_dup and top_count int32 [n], dup_bytes, dup_chars, unit_bytes, unit_chars, doc_chars
        and top_first int64 [n].  trim: blanks (space, tab, CR) at a line's ends do not count and a line of blanks is blank;
        mark_first: the first occurrence of a repeated unit is flagged as well."""
        bs, text, doc_off = _join_texts(texts)
        n = len(bs)
        self.encode_batch_packed(text, doc_off, True, False, None)
        b = self._b()
        nu = b.line_units(unit, trim, seed, doc_index_base)
        with _device_arrays() as put:
            outs = {name: put(np.zeros(nu, dtype=dt)) for name, dt in _LINES_PER_UNIT}
            outs["unit_off"] = put(np.zeros(n + 1, dtype=np.int64))
            outs.update({name: put(np.zeros(n, dtype=dt)) for name, dt in _LINES_PER_DOC})
            b.line_repeats(unit, trim, mark_first, seed, doc_index_base, **{name: x.ptr for name, x in outs.items() if x._arr.size})
            _stream_sync(b.stream())
            res = {name: x.fetch() for name, x in outs.items()}
        return res

    def line_repeats_batch_device(self, text, doc_off, unit="line", trim=False, mark_first=False, seed=0, doc_index_base=0, ordinary=True,
                                  allowed_special=None):
        """Encodes a device-resident batch (text CUDA torch.uint8, doc_off CUDA torch.int64 [n_docs + 1]) and returns the duplicate
        lines or paragraphs inside its documents as a dict of CUDA tensors written on torch.cuda.current_stream(), by the field
        names of jtk_lines_out (as line_repeats_batch; unit_flags uint8), plus "status" int32 [n_docs].  Waits once for the number of
        units and once for the documents' unit counts (and, with allowed_special, once more for the encode's count of literal
        candidates), not for the encode's token count."""
        import torch
        self._check_device_inputs("line_repeats_batch_device", ("text", text, torch.uint8), ("doc_off", doc_off, torch.int64))
        allow = self._allow(self._b(), allowed_special)
        with self._encode_device_batch(text, doc_off, ordinary, allow) as (b, nd, device, stream):
            res = self._line_repeats_on(b, nd, device, stream, unit, trim, mark_first, seed, doc_index_base)
            res["status"] = self._tok_off_and_status(b, nd, device, stream)[1]
        return res

    @staticmethod
    def _line_repeats_on(b, nd, device, stream, unit, trim, mark_first, seed, doc_index_base):
        """line_units and line_repeats of the batch's last encode into new CUDA tensors, on `stream`."""
        import torch
        nu = b.line_units(unit, trim, seed, doc_index_base, stream)
        res = {name: torch.empty(nu, dtype=getattr(torch, np.dtype(dt).name), device=device) for name, dt in _LINES_PER_UNIT}
        res["unit_off"] = torch.zeros(nd + 1, dtype=torch.int64, device=device)
        res.update({name: torch.empty(nd, dtype=getattr(torch, np.dtype(dt).name), device=device) for name, dt in _LINES_PER_DOC})
        b.line_repeats(unit, trim, mark_first, seed, doc_index_base, stream, **{name: t.data_ptr() for name, t in res.items() if t.numel()})
        return res

    def repetition_signals(self, texts, top=(2, 3, 4), dup=(5, 6, 7, 8, 9, 10), mark_first=False, seed=0, ordinary=True, allowed_special=None,
                           lines=False, trim=False):
        """The fractions the repetition filters of Gopher (Rae et al. 2021, table A1) put a threshold on, for a list of str/bytes:
        {"top": {n: (token_fraction, byte_fraction)}, "dup": {n: (token_fraction, byte_fraction)}, "n_tokens": int64 [n_docs],
        "n_bytes": int64 [n_docs], "status": int32 [n_docs]}, the fractions numpy float64 [n_docs].
          top[n]  the share of the document inside its most frequent n-gram: top_count * n / l in tokens, and top_count * the
                  bytes of t[top_first .. top_first + n) / the document's bytes.
          dup[n]  the share inside n-grams that occur more than once: n_covered / l in tokens, the bytes of the covered tokens /
                  the document's bytes.  mark_first: as for ngram_repeats_batch.
        0.0 for a document without n-grams.  One encode, one jtk_batch_ngram_repeats pass per n; token byte lengths come from
        jtk_batch_token_offsets and the sums are done with torch on the device: no ids on the host.
          lines=True adds the four line-level signals of the same table, from the same encode (jtk_batch_line_repeats):
                  "dup_line" and "dup_paragraph", each (unit_fraction, byte_fraction, char_fraction) = n_dup / the document's
                  units, dup_bytes / the document's bytes, dup_chars / doc_chars -- 0.0 where the denominator is 0 --, and
                  "n_lines", "n_paragraphs" int64 [n_docs].  trim as for line_repeats_batch; mark_first applies here too."""
        import torch
        bs, text, doc_off = _join_texts(texts)
        nd = len(bs)
        top, dup = [int(n) for n in top], [int(n) for n in dup]
        empty = lambda: (np.zeros(nd, dtype=np.float64), np.zeros(nd, dtype=np.float64))
        if nd == 0 or not len(text):
            out = {"top": {n: empty() for n in top}, "dup": {n: empty() for n in dup}, "n_tokens": np.zeros(nd, dtype=np.int64),
                   "n_bytes": np.zeros(nd, dtype=np.int64), "status": np.zeros(nd, dtype=np.int32)}
            if lines:
                out.update({"dup_line": empty() + empty()[:1], "dup_paragraph": empty() + empty()[:1],
                            "n_lines": np.zeros(nd, dtype=np.int64), "n_paragraphs": np.zeros(nd, dtype=np.int64)})
            return out
        device = torch.device("cuda", N.lib().jtk_encoding_device(self._h))
        d_off = torch.from_numpy(doc_off).to(device)
        d_text = torch.from_numpy(text.copy()).to(device)                        # (a copy: frombuffer views are read-only)
        self._check_device_inputs("repetition_signals", ("text", d_text, torch.uint8), ("doc_off", d_off, torch.int64))
        allow = self._allow(self._b(), allowed_special)
        tops, dups = {}, {}
        with self._encode_device_batch(d_text, d_off, ordinary, allow) as (b, _, _, stream):
            nt = b.result()[0]
            pos = torch.empty(nt, dtype=torch.int64, device=device)
            if nt:
                b.token_offsets(pos.data_ptr(), stream)
            for n in top:
                tops[n] = (torch.empty(nd, dtype=torch.int32, device=device), torch.empty(nd, dtype=torch.int64, device=device))
                b.ngram_repeats(n, None, None, None, tops[n][0].data_ptr(), tops[n][1].data_ptr(), seed=seed, stream=stream)
            for n in dup:
                dups[n] = (torch.empty(nt, dtype=torch.uint8, device=device), torch.empty(nd, dtype=torch.int32, device=device))
                b.ngram_repeats(n, dups[n][0].data_ptr() if nt else None, None, dups[n][1].data_ptr(), None, None, seed=seed,
                                mark_first=mark_first, stream=stream)
            units = {}
            if lines:
                for name in ("line", "paragraph"):
                    units[name] = self._line_repeats_on(b, nd, device, stream, name, trim, mark_first, seed, 0)
            tok_off, status = self._tok_off_and_status(b, nd, device, stream)
        # (joined into torch's current stream: the sums follow the passes)
        l = tok_off[1:] - tok_off[:-1]
        n_bytes = d_off[1:] - d_off[:-1]
        has = l > 0
        end = torch.cat([pos[1:], d_off[-1:]]) if nt else pos
        if nt:
            end[tok_off[1:][has] - 1] = d_off[1:][has]                           # a document's last token ends where the document does
        cum = torch.zeros(nt + 1, dtype=torch.int64, device=device)              # cum[t] = the bytes of the tokens before t
        cum[1:] = torch.cumsum(end - pos, 0)
        lf, bf = l.clamp(min=1).double(), n_bytes.clamp(min=1).double()
        out = {"top": {}, "dup": {}}
        for n in top:
            count, first = tops[n][0].long(), tops[n][1]
            at = (tok_off[:-1] + first.clamp(min=0)).clamp(max=max(nt - n, 0))
            gram = torch.where(count > 0, cum[(at + n).clamp(max=nt)] - cum[at], torch.zeros_like(at))
            out["top"][n] = (((count * n).double() / lf).cpu().numpy(), ((count * gram).double() / bf).cpu().numpy())
        for n in dup:
            flags, covered = dups[n]
            ccum = torch.zeros(nt + 1, dtype=torch.int64, device=device)
            ccum[1:] = torch.cumsum((end - pos) * ((flags & N.JTK_RP_COVERED) != 0), 0)
            cbytes = ccum[tok_off[1:]] - ccum[tok_off[:-1]]
            out["dup"][n] = ((covered.double() / lf).cpu().numpy(), (cbytes.double() / bf).cpu().numpy())
        frac = lambda num, den: torch.where(den > 0, num.double() / den.clamp(min=1).double(), torch.zeros_like(num, dtype=torch.float64)).cpu().numpy()
        for name, r in units.items():
            n_units = r["unit_off"][1:] - r["unit_off"][:-1]
            out["dup_" + name] = (frac(r["n_dup"].long(), n_units), frac(r["dup_bytes"], n_bytes), frac(r["dup_chars"], r["doc_chars"]))
            out["n_%ss" % name] = n_units.cpu().numpy()
        out["n_tokens"], out["n_bytes"], out["status"] = l.cpu().numpy(), n_bytes.cpu().numpy(), status.cpu().numpy()
        return out

    def near_duplicates(self, texts, threshold=0.8, ngram=5, num_hashes=128, bands=16, seed=0, ordinary=True, allowed_special=None):
        """Clusters of near-duplicate documents by MinHash and LSH: int64 [n] labels, the smallest document index of each
        document's cluster.  Per band the documents that have shingles are stable-sorted by band key on the device and every
        two consecutive ones with equal keys are a candidate pair; the pairs of all bands, made unique, are verified by
        signature agreement (minhash_agree) and those with agree >= ceil(threshold * num_hashes) are joined (union-find on the
        host).  A document without shingles (empty or refused) is its own cluster.  Deterministic: the same texts and
        parameters give the same labels on every device."""
        import math
        import torch
        if bands < 1:
            raise ValueError("near_duplicates needs bands >= 1")
        bs, text, doc_off = _join_texts(texts)
        n = len(bs)
        labels = np.arange(n, dtype=np.int64)
        if n < 2:
            return labels
        device = torch.device("cuda", N.lib().jtk_encoding_device(self._h))
        if not len(text):
            return labels
        doc_off = torch.from_numpy(doc_off).to(device)
        text = torch.from_numpy(text.copy()).to(device)                          # (a copy: frombuffer views are read-only)
        sig, n_shingles, band_keys, _, _ = self.minhash_batch_device(text, doc_off, ngram, num_hashes, bands, seed, ordinary, allowed_special)
        live = torch.nonzero(n_shingles > 0).flatten()
        if live.numel() < 2:
            return labels
        codes = []
        for j in range(bands):
            keys, order = torch.sort(band_keys[live, j], stable=True)
            docs = live[order]
            eq = keys[1:] == keys[:-1]
            codes.append(docs[:-1][eq] * n + docs[1:][eq])
        codes = torch.unique(torch.cat(codes))
        if codes.numel() == 0:
            return labels
        pa = torch.div(codes, n, rounding_mode="floor").contiguous()
        pb = (codes - pa * n).contiguous()
        agree = torch.empty(codes.numel(), dtype=torch.int32, device=device)
        b = self._b()
        with self._on_current_stream(b, device) as stream:
            b.minhash_agree(sig.data_ptr(), n, num_hashes, pa.data_ptr(), pb.data_ptr(), codes.numel(), agree.data_ptr(), stream)
        keep = agree >= int(math.ceil(threshold * num_hashes))
        pa, pb = pa[keep].cpu().numpy(), pb[keep].cpu().numpy()
        parent = list(range(n))

        def find(x):
            while parent[x] != x:
                parent[x] = parent[parent[x]]
                x = parent[x]
            return x

        for a, c in zip(pa.tolist(), pb.tolist()):
            ra, rc = find(a), find(c)
            if ra != rc:
                parent[max(ra, rc)] = min(ra, rc)        # (the root is the component's smallest index)
        for d in range(n):
            labels[d] = find(d)
        return labels

    def special_ids(self, allowed_special):
        """"all" or an iterable of special-token literals -> their ids (ValueError for a literal that is no special token)."""
        if isinstance(allowed_special, str):
            if allowed_special != "all":
                raise ValueError('allowed_special must be "all" or an iterable of special-token literals')
            return sorted(set(self._specials.values()))
        ids = []
        for lit in allowed_special:
            key = lit.decode("utf-8") if isinstance(lit, (bytes, bytearray)) else lit
            if key not in self._specials:
                raise ValueError("%r is not a special token of %s" % (lit, self._name))
            ids.append(self._specials[key])
        return ids

    def _allow(self, b, allowed_special):
        """Sets the batch's allowed set for allowed_special (not None); returns whether the encode takes the flag."""
        if allowed_special is None:
            return False
        if self._host_pattern is not None:
            raise ValueError("allowed_special: the device cannot run this encoding's custom split pattern")
        b.set_allowed_special(self.special_ids(allowed_special))
        return True

    def encode_with_special_tokens(self, text, allowed_special="all", ordinary=False):
        """tiktoken's encode(text, allowed_special=...) for one document, through a batch of one: the allowed literals become
        their ids, the text between them is encodeOrdinary() of each segment.  Without `ordinary`, a literal outside the
        allowed set raises UnsupportedOperationError, as encode() does; with it, such literals are ordinary text."""
        if text is None:
            return []
        _, text_u8, doc_off = _join_texts([text])
        res = self.encode_batch_packed(text_u8, doc_off, ordinary, False, allowed_special)
        if res.status[0] < 0:
            _check(int(res.status[0]))
        return res.tokens.tolist()

    def _match_on_host(self, text_u8, doc_off):
        """while (matcher.find()) over every document (GptBytePairEncoding.java:77-80) -> byte ranges of the matches."""
        raw = np.ascontiguousarray(text_u8, dtype=np.uint8).tobytes()
        pb, pe = [], []
        for d in range(len(doc_off) - 1):
            lo, hi = int(doc_off[d]), int(doc_off[d + 1])
            doc = raw[lo:hi].decode("utf-8")
            # character index -> byte offset
            pos = 0
            ci = 0
            for m in self._host_pattern.finditer(doc):
                s, e = m.span()
                if e == s:
                    continue
                pos += len(doc[ci:s].encode("utf-8"))
                nb = len(doc[s:e].encode("utf-8"))
                pb.append(lo + pos)
                pe.append(lo + pos + nb)
                pos += nb
                ci = e
        return np.array(pb, dtype=np.int64), np.array(pe, dtype=np.int64)

    def encode_batch_max_tokens(self, texts, max_tokens, ordinary=False):
        """List of str/bytes -> list of EncodingResult, as Encoding.encode(text, maxTokens) gives for each.  Only the leading
        bytes of each document are encoded (jtk_batch_encode_max_tokens), as the reference stops matching at maxTokens."""
        bs, text, doc_off = _join_texts(texts)
        if self._host_pattern is not None or len(bs) * max(0, int(max_tokens)) > (1 << 28):
            # a custom pattern (matched on the host), or a limit so large that n_docs x max_tokens ids are no sensible array:
            # encode whole, cut on the device
            res = self.encode_batch_packed(text, doc_off, ordinary)
            b = self._b()
            if len(res.status) and res.status.min() < 0:
                _check(int(res.status.min()))
            kept, flag = b.truncate(max(0, int(max_tokens)))
            return [EncodingResult(res.tokens[res.tok_off[d]:res.tok_off[d] + kept[d]].tolist(), bool(flag[d])) for d in range(len(bs))]
        toks, kept, flag, status = self._b().encode_max_tokens(text, doc_off, max_tokens, ordinary)
        if len(status) and status.min() < 0:
            _check(int(status.min()))
        return [EncodingResult(toks[d, :kept[d]].tolist(), bool(flag[d])) for d in range(len(bs))]

    def encode_batch_max_tokens_device(self, text, doc_off, max_tokens, ordinary=False, pad_id=-1, out=None):
        """Encoding.encode(text, maxTokens) / encodeOrdinary for every document of a device-resident batch, in a model's layout.
        text: CUDA torch.uint8 tensor, doc_off: CUDA torch.int64 tensor [n_docs + 1], on this encoding's device.  Returns CUDA
        tensors (tokens int32 [n_docs, max_tokens] -- `out` if given --, kept int64, truncated bool, status int32), written on
        torch.cuda.current_stream().  Per-document statuses come back in `status`; they do not raise."""
        import torch
        self._check_device_inputs("encode_batch_max_tokens_device", ("text", text, torch.uint8), ("doc_off", doc_off, torch.int64))
        mt = int(max_tokens)
        if mt < 0:
            raise ValueError("max_tokens must be >= 0")
        nd = self._n_docs(doc_off)
        device = text.device
        if out is None:
            out = torch.empty((nd, mt), dtype=torch.int32, device=device)
        elif (not isinstance(out, torch.Tensor) or out.shape != (nd, mt) or out.dtype != torch.int32 or out.device != device
              or not out.is_contiguous()):
            raise ValueError("out must be a contiguous int32 tensor of shape (%d, %d) on %s" % (nd, mt, device))
        kept = torch.empty(nd, dtype=torch.int64, device=device)
        truncated = torch.empty(nd, dtype=torch.bool, device=device)
        status = torch.empty(nd, dtype=torch.int32, device=device)
        if nd > 0:
            stream = torch.cuda.current_stream(device).cuda_stream
            self._b().encode_device_max_tokens(text.data_ptr(), doc_off.data_ptr(), nd, text.numel(), mt, out.data_ptr(),
                                               kept.data_ptr(), truncated.data_ptr(), status.data_ptr(), ordinary, pad_id, stream)
        return out, kept, truncated, status

    def chunk_batch(self, texts, chunk_tokens, overlap=0, ordinary=False, allowed_special=None, unit="byte", prefer=None,
                    min_tokens=None):
        """Every text cut into consecutive chunks of at most chunk_tokens tokens (overlapping by up to `overlap` tokens), each a
        whole number of characters unless the tokens do not allow it: per document a list of (tokens, start, end, split), with
        start / end byte positions in that document (jtk_batch_chunk; the rule is in jtk_chunk_rules.h).  The chunks are
        slices of encode(text); with overlap 0 they concatenate to it.  A document that cannot be encoded raises.
        allowed_special: as for encode_batch (a special token's byte span is its literal).
        unit: "byte" (default), "char" -- start / end are indices into the Python str, text[start:end] is the chunk's text -- or
        "utf16", indices into a Java String (start rounds down, end up, to a character for a split chunk).
        prefer (an iterable of "word", "sentence", "line", "paragraph", the string "all", or a JTK_CUT_* mask) and / or
        min_tokens (default (chunk_tokens + 1) // 2): the chunks end at the best such boundary between min_tokens and
        chunk_tokens and overlaps start on one (jtk_batch_chunk_prefer; the rule is in jtk_chunk_prefer_rules.h), and the tuples
        gain a fifth field, the JTK_LEVEL_* of the chunk's end (6: the document's end)."""
        u = self._char_unit(unit, "chunk_batch")
        leveled = prefer is not None or min_tokens is not None
        bs, text, doc_off = _join_texts(texts)
        res = self.encode_batch_packed(text, doc_off, ordinary, False, allowed_special)
        if len(res.status) and res.status.min() < 0:
            _check(int(res.status.min()))
        b = self._b()
        if leveled:
            b.chunk_prefer(chunk_tokens, overlap, min_tokens, 0 if prefer is None else prefer)
        else:
            b.chunk(chunk_tokens, overlap)
        f = b.chunk_fetch()
        level = b.chunk_levels()[0] if leveled else None
        nc = len(f["doc"])
        start, end = f["byte_begin"] - doc_off[f["doc"]], f["byte_end"] - doc_off[f["doc"]]
        if u is not None and nc:
            p_doc, p_bb, p_be = (b.chunk_device_result()[i] for i in (1, 4, 5))
            with _device_arrays() as put:
                d_start, d_end = put(np.zeros(nc, dtype=np.int64)), put(np.zeros(nc, dtype=np.int64))
                b.char_positions(u, p_bb, nc, d_start.ptr, "floor", p_doc)
                b.char_positions(u, p_be, nc, d_end.ptr, "ceil", p_doc)
                _stream_sync(b.stream())
                start, end = d_start.fetch(), d_end.fetch()
        out = [[] for _ in bs]
        for c in range(nc):
            d, tb, n = int(f["doc"][c]), int(f["tok_begin"][c]), int(f["n_tok"][c])
            rec = (res.tokens[tb:tb + n].tolist(), int(start[c]), int(end[c]), bool(f["split"][c]))
            out[d].append(rec + (int(level[c]),) if leveled else rec)
        return out

    def chunk_batch_device(self, text, doc_off, chunk_tokens, overlap=0, ordinary=False, pad_id=-1, allowed_special=None, unit=None,
                           prefer=None, min_tokens=None):
        """chunk_batch for a device-resident batch, in a model's layout.  text: CUDA torch.uint8 tensor, doc_off: CUDA torch.int64
        tensor [n_docs + 1], on this encoding's device.  Returns a dict of CUDA tensors written on torch.cuda.current_stream():
        rows int32 [n_chunks, chunk_tokens] (the chunk's ids, then pad_id), n_tok int32, doc int64, byte_begin / byte_end int64
        (positions in `text`), split bool [n_chunks], chunk_off int64 [n_docs + 1] and the per-document status int32 (documents
        with a negative status have no chunks; they do not raise).  The call waits once, for the chunk count (and, with
        allowed_special -- as for encode_batch --, once more for the encode's count of literal candidates).
        unit ("char", "utf16" or a JTK_UNIT_* value): the dict also holds char_begin / char_end int64 [n_chunks], the chunk's
        range in that unit, relative to its document (begin rounded down, end up); byte_begin / byte_end stay as they are.
        prefer / min_tokens: as for chunk_batch (jtk_batch_chunk_prefer); the dict then also holds level uint8 [n_chunks], the
        JTK_LEVEL_* of every chunk's end, and the call waits for the encode before it waits for the chunk count."""
        import torch
        self._check_device_inputs("chunk_batch_device", ("text", text, torch.uint8), ("doc_off", doc_off, torch.int64))
        leveled = prefer is not None or min_tokens is not None
        mask = prefer_mask(0 if prefer is None else prefer)
        u = None if unit is None else _unit(unit)
        allow = self._allow(self._b(), allowed_special)
        N_, ov = int(chunk_tokens), int(overlap)
        if N_ < 1 or not 0 <= ov < N_:
            raise ValueError("need chunk_tokens >= 1 and 0 <= overlap < chunk_tokens")
        with self._encode_device_batch(text, doc_off, ordinary, allow) as (b, nd, device, stream):
            nc = b.chunk_prefer(N_, ov, min_tokens, mask, stream) if leveled else b.chunk(N_, ov, stream)
            out = dict.fromkeys(("rows", "n_tok", "doc", "byte_begin", "byte_end", "split", "chunk_off", "status"))   # (their order)
            out["rows"] = torch.empty((nc, N_), dtype=torch.int32, device=device)
            b.chunk_rows(pad_id, out["rows"].data_ptr(), stream)
            p_off, p_doc, _, p_ntok, p_bb, p_be, p_split = b.chunk_device_result()
            p_status = b.device_result()[2]
            for key, src, n, dt in (("chunk_off", p_off, nd + 1, torch.int64), ("doc", p_doc, nc, torch.int64),
                                    ("n_tok", p_ntok, nc, torch.int32), ("byte_begin", p_bb, nc, torch.int64),
                                    ("byte_end", p_be, nc, torch.int64), ("split", p_split, nc, torch.bool),
                                    ("status", p_status, nd, torch.int32)):
                out[key] = _device_copy(src, n, dt, device, stream)
            if leveled:
                out["level"] = _device_copy(b.chunk_levels_device() if nc else None, nc, torch.uint8, device, stream)
            if u is not None:
                out["char_begin"] = torch.empty(nc, dtype=torch.int64, device=device)
                out["char_end"] = torch.empty(nc, dtype=torch.int64, device=device)
                if nc:
                    b.char_positions(u, p_bb, nc, out["char_begin"].data_ptr(), "floor", p_doc, stream)
                    b.char_positions(u, p_be, nc, out["char_end"].data_ptr(), "ceil", p_doc, stream)
        return out

    def _sep_id(self, sep):
        """None -> -1, a special-token literal -> its id, an int -> itself."""
        if sep is None:
            return -1
        if isinstance(sep, (str, bytes, bytearray)):
            key = sep.decode("utf-8") if isinstance(sep, (bytes, bytearray)) else sep
            if key not in self._specials:
                raise ValueError("%r is not a special token of %s" % (sep, self._name))
            return self._specials[key]
        return int(sep)

    @staticmethod
    def _batch_spans(train_spans, doc_off, doc_units=None):
        """Per-document (start, end) byte ranges -> sorted batch positions (begin, end int64), checked.  With doc_units (the
        documents' lengths in characters or UTF-16 units) the ranges are in that unit: (doc, begin, end int64), begin / end
        still relative to their document, for jtk_batch_byte_positions."""
        nd = len(doc_off) - 1
        if len(train_spans) != nd:
            raise ValueError("train_spans needs one list of (start, end) per text (%d for %d texts)" % (len(train_spans), nd))
        begin, end, doc = [], [], []
        for d, spans in enumerate(train_spans):
            n, prev = int(doc_off[d + 1] - doc_off[d]) if doc_units is None else int(doc_units[d]), 0
            for a, e in spans or ():
                a, e = int(a), int(e)
                if a < 0 or e < a or e > n:
                    if doc_units is not None:
                        raise ValueError("train_spans[%d]: (%d, %d) is not a character range inside the text (%d units)" % (d, a, e, n))
                    raise ValueError("train_spans[%d]: (%d, %d) is not a byte range inside the text (%d bytes)" % (d, a, e, n))
                if a < prev:
                    raise ValueError("train_spans[%d]: (%d, %d) starts before the previous range ends: ranges must be sorted "
                                     "and must not overlap" % (d, a, e))
                prev = e
                base = int(doc_off[d]) if doc_units is None else 0
                begin.append(base + a)
                end.append(base + e)
                doc.append(d)
        if doc_units is not None:
            return np.array(doc, dtype=np.int64), np.array(begin, dtype=np.int64), np.array(end, dtype=np.int64)
        return np.array(begin, dtype=np.int64), np.array(end, dtype=np.int64)

    def pack_batch(self, texts, seq_len, sep=None, sep_first=False, whole_docs=False, drop_last=False, pad_id=-1, ordinary=False,
                   allowed_special=None, train_spans=None, span_rule="whole", label_shift=False, label_sep=False,
                   ignore_index=-100, span_unit="byte", fim=None):
        """Every text encoded, then packed into rows of seq_len tokens (jtk_batch_pack; the rule is in jtk_pack_rules.h): a dict
        of numpy arrays rows, positions int32 [n_rows, seq_len], cu_seqlens int32 [n_segments + 1], seg_doc int64
        [n_segments], status int32 [n_docs] and max_seqlen (int).  sep: None, a token id or a special-token literal such as
        "<|endoftext|>", after each document (or before it with sep_first).  whole_docs: next-fit of whole documents instead of
        one concatenated stream; drop_last (concat only): omit a partial last row.  Documents with a negative status are left
        out (they do not raise).
        train_spans: per text a list of (start, end) byte ranges inside that text, sorted and not overlapping (ValueError
        otherwise; an empty list: nothing of the text is trained on).  The result then also holds labels int32
        [n_rows, seq_len] -- a cell's id where its token lies in a range by span_rule ("whole": entirely inside, "start": its
        first byte, "any": any byte), ignore_index elsewhere, on separators (unless label_sep, for a separator after a trainable
        last token) and on pad; label_shift: next-token targets within each segment -- and tok_span int32 [n_tokens], each
        token's range (numbered over the batch) or -1.  The rule is in jtk_label_rules.h.
        span_unit: "byte" (default), or "char" / "utf16": train_spans are ranges of the Python str / of a Java String, checked
        against the texts' lengths in that unit and converted on the device (jtk_batch_byte_positions).
        fim: a FimParams for the encode (with ordinary=True; see encode_batch); the dict then also holds fim_kind, fim_cut and
        fim_part_tok.  Together with train_spans it raises ValueError: a rearranged document has no positions in the text."""
        if fim is not None and train_spans is not None:
            raise ValueError("fim= and train_spans= do not combine: after the transformation tokens have no positions in the text")
        su = self._char_unit(span_unit, "pack_batch") if train_spans is not None else None
        bs, text, doc_off = _join_texts(texts)
        sep_id = self._sep_id(sep)
        if train_spans is not None:
            rule = _span_rule(span_rule)
            if su is None:
                begin, end = self._batch_spans(train_spans, doc_off)
            elif len(train_spans) != len(bs):
                self._batch_spans(train_spans, doc_off)                     # (raises: one list per text)
        res = self.encode_batch_packed(text, doc_off, ordinary, False, allowed_special, fim=fim)
        b = self._b()
        _, _, mx = b.pack(seq_len, sep_id, whole_docs, sep_first, drop_last)
        f = b.pack_fetch(pad_id)
        f["status"] = res.status.copy()
        if fim is not None:
            f["fim_kind"], f["fim_cut"], f["fim_part_tok"] = res.fim_kind, res.fim_cut, res.fim_part_tok
        f["max_seqlen"] = mx
        if train_spans is not None:
            with _device_arrays() as put:
                if su is not None:
                    # the ranges are checked against the documents' lengths in the unit, then become byte positions on the device
                    units = put(np.zeros(max(len(bs), 1), dtype=np.int64))
                    b.char_index(su, units.ptr)
                    _stream_sync(b.stream())
                    doc, begin, end = self._batch_spans(train_spans, doc_off, units.fetch()[:len(bs)])
                    d_doc, d_begin, d_end = put(doc), put(begin), put(end)
                    b.byte_positions(su, d_doc.ptr, d_begin.ptr, len(doc), d_begin.ptr)     # (in place: one lane per entry)
                    b.byte_positions(su, d_doc.ptr, d_end.ptr, len(doc), d_end.ptr)
                else:
                    d_begin, d_end = put(begin), put(end)
                d_span = put(np.zeros(len(res.tokens), dtype=np.int32))
                b.token_spans(d_begin.ptr, d_end.ptr, len(begin), rule, d_span.ptr)
                f["labels"] = b.pack_labels_fetch(d_span.ptr, ignore_index, label_shift, label_sep)   # (synchronises)
                f["tok_span"] = d_span.fetch()
        return f

    def _check_device_spans(self, text, span_begin, span_end):
        import torch
        for name, t in (("span_begin", span_begin), ("span_end", span_end)):
            if not isinstance(t, torch.Tensor) or t.device.type != "cuda" or t.dtype != torch.int64 or t.dim() != 1:
                raise ValueError("%s must be a 1-d CUDA tensor of torch.int64" % name)
            if t.device != text.device:
                raise ValueError("%s is on %s, the text on %s" % (name, t.device, text.device))
            if not t.is_contiguous():
                raise ValueError("%s must be contiguous" % name)
        if span_begin.numel() != span_end.numel():
            raise ValueError("span_begin and span_end must have the same length")

    def pack_batch_device(self, text, doc_off, seq_len, sep=None, sep_first=False, whole_docs=False, drop_last=False, pad_id=-1,
                          ordinary=False, allowed_special=None, span_begin=None, span_end=None, span_rule="whole",
                          label_shift=False, label_sep=False, ignore_index=-100, fim=None):
        """pack_batch for a device-resident batch.  text: CUDA torch.uint8 tensor, doc_off: CUDA torch.int64 tensor [n_docs + 1],
        on this encoding's device.  Returns a dict of CUDA tensors written on torch.cuda.current_stream(): rows int32
        [n_rows, seq_len], positions int32 [n_rows, seq_len], cu_seqlens int32 [n_segments + 1], seg_doc int64 [n_segments],
        status int32 [n_docs], and max_seqlen as a Python int -- what a varlen attention call takes.  The call waits once, for
        the counts (and, with allowed_special, once more for the encode's count of literal candidates).
        span_begin / span_end: CUDA torch.int64 tensors of equal length, byte ranges [begin, end) in positions of `text`, sorted
        and disjoint (not checked: ranges out of order give unspecified labels).  The dict then also holds labels int32
        [n_rows, seq_len] and tok_span int32 [n_tokens], as pack_batch describes them, written on the same stream; the token
        count costs one more wait.
        fim: a FimParams for the encode (with ordinary=True; not with spans: ValueError); the dict then also holds fim_kind uint8
        [n_docs], fim_cut int64 [n_docs, 2] and fim_part_tok int64 [n_docs, 3], written on the same stream."""
        import torch
        self._check_device_inputs("pack_batch_device", ("text", text, torch.uint8), ("doc_off", doc_off, torch.int64))
        if (span_begin is None) != (span_end is None):
            raise ValueError("span_begin and span_end go together")
        if fim is not None and span_begin is not None:
            raise ValueError("fim= and spans do not combine: after the transformation tokens have no positions in the text")
        if span_begin is not None:
            self._check_device_spans(text, span_begin, span_end)
            rule = _span_rule(span_rule)
        L = int(seq_len)
        if L < 1:
            raise ValueError("seq_len must be >= 1")
        if whole_docs and drop_last:
            raise ValueError("drop_last applies to the concatenated stream only")
        sep_id = self._sep_id(sep)
        use_fim = self._fim(self._b(), fim, ordinary, allowed_special)
        allow = self._allow(self._b(), allowed_special)
        with self._encode_device_batch(text, doc_off, ordinary, allow, fim=use_fim) as (b, nd, device, stream):
            nr, ns, mx = b.pack(L, sep_id, whole_docs, sep_first, drop_last, stream)
            out = dict(rows=torch.empty((nr, L), dtype=torch.int32, device=device),
                       positions=torch.empty((nr, L), dtype=torch.int32, device=device),
                       cu_seqlens=torch.empty(ns + 1, dtype=torch.int32, device=device),
                       seg_doc=torch.empty(ns, dtype=torch.int64, device=device))
            b.pack_write(pad_id, out["rows"].data_ptr(), out["positions"].data_ptr(), out["cu_seqlens"].data_ptr(),
                         out["seg_doc"].data_ptr(), stream)
            # (the results are asked for only when there are documents to copy them for)
            out["status"] = _device_copy(b.device_result()[2] if nd else None, nd, torch.int32, device, stream)
            if use_fim:
                srcs = b.fim_device_result() if nd else (None, None, None)
                for key, shape, dt, src in zip(("fim_kind", "fim_cut", "fim_part_tok"), (nd, (nd, 2), (nd, 3)),
                                               (torch.uint8, torch.int64, torch.int64), srcs):
                    out[key] = _device_copy(src, shape, dt, device, stream)
            if span_begin is not None:
                nt = b.result()[0]
                out["tok_span"] = torch.empty(nt, dtype=torch.int32, device=device)
                out["labels"] = torch.empty((nr, L), dtype=torch.int32, device=device)
                b.token_spans(span_begin.data_ptr(), span_end.data_ptr(), span_begin.numel(), rule, out["tok_span"].data_ptr(), stream)
                b.pack_labels(out["tok_span"].data_ptr(), ignore_index, out["labels"].data_ptr(), label_shift, label_sep, stream)
        out["max_seqlen"] = mx
        return out

    def token_spans_device(self, text, doc_off, span_begin, span_end, rule="whole", ordinary=False, allowed_special=None):
        """For callers who do not pack: encodes a device-resident batch (text CUDA torch.uint8, doc_off CUDA torch.int64
        [n_docs + 1]) and returns (tok_span int32 [n_tokens], tok_off int64 [n_docs + 1], status int32 [n_docs]) as CUDA tensors
        written on torch.cuda.current_stream(): per token the lowest of the byte ranges [span_begin[i], span_end[i]) (CUDA
        torch.int64, positions in `text`, sorted and disjoint) that holds it by `rule`, or -1 (jtk_label_rules.h).  The ids
        stay in the batch (device_result).  Waits once, for the token count."""
        import torch
        self._check_device_inputs("token_spans_device", ("text", text, torch.uint8), ("doc_off", doc_off, torch.int64))
        self._check_device_spans(text, span_begin, span_end)
        rule = _span_rule(rule)
        allow = self._allow(self._b(), allowed_special)
        with self._encode_device_batch(text, doc_off, ordinary, allow) as (b, nd, device, stream):
            nt = b.result()[0]
            tok_span = torch.empty(nt, dtype=torch.int32, device=device)
            b.token_spans(span_begin.data_ptr(), span_end.data_ptr(), span_begin.numel(), rule, tok_span.data_ptr(), stream)
            tok_off, status = self._tok_off_and_status(b, nd, device, stream)
        return tok_span, tok_off, status

    def token_offsets_device(self, text, doc_off, unit="char", ordinary=False, allowed_special=None):
        """Encodes a device-resident batch (text CUDA torch.uint8, doc_off CUDA torch.int64 [n_docs + 1]) and returns (begin int64
        [n_tokens], end int64 [n_tokens], tok_off int64 [n_docs + 1], status int32 [n_docs]) as CUDA tensors written on
        torch.cuda.current_stream(): every token's range in its document in `unit` ("char", "utf16", "byte" or a JTK_UNIT_*
        value), begin rounded down and end up to a character (jtk_batch_token_char_offsets).  The ids stay in the batch
        (device_result).  Waits once, for the token count."""
        import torch
        self._check_device_inputs("token_offsets_device", ("text", text, torch.uint8), ("doc_off", doc_off, torch.int64))
        u = _unit(unit)
        allow = self._allow(self._b(), allowed_special)
        with self._encode_device_batch(text, doc_off, ordinary, allow) as (b, nd, device, stream):
            nt = b.result()[0]
            begin = torch.empty(nt, dtype=torch.int64, device=device)
            end = torch.empty(nt, dtype=torch.int64, device=device)
            b.token_char_offsets(u, begin.data_ptr() if nt else None, end.data_ptr() if nt else None, stream)
            tok_off, status = self._tok_off_and_status(b, nd, device, stream)
        return begin, end, tok_off, status

    def count_tokens_batch(self, texts, ordinary=False, allowed_special=None):
        """Encoding.countTokens / countTokensOrdinary for every text, one device call, no token ids written.  allowed_special:
        as for encode_batch."""
        _, text, doc_off = _join_texts(texts)
        b = self._b()
        b.encode_host(text, doc_off, ordinary, count_only=True, allow_special=self._allow(b, allowed_special))
        counts, status = b.fetch_counts()
        if len(status) and status.min() < 0:
            _check(int(status.min()))
        return counts.tolist()

    def decode_batch(self, token_lists, strict=True, stop_strings=None, search_from=None, keep_stop_string=False):
        """List of token-id lists -> list of bytes (Encoding.decodeBytes for each), one device call.
        strict: raise for a list with an unknown id, as the reference does (GptBytePairEncoding.java:313).
        stop_strings, search_from, keep_stop_string: as for decode_rows."""
        ids, seq_off = _join_ids(token_lists)
        b = self._b()
        b.decode_host(ids, seq_off)
        out, byte_off, status = b.decode_fetch()
        if strict and len(status) and status.min() < 0:
            q = int(np.argmin(status))
            raise EncodingError(int(status[q]), "Unknown token for decoding (list %d)" % q)
        raw = out.tobytes()
        if stop_strings is not None:
            return self._cut_at_stops(b, raw, byte_off, len(token_lists), stop_strings, search_from, keep_stop_string)
        return [raw[byte_off[q]:byte_off[q + 1]] for q in range(len(token_lists))]

    def _stop_ids(self, stop):
        """Ids or special-token literals -> ids (at most JTK_DECODE_MAX_STOP_IDS)."""
        if isinstance(stop, (int, np.integer, str, bytes, bytearray)):
            stop = (stop,)
        ids = [self._sep_id(x) for x in stop]
        if len(ids) > N.JTK_DECODE_MAX_STOP_IDS:
            raise ValueError("at most %d stop ids" % N.JTK_DECODE_MAX_STOP_IDS)
        return ids

    def decode_rows_device(self, rows, begin=None, end=None, pad_id=None, stop=(), keep_stop=False, cell_offsets=False,
                           stop_strings=None, search_from=None):
        """Encoding.decodeBytes for every row of a device-resident id matrix, as generate() or this library's padded rows hand
        it out (jtk_batch_decode_rows_device; the rule is in jtk_decode_rows_rules.h).  rows: 2-d CUDA torch.int32 / int64
        tensor on this encoding's device with stride(1) == 1 (a row-strided view is read in place); begin / end: CUDA int64
        [n_rows] or None, the window of columns of every row; pad_id: cells holding it are skipped (None: no cell is); stop:
        ids or special-token literals, the first of which ends its row (keep_stop: and is decoded too).  Returns a dict of CUDA
        tensors written on torch.cuda.current_stream(): bytes uint8, byte_off int64 [n_rows + 1], status int32 [n_rows] (0 or
        JTK_ERR_UNKNOWN_TOKEN; rows do not raise) and, with cell_offsets, cell_byte int64 [n_rows, width]: where in `bytes`
        every cell's bytes start.  The call waits as decode does: once for the size of the output, once at the end.
        stop_strings (a sequence of bytes / str, a str as its UTF-8 bytes; None: no search) runs jtk_batch_decode_find_stops over
        the rows' bytes and adds stop_pos int64, stop_which int32, hold int32 and stop_col int64, each [n_rows] (the rule is
        jtk_stop_rules.h; positions are bytes in `bytes`, UTF-16 positions of stops are not computed); search_from: CUDA int64
        [n_rows] or None, where in every row's bytes the search starts.  cell_byte is then computed for stop_col even without
        cell_offsets, but returned only with it."""
        import torch
        dev = N.lib().jtk_encoding_device(self._h)
        if (not isinstance(rows, torch.Tensor) or rows.device.type != "cuda" or rows.dim() != 2
                or rows.dtype not in (torch.int32, torch.int64)):
            raise ValueError("rows must be a 2-d CUDA tensor of torch.int32 or torch.int64")
        if rows.device.index != dev:
            raise ValueError("rows is on cuda:%s, the encoding on cuda:%d" % (rows.device.index, dev))
        nr, width = rows.shape
        stride = width
        if nr > 1 and width > 0:
            if rows.stride(1) != 1 or rows.stride(0) < width:
                raise ValueError("rows must have stride(1) == 1 and stride(0) >= width")
            stride = rows.stride(0)
        elif width > 1 and rows.stride(1) != 1:
            raise ValueError("rows must have stride(1) == 1 and stride(0) >= width")
        device = rows.device
        def check_per_row(name, t):
            if (not isinstance(t, torch.Tensor) or t.device != device or t.dtype != torch.int64 or t.dim() != 1 or t.numel() != nr
                    or not t.is_contiguous()):
                raise ValueError("%s must be a contiguous CUDA int64 tensor of n_rows entries on %s" % (name, device))
        for name, t in (("begin", begin), ("end", end)):
            if t is not None:
                check_per_row(name, t)
        if search_from is not None:
            if stop_strings is None:
                raise ValueError("search_from needs stop_strings")
            check_per_row("search_from", search_from)
        stop_ids = self._stop_ids(stop)
        b = self._b()
        with self._on_current_stream(b, device) as stream:
            want_cells = cell_offsets or stop_strings is not None
            cells = torch.empty((nr, width), dtype=torch.int64, device=device) if want_cells else None
            nb = b.decode_rows_device(rows.data_ptr() if nr * width else None, rows.element_size(), nr, width, stride,
                                      None if begin is None else begin.data_ptr(), None if end is None else end.data_ptr(),
                                      0 if pad_id is None else int(pad_id), stop_ids, pad_id is not None, keep_stop,
                                      cells.data_ptr() if want_cells and nr * width else None, stream)
            out = {}
            for key, n, dt, src in zip(("bytes", "byte_off", "status"), (nb, nr + 1, nr), (torch.uint8, torch.int64, torch.int32),
                                       b.decode_device_result()):
                out[key] = _device_copy(src, n, dt, device, stream)
            if cell_offsets:
                out["cell_byte"] = cells
            if stop_strings is not None:
                b.decode_find_stops(stop_strings, None if search_from is None else search_from.data_ptr(),
                                    cells.data_ptr() if nr * width else None, width, stream)
                for key, dt, src in zip(("stop_pos", "stop_which", "hold", "stop_col"), (torch.int64, torch.int32, torch.int32, torch.int64),
                                        b.decode_stops_device_result()):
                    out[key] = _device_copy(src, nr, dt, device, stream)
        return out

    def _cut_at_stops(self, b, raw, byte_off, n, stop_strings, search_from, keep_stop_string):
        """The sequences of the batch's last decode, cut at the first stop string (jtk_batch_decode_find_stops): search_from is
        a host array of n byte offsets or None; keep_stop_string keeps the matched string at the end of its sequence."""
        bs = _stop_blob(stop_strings)
        lens = np.diff(bs[1].astype(np.int64))
        with _device_arrays() as put:
            d_from = None
            if search_from is not None:
                f = np.ascontiguousarray(search_from, dtype=np.int64)
                if f.shape != (n,):
                    raise ValueError("search_from needs one entry per sequence")
                d_from = put(f).ptr
            b.decode_find_stops(stop_strings, d_from)
            pos, which, _, _ = b.decode_stops_fetch()
        return [raw[byte_off[q]:pos[q] + (int(lens[which[q]]) if keep_stop_string and which[q] >= 0 else 0)] for q in range(n)]

    def decode_rows(self, rows, begin=None, end=None, pad_id=None, stop=(), keep_stop=False, strict=True, stop_strings=None,
                    search_from=None, keep_stop_string=False):
        """The same for a numpy id matrix (2-d, int32 or int64) -> list of bytes, one per row.  strict: raise for a row with an
        unknown id among its decoded cells, as decode_batch does.  stop_strings: every row is cut at its first stop string
        (found on the device: jtk_batch_decode_find_stops), searched from byte search_from[r] of the row (a host array, None:
        0); keep_stop_string: the matched string stays at the row's end."""
        b = self._b()
        rows = np.asarray(rows)
        b.decode_rows_host(rows, begin, end, 0 if pad_id is None else int(pad_id), self._stop_ids(stop), pad_id is not None, keep_stop)
        out, byte_off, status = b.decode_fetch()
        if strict and len(status) and status.min() < 0:
            q = int(np.argmin(status))
            raise EncodingError(int(status[q]), "Unknown token for decoding (row %d)" % q)
        raw = out.tobytes()
        if stop_strings is not None:
            return self._cut_at_stops(b, raw, byte_off, rows.shape[0], stop_strings, search_from, keep_stop_string)
        return [raw[byte_off[q]:byte_off[q + 1]] for q in range(rows.shape[0])]

    # ---- UTF-16 in and out: a Java String's char[] crosses as it is (the rules are jtk_utf16_rules.h) -------------
    def encode_batch_utf16(self, units, unit_off, ordinary=False, allowed_special=None):
        """numpy uint16 units (a String's chars, documents back to back) and int64 unit_off [n_docs + 1] -> BatchResult: the
        tokens of String.getBytes(UTF_8) of every document, transcoded and encoded on the device (jtk_batch_encode_utf16: one
        upload, not chunk-pipelined).  allowed_special: as for encode_batch."""
        if self._host_pattern is not None:
            raise ValueError("encode_batch_utf16: the device cannot run this encoding's custom split pattern")
        b = self._b()
        b.encode_utf16_host(units, unit_off, ordinary, allow_special=self._allow(b, allowed_special))
        return b.fetch()

    def _check_utf16_inputs(self, what, units, unit_off):
        import torch
        self._check_device_inputs(what, ("units", units, torch.uint16), ("unit_off", unit_off, torch.int64))
        if unit_off.numel() < 1:
            raise ValueError("unit_off needs n_docs + 1 entries")

    def transcode_utf16_device(self, units, unit_off):
        """Device-resident UTF-16 (units CUDA torch.uint16, any 2-byte alignment; unit_off CUDA torch.int64 [n_docs + 1]) ->
        (utf8 uint8 [n_bytes], doc_off int64 [n_docs + 1]) as CUDA tensors written on torch.cuda.current_stream(): the rule of
        String.getBytes(UTF_8) per document (jtk_batch_transcode_utf16_device).  Waits once, for the byte count and the check of
        the offsets (EncodingError JTK_ERR_INVALID_ARGUMENT for offsets that decrease or leave [0, n_units])."""
        import torch
        self._check_utf16_inputs("transcode_utf16_device", units, unit_off)
        device, nd = units.device, unit_off.numel() - 1
        b = self._b()
        with self._on_current_stream(b, device) as stream:
            nb = b.transcode_utf16_device(units.data_ptr() if units.numel() else None, unit_off.data_ptr(), nd, units.numel(), stream)
            p_text, p_off, _ = b.utf8_device_result()
            utf8 = _device_copy(p_text, nb, torch.uint8, device, stream)
            doc_off = _device_copy(p_off, nd + 1, torch.int64, device, stream)
        return utf8, doc_off

    def encode_batch_utf16_device(self, units, unit_off, ordinary=False, allowed_special=None):
        """Encodes device-resident UTF-16 (as transcode_utf16_device takes it) -> (tokens int32 [n_tokens], tok_off int64
        [n_docs + 1], status int32 [n_docs], doc_off int64 [n_docs + 1]) as CUDA tensors written on torch.cuda.current_stream().
        doc_off are the documents' byte offsets in the transcoded text, which the batch keeps as the encode's text for the
        post-passes (chunk, pack, character positions: positions in "utf16" index the caller's units).  Waits for the byte
        count and the token count."""
        import torch
        self._check_utf16_inputs("encode_batch_utf16_device", units, unit_off)
        b = self._b()
        allow = self._allow(b, allowed_special)
        device, nd = units.device, unit_off.numel() - 1
        with self._on_current_stream(b, device) as stream:
            nt = b.encode_utf16_device(units.data_ptr() if units.numel() else None, unit_off.data_ptr(), nd, units.numel(), ordinary,
                                       stream=stream, allow_special=allow)
            p_tok, p_off, p_status = b.device_result()
            tokens = _device_copy(p_tok, nt, torch.int32, device, stream)
            tok_off = _device_copy(p_off, nd + 1, torch.int64, device, stream)
            status = _device_copy(p_status, nd, torch.int32, device, stream)
            doc_off = _device_copy(b.utf8_device_result()[1], nd + 1, torch.int64, device, stream)
        return tokens, tok_off, status, doc_off

    def decode_batch_utf16(self, token_lists, strict=True):
        """List of token-id lists -> list of str: new String(decodeBytes(tokens), UTF_8) for each, decoded and transcoded to
        UTF-16 units on the device (jtk_batch_decode_utf16: one U+FFFD per maximal ill-formed subpart).  strict: as decode_batch."""
        ids, seq_off = _join_ids(token_lists)
        b = self._b()
        b.decode_host(ids, seq_off)
        b.decode_utf16()
        units, unit_off, status = b.decode_utf16_fetch()
        if strict and len(status) and status.min() < 0:
            q = int(np.argmin(status))
            raise EncodingError(int(status[q]), "Unknown token for decoding (list %d)" % q)
        raw = units.tobytes()
        return [raw[2 * unit_off[q]:2 * unit_off[q + 1]].decode("utf-16-le", "surrogatepass") for q in range(len(token_lists))]

    def decode_rows_utf16_device(self, rows, begin=None, end=None, pad_id=None, stop=(), keep_stop=False, cell_offsets=False,
                                 stop_strings=None, search_from=None):
        """decode_rows_device, then the rows' bytes as UTF-16 units (jtk_batch_decode_utf16).  Returns its dict with, added, units
        uint16 and unit_off int64 [n_rows + 1] (CUDA tensors written on torch.cuda.current_stream()): row r is
        units[unit_off[r]:unit_off[r + 1]], new String(bytes of row r, UTF_8).  status is the decode's.  stop_strings /
        search_from: as for decode_rows_device; the stops are positions in `bytes`, not in `units`."""
        import torch
        out = self.decode_rows_device(rows, begin, end, pad_id, stop, keep_stop, cell_offsets, stop_strings, search_from)
        device, nr = rows.device, rows.shape[0]
        b = self._b()
        with self._on_current_stream(b, device) as stream:
            nu = b.decode_utf16(stream)
            p_units, p_off, _ = b.decode_utf16_device_result()
            out["units"] = _device_copy(p_units, nu, torch.uint16, device, stream)
            out["unit_off"] = _device_copy(p_off, nr + 1, torch.int64, device, stream)
        return out

    def vocab_size(self):
        return N.lib().jtk_encoding_vocab_size(self._h)

    def pair_count(self):
        return N.lib().jtk_encoding_pair_count(self._h)
