"""jtokkit_amd -- MI355X-native batch BPE encode path behind JTokkit's Encoding API."""
from .encoding import C4_PHRASES, GOPHER_STOP_WORDS, Batch, BatchResult, CompactBatchResult, EncodingError, FimParams, EncodingResult, HipEncoding, HostBuffer, NgramSet, PhraseSet, SeenSet, UnsupportedOperationError
from .registry import ENCODING_PARAMS, get_encoding, new_custom_encoding, new_encoding

__all__ = ["C4_PHRASES", "GOPHER_STOP_WORDS", "Batch", "BatchResult", "FimParams", "CompactBatchResult", "HostBuffer", "EncodingError", "EncodingResult", "HipEncoding", "NgramSet", "PhraseSet", "SeenSet",
           "UnsupportedOperationError", "ENCODING_PARAMS", "get_encoding", "new_custom_encoding", "new_encoding"]
