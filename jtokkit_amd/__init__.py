"""jtokkit_amd -- MI355X-native batch BPE encode path behind JTokkit's Encoding API."""
from .encoding import GOPHER_STOP_WORDS, Batch, BatchResult, CompactBatchResult, EncodingError, FimParams, EncodingResult, HipEncoding, HostBuffer, NgramSet, SeenSet, UnsupportedOperationError
from .registry import ENCODING_PARAMS, get_encoding, new_custom_encoding, new_encoding

__all__ = ["GOPHER_STOP_WORDS", "Batch", "BatchResult", "FimParams", "CompactBatchResult", "HostBuffer", "EncodingError", "EncodingResult", "HipEncoding", "NgramSet", "SeenSet", "UnsupportedOperationError",
           "ENCODING_PARAMS", "get_encoding", "new_custom_encoding", "new_encoding"]
