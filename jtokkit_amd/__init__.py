"""jtokkit_amd -- MI355X-native batch BPE encode path behind JTokkit's Encoding API."""
from .encoding import Batch, BatchResult, CompactBatchResult, EncodingError, FimParams, EncodingResult, HipEncoding, HostBuffer, NgramSet, UnsupportedOperationError
from .registry import ENCODING_PARAMS, get_encoding, new_custom_encoding, new_encoding

__all__ = ["Batch", "BatchResult", "FimParams", "CompactBatchResult", "HostBuffer", "EncodingError", "EncodingResult", "HipEncoding", "NgramSet", "UnsupportedOperationError",
           "ENCODING_PARAMS", "get_encoding", "new_custom_encoding", "new_encoding"]
