"""Quantizers of the MI355X build (module paths mirror /root/reference/src/haag_vq/methods)."""

from .base_quantizer import BaseQuantizer
from .base_search_index import BaseSearchIndex

__all__ = ["BaseQuantizer", "BaseSearchIndex", "IvfQuantizedIndex", "RankAwareQuantizer"]


def __getattr__(name):
    # resolved on first use: the search indexes import torch and the native library
    if name == "IvfQuantizedIndex":
        from .search.ivf_quantized_index import IvfQuantizedIndex

        return IvfQuantizedIndex
    if name == "RankAwareQuantizer":
        from .rank_aware_quantization import RankAwareQuantizer

        return RankAwareQuantizer
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
