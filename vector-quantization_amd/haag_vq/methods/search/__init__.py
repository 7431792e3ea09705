from .faiss_ivfpq_index import FaissIvfPqIndex
from .flat_quantized_index import (ExtendedRaBitQFlatIndex, FlatQuantizedIndex, FlatADCIndex, RankAwareFlatIndex,
                                   search_codes)
from .ivf_listpq_index import IvfListPqIndex
from .ivf_quantized_index import IvfQuantizedIndex
from .lvq2_index import LVQ2Index
from .rabitq_index import RaBitQIndex
from .rabitq_ivf_index import RaBitQIVFIndex
from .refined_index import RefinedIndex

__all__ = ["FaissIvfPqIndex", "FlatQuantizedIndex", "FlatADCIndex", "RankAwareFlatIndex", "ExtendedRaBitQFlatIndex",
           "IvfQuantizedIndex", "IvfListPqIndex", "LVQ2Index", "RaBitQIndex", "RaBitQIVFIndex", "RefinedIndex", "search_codes"]
