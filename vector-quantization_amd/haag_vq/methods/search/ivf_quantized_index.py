"""IvfQuantizedIndex — a k-means IVF shell around per-list SQ / LVQ quantizers, on the MI355X.

Drop-in for the reference's ``IvfQuantizedIndex`` (methods/search/ivf_quantized_index.py): fit
trains ``K`` coarse centroids, assigns every row to its nearest one and fits one quantizer per
list on that list's residuals x - centroid; search decodes the rows of the ``nprobe`` nearest
lists, adds each list's centroid back and ranks by the exact distance to the reconstruction.

Native for factories that return this package's ``ScalarQuantizer`` (4 / 8 / 16 bits, f32) or
``LVQQuantizer`` (1..8 bits); the factory is called once, to learn the kind and the bits, and
any other quantizer raises ``NotImplementedError`` (a ``ProductQuantizer`` per list is
``IvfListPqIndex``, ivf_listpq_index.py).  The coarse
quantizer and the lists are the ones of ``FaissIvfPqIndex`` (``_ivf.train_coarse``, bucket
order), the per-list parameters are (K, d) tensors, and no list is decoded to memory: the
search is ``mivq_ivf_sq_search`` / ``mivq_ivf_lvq_search`` (include/mivq.h), bit-identical to
decode + add + ``mivq_flat_search`` over the probed rows.  faiss is absent, so the centroids
are not claimed to equal faiss'.

``search_with_scores`` returns what the reference returns: ``(ids uint32, dists float32)`` of
shape (nq, k) always, ascending; for ``'ip'`` the negated inner products; slots the probed lists
cannot fill hold id 0xFFFFFFFF and FLT_MAX (L2) / -FLT_MAX (IP).  ``save`` / ``load`` write an
``.npz`` of plain arrays (the reference pickles its quantizer objects).
"""

from __future__ import annotations

from typing import Tuple

import numpy as np
import torch

from ... import _arrays
from .._ivf import IvfCodes
from ._ivf_shell import IvfShellIndex


def _kind_of(q) -> Tuple[str, int]:
    if getattr(q, "code_kind", None) is not None:
        return q.code_kind, int(q.num_bits)
    raise NotImplementedError(
        f"IvfQuantizedIndex is native for ScalarQuantizer (4 / 8 / 16 bits) and LVQQuantizer (1..8 bits); "
        f"the factory returned {type(q).__name__}")


class IvfQuantizedIndex(IvfShellIndex):
    """IVF + per-list quantization: ``K`` coarse cells, ``nprobe`` of them scanned per query."""

    def _adopt(self, q) -> None:
        self._kind, self._bits = _kind_of(q)

    def _engine(self, d: int, metric: int) -> IvfCodes:
        return IvfCodes(d, self._K, self._kind, self._bits, metric)

    def _extra_bytes(self) -> int:
        """The per-list parameters ((K, d) f32: lo and den for SQ, mu for LVQ), which the reference
        keeps in its quantizer objects and does not count."""
        return sum(t.numel() * t.element_size() for t in self._index.params)

    def _own_arrays(self) -> dict:
        return dict(kind=np.array(self._kind), bits=np.array(self._bits),
                    **{f"param{i}": _arrays.to_host(t) for i, t in enumerate(self._index.params)})

    def _load_settings(self, z) -> None:
        self._kind, self._bits = str(z["kind"]), int(z["bits"])

    def _load_arrays(self, z, index: IvfCodes) -> None:
        index.params = tuple(_arrays.to_device(np.array(z[f"param{i}"]), torch.float32)
                             for i in range(2 if self._kind == "sq" else 1))
