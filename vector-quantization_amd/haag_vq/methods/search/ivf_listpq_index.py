"""IvfListPqIndex — a k-means IVF shell around one product quantizer per list, on the MI355X.

Drop-in for the reference's ``IvfQuantizedIndex`` (methods/search/ivf_quantized_index.py) when its
factory returns a ``ProductQuantizer`` — the ``pq_ivf`` method of run_benchmarks: fit trains ``K``
coarse centroids, assigns every row to its nearest one and trains one PQ codebook per list on that
list's residuals x - centroid; search ranks the rows of the ``nprobe`` nearest lists by the
distance to decompress(codes) + centroid.  The constructor is the reference's, so a caller of the
reference changes only the class name (this package's ``IvfQuantizedIndex`` stays native for SQ
and LVQ and refuses PQ).

The factory is called once and must return this package's ``ProductQuantizer``; its ``M``, ``B``,
``niter`` and ``seed`` serve every list (the reference calls the factory per list; every instance
has the same settings).  The coarse quantizer and the lists are the ones of ``FaissIvfPqIndex``
(``_ivf.train_coarse``, bucket order); the codebooks are one (K, M, 2^B, D/M) tensor, each list's
trained by ``_kmeans.train_pq`` on its residuals.  No list is decoded: the search is
``mivq_ivf_listpq_search`` (include/mivq.h), an ADC whose lookup table belongs to a (query,
probed list) pair and is built on codebook + centroid, so the key is the ADC distance to the
reconstruction ``reconstruct`` returns — the reference's exact distance up to the fp32 reordering
``FlatQuantizedIndex`` documents for PQ.  faiss is absent, so neither centroids nor codebooks are
claimed to equal faiss'.

As in the reference (faiss refuses to train 2^B centroids on fewer points), a fit in which a
non-empty list holds fewer than 2^B rows raises; here all lists are checked right after the
assignment, before any training.  Empty lists are skipped.

``search_with_scores`` returns what the reference returns: ``(ids uint32, dists float32)`` of
shape (nq, k) always, ascending; for ``'ip'`` the negated inner products; slots the probed lists
cannot fill hold id 0xFFFFFFFF and FLT_MAX (L2) / -FLT_MAX (IP).  ``save`` / ``load`` write an
``.npz`` of plain arrays (the reference pickles its quantizer objects).
"""

from __future__ import annotations

import numpy as np
import torch

from ... import _arrays
from .._ivf import IvfListPq
from ._ivf_shell import IvfShellIndex


class IvfListPqIndex(IvfShellIndex):
    """IVF + one PQ codebook per list: ``K`` coarse cells, ``nprobe`` of them scanned per query."""

    def _adopt(self, q) -> None:
        from ..product_quantization import ProductQuantizer

        if not isinstance(q, ProductQuantizer):
            raise ValueError(f"IvfListPqIndex needs a factory of ProductQuantizer; it returned {type(q).__name__} "
                             f"(per-list SQ / LVQ: IvfQuantizedIndex)")
        self._M, self._B, self._niter, self._seed = int(q.M), int(q.B), int(q.niter), int(q.seed)

    def _engine(self, d: int, metric: int) -> IvfListPq:
        return IvfListPq(d, self._K, self._M, self._B, metric, niter=self._niter, seed=self._seed)

    def _extra_bytes(self) -> int:
        """The codebook bytes K * D * 2^B * 4, which the reference keeps in its quantizer objects
        and does not count.  They dominate at many lists: 1 GiB at K = 1024, D = 1024, B = 8."""
        return self._K * self._D * (1 << self._B) * 4

    def _own_arrays(self) -> dict:
        return dict(codebooks=_arrays.to_host(self._index.codebooks), M=np.array(self._M), B=np.array(self._B),
                    niter=np.array(self._niter), seed=np.array(self._seed))

    def _load_settings(self, z) -> None:
        self._M, self._B = int(z["M"]), int(z["B"])
        self._niter, self._seed = int(z["niter"]), int(z["seed"])

    def _load_arrays(self, z, index: IvfListPq) -> None:
        index.codebooks = _arrays.to_device(np.array(z["codebooks"]), torch.float32)
