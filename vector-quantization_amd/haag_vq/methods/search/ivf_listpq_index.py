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

from pathlib import Path
from typing import Callable, Literal, Optional, Tuple

import numpy as np
import torch

from ... import _arrays, _native
from .._ivf import IvfListPq, IvfLists
from ..base_quantizer import BaseQuantizer
from ..base_search_index import BaseSearchIndex

_METRIC = {"l2": _native.METRIC_L2, "ip": _native.METRIC_INNER_PRODUCT}
_MAX_K = 256
_FLT_MAX = np.finfo(np.float32).max
_DECODE_BYTES = 1 << 28  # reconstruction_mse: decoded rows per step


class IvfListPqIndex(BaseSearchIndex):
    """IVF + one PQ codebook per list: ``K`` coarse cells, ``nprobe`` of them scanned per query."""

    def __init__(self, quantizer_factory: Callable[[], BaseQuantizer], K: int = 4096, nprobe: int = 200) -> None:
        from ..product_quantization import ProductQuantizer

        self._quantizer_factory = quantizer_factory
        q = quantizer_factory()
        if not isinstance(q, ProductQuantizer):
            raise ValueError(f"IvfListPqIndex needs a factory of ProductQuantizer; it returned {type(q).__name__} "
                             f"(per-list SQ / LVQ: IvfQuantizedIndex)")
        self._M, self._B, self._niter, self._seed = int(q.M), int(q.B), int(q.niter), int(q.seed)
        self._K = int(K)
        self._nprobe = int(nprobe)
        if self._K <= 0 or self._nprobe <= 0:
            raise ValueError(f"K and nprobe must be positive, got {K}, {nprobe}")
        self._index: Optional[IvfListPq] = None
        self._metric: Literal["l2", "ip"] = "l2"
        self._N: int = 0
        self._D: int = 0

    @property
    def nprobe(self) -> int:
        return self._nprobe

    @nprobe.setter
    def nprobe(self, v: int) -> None:
        self._nprobe = int(v)

    @property
    def ntotal(self) -> int:
        return self._N

    def fit(self, X, metric: Literal["l2", "ip"] = "l2", centroids=None) -> None:
        """``centroids`` (K, D): use these coarse centroids instead of training them."""
        if metric not in _METRIC:
            raise ValueError(f"metric must be 'l2' or 'ip', got {metric!r}")
        Xd = _arrays.to_device(X, torch.float32)
        n, d = int(Xd.shape[0]), int(Xd.shape[1])
        index = IvfListPq(d, self._K, self._M, self._B, _METRIC[metric], niter=self._niter, seed=self._seed)
        if centroids is None:
            index.train(Xd)
        else:
            index.coarse = _arrays.to_device(centroids, torch.float32)
            if tuple(index.coarse.shape) != (self._K, d):
                raise ValueError(f"centroids must be ({self._K}, {d}), got {tuple(index.coarse.shape)}")
        index.fit_lists(Xd)
        self._index, self._metric, self._N, self._D = index, metric, n, d

    def _require_fit(self) -> IvfListPq:
        if self._index is None or self._index.lists is None:
            raise RuntimeError("IvfListPqIndex must be fit() before use.")
        return self._index

    def _check_limits(self, k: int) -> None:
        if int(k) > _MAX_K:
            raise ValueError(f"k={k}: the search supports at most k = {_MAX_K}")
        nprobe = max(1, min(self._nprobe, self._K))
        if nprobe > 256:
            raise ValueError(f"nprobe={nprobe}: the probe selection supports at most 256 lists")

    def search(self, Q, k: int) -> np.ndarray:
        ids, _ = self.search_with_scores(Q, k)
        return ids

    def search_device(self, Q, k: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """Device-resident search: the raw keys (dists f32 (nq, k): squared L2, or negated inner
        products; +inf where the probed lists hold fewer than k rows) and ids int32 (nq, k)
        holding uint32 ids."""
        index = self._require_fit()
        self._check_limits(k)
        return index.search(_arrays.to_device(Q, torch.float32), int(k), self._nprobe)

    def search_with_scores(self, Q, k: int) -> Tuple[np.ndarray, np.ndarray]:
        self._require_fit()
        self._check_limits(k)
        nq = int(Q.shape[0])
        if int(k) <= 0:
            return np.empty((nq, 0), dtype=np.uint32), np.empty((nq, 0), dtype=np.float32)
        d, i = self.search_device(Q, k)
        ids = _arrays.to_host(i).view(np.uint32)
        dists = _arrays.to_host(d)
        # the reference's sentinels for the slots it leaves unfilled
        dists[ids == _native.NO_ID] = -_FLT_MAX if self._metric == "ip" else _FLT_MAX
        return ids, dists

    def memory_footprint(self) -> int:
        """The reference's formula (centroid bytes + code bytes) plus the codebook bytes
        K * D * 2^B * 4, which the reference keeps in its quantizer objects and does not count.
        The codebooks dominate at many lists: 1 GiB at K = 1024, D = 1024, B = 8."""
        if self._index is None or self._index.lists is None:
            return 0
        codes = self._index.lists.codes
        return self._K * self._D * 4 + codes.numel() * codes.element_size() + self._K * self._D * (1 << self._B) * 4

    def reconstruction_mse(self, X, sample_ids: Optional[np.ndarray] = None) -> Optional[float]:
        if self._index is None or self._index.lists is None:
            return None
        if sample_ids is None:
            sample_ids = np.arange(self._N)
        sample_ids = np.asarray(sample_ids, dtype=np.int64)
        sample_ids = sample_ids[(sample_ids >= 0) & (sample_ids < self._N)]
        if sample_ids.size == 0:
            return None
        total = 0.0
        step = max(1, _DECODE_BYTES // (4 * self._D))
        for s in range(0, sample_ids.size, step):
            rows = sample_ids[s:s + step]
            xh = _arrays.to_host(self._index.reconstruct(torch.from_numpy(rows)))
            x = np.asarray(_arrays.to_host(X[rows]) if _arrays.is_tensor(X) else X[rows], dtype=np.float32)
            total += float(np.mean((x - xh) ** 2, axis=1).astype(np.float64).sum())
        return total / sample_ids.size

    def save(self, path: str | Path) -> None:
        if self._index is None or self._index.lists is None:
            raise RuntimeError("IvfListPqIndex.save() called before fit()")
        path = Path(path)
        path.parent.mkdir(parents=True, exist_ok=True)
        ix, L = self._index, self._index.lists
        with open(path, "wb") as f:
            np.savez(f, coarse=_arrays.to_host(ix.coarse), codebooks=_arrays.to_host(ix.codebooks),
                     offsets=_arrays.to_host(L.offsets), codes=_arrays.to_host(L.codes), ids=_arrays.to_host(L.ids),
                     M=np.array(self._M), B=np.array(self._B), niter=np.array(self._niter), seed=np.array(self._seed),
                     K=np.array(self._K), nprobe=np.array(self._nprobe), metric=np.array(self._metric),
                     N=np.array(self._N), D=np.array(self._D))

    def load(self, path: str | Path) -> None:
        with np.load(Path(path), allow_pickle=False) as z:
            self._M, self._B = int(z["M"]), int(z["B"])
            self._niter, self._seed = int(z["niter"]), int(z["seed"])
            self._K, self._nprobe = int(z["K"]), int(z["nprobe"])
            self._metric = str(z["metric"])
            self._N, self._D = int(z["N"]), int(z["D"])
            index = IvfListPq(self._D, self._K, self._M, self._B, _METRIC[self._metric], niter=self._niter,
                              seed=self._seed)
            index.coarse = _arrays.to_device(np.array(z["coarse"]), torch.float32)
            index.codebooks = _arrays.to_device(np.array(z["codebooks"]), torch.float32)
            index.lists = IvfLists(offsets=_arrays.to_device(np.array(z["offsets"]), torch.int64),
                                   codes=_arrays.to_device(np.array(z["codes"]), torch.uint8),
                                   ids=_arrays.to_device(np.array(z["ids"]), torch.int32), tau=None)
            index.ntotal = self._N
            index._index_rows()
        self._index = index
