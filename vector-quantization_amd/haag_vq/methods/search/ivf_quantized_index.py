"""IvfQuantizedIndex — a k-means IVF shell around per-list SQ / LVQ quantizers, on the MI355X.

Drop-in for the reference's ``IvfQuantizedIndex`` (methods/search/ivf_quantized_index.py): fit
trains ``K`` coarse centroids, assigns every row to its nearest one and fits one quantizer per
list on that list's residuals x - centroid; search decodes the rows of the ``nprobe`` nearest
lists, adds each list's centroid back and ranks by the exact distance to the reconstruction.

Native for factories that return this package's ``ScalarQuantizer`` (4 / 8 / 16 bits, f32) or
``LVQQuantizer`` (1..8 bits); the factory is called once, to learn the kind and the bits, and
any other quantizer raises ``NotImplementedError`` (per-list PQ is not built).  The coarse
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

from pathlib import Path
from typing import Callable, Literal, Optional, Tuple

import numpy as np
import torch

from ... import _arrays, _native
from .._ivf import IvfCodes, IvfLists
from ..base_quantizer import BaseQuantizer
from ..base_search_index import BaseSearchIndex

_METRIC = {"l2": _native.METRIC_L2, "ip": _native.METRIC_INNER_PRODUCT}
_MAX_K = 256
_FLT_MAX = np.finfo(np.float32).max
_DECODE_BYTES = 1 << 28  # reconstruction_mse: decoded rows per step


def _kind_of(q) -> Tuple[str, int]:
    from ..lvq_quantization import LVQQuantizer
    from ..scalar_quantization import ScalarQuantizer

    if isinstance(q, ScalarQuantizer):
        return "sq", int(q.num_bits)
    if isinstance(q, LVQQuantizer):
        return "lvq", int(q.num_bits)
    raise NotImplementedError(
        f"IvfQuantizedIndex is native for ScalarQuantizer (4 / 8 / 16 bits) and LVQQuantizer (1..8 bits); "
        f"the factory returned {type(q).__name__}")


class IvfQuantizedIndex(BaseSearchIndex):
    """IVF + per-list quantization: ``K`` coarse cells, ``nprobe`` of them scanned per query."""

    def __init__(self, quantizer_factory: Callable[[], BaseQuantizer], K: int = 4096, nprobe: int = 200) -> None:
        self._quantizer_factory = quantizer_factory
        self._kind, self._bits = _kind_of(quantizer_factory())
        self._K = int(K)
        self._nprobe = int(nprobe)
        if self._K <= 0 or self._nprobe <= 0:
            raise ValueError(f"K and nprobe must be positive, got {K}, {nprobe}")
        self._index: Optional[IvfCodes] = None
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
        index = IvfCodes(d, self._K, self._kind, self._bits, _METRIC[metric])
        if centroids is None:
            index.train(Xd)
        else:
            index.coarse = _arrays.to_device(centroids, torch.float32)
            if tuple(index.coarse.shape) != (self._K, d):
                raise ValueError(f"centroids must be ({self._K}, {d}), got {tuple(index.coarse.shape)}")
        index.fit_lists(Xd)
        self._index, self._metric, self._N, self._D = index, metric, n, d

    def _require_fit(self) -> IvfCodes:
        if self._index is None or self._index.lists is None:
            raise RuntimeError("IvfQuantizedIndex must be fit() before use.")
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
        """The reference's formula (centroid bytes + code bytes) plus the per-list parameters
        ((K, d) f32: lo and den for SQ, mu for LVQ), which the reference keeps in its quantizer
        objects and does not count."""
        if self._index is None or self._index.lists is None:
            return 0
        codes = self._index.lists.codes
        params = sum(t.numel() * t.element_size() for t in self._index.params)
        return self._K * self._D * 4 + codes.numel() * codes.element_size() + params

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
            raise RuntimeError("IvfQuantizedIndex.save() called before fit()")
        path = Path(path)
        path.parent.mkdir(parents=True, exist_ok=True)
        ix, L = self._index, self._index.lists
        arrays = {f"param{i}": _arrays.to_host(t) for i, t in enumerate(ix.params)}
        with open(path, "wb") as f:
            np.savez(f, coarse=_arrays.to_host(ix.coarse), offsets=_arrays.to_host(L.offsets),
                     codes=_arrays.to_host(L.codes), ids=_arrays.to_host(L.ids), kind=np.array(self._kind),
                     bits=np.array(self._bits), K=np.array(self._K), nprobe=np.array(self._nprobe),
                     metric=np.array(self._metric), N=np.array(self._N), D=np.array(self._D), **arrays)

    def load(self, path: str | Path) -> None:
        with np.load(Path(path), allow_pickle=False) as z:
            self._kind, self._bits = str(z["kind"]), int(z["bits"])
            self._K, self._nprobe = int(z["K"]), int(z["nprobe"])
            self._metric = str(z["metric"])
            self._N, self._D = int(z["N"]), int(z["D"])
            index = IvfCodes(self._D, self._K, self._kind, self._bits, _METRIC[self._metric])
            index.coarse = _arrays.to_device(np.array(z["coarse"]), torch.float32)
            index.params = tuple(_arrays.to_device(np.array(z[f"param{i}"]), torch.float32)
                                 for i in range(2 if self._kind == "sq" else 1))
            codes = np.array(z["codes"])
            index.lists = IvfLists(offsets=_arrays.to_device(np.array(z["offsets"]), torch.int64),
                                   codes=_arrays.to_device(codes, torch.int16 if codes.dtype.itemsize == 2 else torch.uint8),
                                   ids=_arrays.to_device(np.array(z["ids"]), torch.int32), tau=None)
            index.ntotal = self._N
            index._index_rows()
        self._index = index
