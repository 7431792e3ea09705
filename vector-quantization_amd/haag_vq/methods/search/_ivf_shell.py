"""The shell of the per-list IVF indexes: everything ``IvfQuantizedIndex`` and ``IvfListPqIndex``
do around their engines (_ivf.IvfCodes / _ivf.IvfListPq).

A subclass says what the factory's quantizer must be and what to keep of it (``_adopt``), how to
construct its engine (``_engine``), which entries of its own an index file holds (``_own_arrays``,
read back by ``_load_settings`` / ``_load_arrays``) and what its engine keeps besides centroids and
codes (``_extra_bytes``).
"""

from __future__ import annotations

from pathlib import Path
from typing import Callable, Literal, Optional, Tuple

import numpy as np
import torch

from ... import _arrays
from .._ivf import IvfLists, _IvfRowEngine
from ..base_quantizer import BaseQuantizer
from ..base_search_index import BaseSearchIndex
from ._common import FLT_MAX, MAX_K, METRIC, check_metric, empty_results, results_to_host, sampled_mse, save_npz


class NprobeMixin:
    """``nprobe``, settable between searches."""

    _nprobe: int

    @property
    def nprobe(self) -> int:
        return self._nprobe

    @nprobe.setter
    def nprobe(self, v: int) -> None:
        self._nprobe = int(v)


class IvfShellIndex(NprobeMixin, BaseSearchIndex):
    """``K`` coarse cells with one quantizer each, ``nprobe`` of them scanned per query."""

    def __init__(self, quantizer_factory: Callable[[], BaseQuantizer], K: int = 4096, nprobe: int = 200) -> None:
        self._quantizer_factory = quantizer_factory
        self._adopt(quantizer_factory())
        self._K = int(K)
        self._nprobe = int(nprobe)
        if self._K <= 0 or self._nprobe <= 0:
            raise ValueError(f"K and nprobe must be positive, got {K}, {nprobe}")
        self._index: Optional[_IvfRowEngine] = None
        self._metric: Literal["l2", "ip"] = "l2"
        self._N: int = 0
        self._D: int = 0

    # ------------------------------------------------------------- what a subclass supplies
    def _adopt(self, q: BaseQuantizer) -> None:
        """Refuse a quantizer this index is not native for; keep its settings."""
        raise NotImplementedError

    def _engine(self, d: int, metric: int) -> _IvfRowEngine:
        raise NotImplementedError

    def _own_arrays(self) -> dict:
        """What ``save`` writes besides the coarse centroids, the lists and K / nprobe / metric / N / D."""
        raise NotImplementedError

    def _load_settings(self, z) -> None:
        """Restore from an open index file the settings ``_engine`` needs."""
        raise NotImplementedError

    def _load_arrays(self, z, index: _IvfRowEngine) -> None:
        """Put the engine's own arrays of an open index file in place."""
        raise NotImplementedError

    def _extra_bytes(self) -> int:
        raise NotImplementedError

    # ------------------------------------------------------------- the shell
    @property
    def ntotal(self) -> int:
        return self._N

    def _fitted(self) -> bool:
        return self._index is not None and self._index.lists is not None

    def fit(self, X, metric: Literal["l2", "ip"] = "l2", centroids=None) -> None:
        """``centroids`` (K, D): use these coarse centroids instead of training them."""
        mt = check_metric(metric)
        Xd = _arrays.to_device(X, torch.float32)
        n, d = int(Xd.shape[0]), int(Xd.shape[1])
        index = self._engine(d, mt)
        if centroids is None:
            index.train(Xd)
        else:
            index.coarse = _arrays.to_device(centroids, torch.float32)
            if tuple(index.coarse.shape) != (self._K, d):
                raise ValueError(f"centroids must be ({self._K}, {d}), got {tuple(index.coarse.shape)}")
        index.fit_lists(Xd)
        self._index, self._metric, self._N, self._D = index, metric, n, d

    def _require_fit(self) -> _IvfRowEngine:
        if not self._fitted():
            raise RuntimeError(f"{type(self).__name__} must be fit() before use.")
        return self._index

    def _check_limits(self, k: int) -> None:
        if int(k) > MAX_K:
            raise ValueError(f"k={k}: the search supports at most k = {MAX_K}")
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
        if int(k) <= 0:
            return empty_results(int(Q.shape[0]), 0)
        # the reference's sentinels for the slots it leaves unfilled
        return results_to_host(*self.search_device(Q, k), sentinel=-FLT_MAX if self._metric == "ip" else FLT_MAX)

    def memory_footprint(self) -> int:
        """The reference's formula (centroid bytes + code bytes) plus ``_extra_bytes``."""
        if not self._fitted():
            return 0
        codes = self._index.lists.codes
        return self._K * self._D * 4 + codes.numel() * codes.element_size() + self._extra_bytes()

    def reconstruction_mse(self, X, sample_ids: Optional[np.ndarray] = None) -> Optional[float]:
        if not self._fitted():
            return None
        return sampled_mse(self._index.reconstruct, X, self._N, self._D, sample_ids)

    def save(self, path: str | Path) -> None:
        if not self._fitted():
            raise RuntimeError(f"{type(self).__name__}.save() called before fit()")
        save_npz(path, coarse=_arrays.to_host(self._index.coarse), **self._index.lists.to_arrays(),
                 K=np.array(self._K), nprobe=np.array(self._nprobe), metric=np.array(self._metric),
                 N=np.array(self._N), D=np.array(self._D), **self._own_arrays())

    def load(self, path: str | Path) -> None:
        with np.load(Path(path), allow_pickle=False) as z:
            self._load_settings(z)
            self._K, self._nprobe = int(z["K"]), int(z["nprobe"])
            self._metric = str(z["metric"])
            self._N, self._D = int(z["N"]), int(z["D"])
            index = self._engine(self._D, METRIC[self._metric])
            index.coarse = _arrays.to_device(np.array(z["coarse"]), torch.float32)
            self._load_arrays(z, index)
            index.lists = IvfLists.from_arrays(z, _arrays.device())
            index.ntotal = self._N
            index._index_rows()
        self._index = index
