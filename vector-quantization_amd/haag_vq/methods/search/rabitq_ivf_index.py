"""RaBitQIVFIndex — IVF coarse quantisation + RaBitQ codes with estimator search, on the MI355X.

Drop-in for the reference's ``RaBitQIVFIndex`` (methods/search/rabitq_ivf_index.py), which wraps
faiss ``IVF{nlist},RaBitQ`` with ``.qb = qb`` and ``.nprobe = nprobe``: train fits ``nlist``
coarse centroids, add stores for every row the 1-bit RaBitQ code of x - (its list's centroid)
with the two per-vector factors, and search ranks the rows of the ``nprobe`` nearest lists by
the RaBitQ estimator, the query residual against each probed list's centroid quantised to
``qb`` bits.  Here the coarse quantizer and the lists are the ones of ``FaissIvfPqIndex``
(``_ivf.train_coarse``, bucket order), the codes are ``mivq_ivf_rabitq_encode`` rows and the
search is ``mivq_ivf_rabitq_search`` (int8 MFMA over the sign bits of the probed lists, estimator
epilogue, top-k selected inside the scan).  faiss is absent, so centroids and results are not
claimed to equal faiss'; the arithmetic is the one of oracle/mivq_oracle.c.

Search returns ``(ids uint32, dists float32)``: squared-L2 estimates ascending, or inner-product
estimates descending (metric ``'ip'``); slots the probed lists cannot fill hold id 0xFFFFFFFF.
``save`` / ``load`` write an ``.npz`` of plain arrays (faiss' index file format is not reproduced).
"""

from __future__ import annotations

from pathlib import Path
from typing import Literal, Optional, Tuple

import numpy as np
import torch

from ... import _arrays, _native
from .._ivf import IvfLists, IvfRaBitQ
from ..base_search_index import BaseSearchIndex
from ._common import MAX_K, METRIC, check_metric, empty_results, results_to_host, save_npz
from ._ivf_shell import NprobeMixin


class RaBitQIVFIndex(NprobeMixin, BaseSearchIndex):
    """IVF + RaBitQ: ``nlist`` coarse cells, ``nprobe`` of them scanned per query, ``qb`` query bits."""

    def __init__(self, nlist: int = 256, nprobe: int = 64, qb: int = 4) -> None:
        self._nlist = int(nlist)
        self._nprobe = int(nprobe)
        self._qb = int(qb)
        if not 0 <= self._qb <= 8:
            raise ValueError(f"qb must be in [0, 8], got {qb}")
        if self._nlist <= 0 or self._nprobe <= 0:
            raise ValueError(f"nlist and nprobe must be positive, got {nlist}, {nprobe}")
        self._index: Optional[IvfRaBitQ] = None
        self._D: int = 0
        self._metric: Literal["l2", "ip"] = "l2"

    @property
    def ntotal(self) -> int:
        return 0 if self._index is None else int(self._index.ntotal)

    @property
    def code_size(self) -> int:
        return _native.rabitq_code_size(self._D)

    def fit(self, X, metric: Literal["l2", "ip"] = "l2") -> None:
        mt = check_metric(metric)
        Xd = _arrays.to_device(X, torch.float32)
        self._D = int(Xd.shape[1])
        self._metric = metric
        index = IvfRaBitQ(self._D, self._nlist, mt)
        index.train(Xd)
        index.add(Xd)
        self._index = index

    def add(self, X) -> None:
        """Append rows to a fitted index (ids continue from ntotal)."""
        self._require_fit().add(_arrays.to_device(X, torch.float32))

    def _require_fit(self) -> IvfRaBitQ:
        if self._index is None or self._index.lists is None:
            raise RuntimeError("RaBitQIVFIndex must be fit() before use.")
        return self._index

    def search(self, Q, k: int) -> np.ndarray:
        ids, _ = self.search_with_scores(Q, k)
        return ids

    def search_device(self, Q, k: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """Device-resident search: (dists f32 (nq, k), ids int32 (nq, k) holding uint32 ids)."""
        index = self._require_fit()
        if k > MAX_K:
            raise ValueError(f"k={k}: the search supports at most k = {MAX_K}")
        Qd = _arrays.to_device(Q, torch.float32)
        d, i = index.search(Qd, k, self._nprobe, self._qb)
        return (-d if self._metric == "ip" else d), i

    def search_with_scores(self, Q, k: int) -> Tuple[np.ndarray, np.ndarray]:
        self._require_fit()
        if int(k) > MAX_K:
            raise ValueError(f"k={k}: the search supports at most k = {MAX_K}")
        nq = int(Q.shape[0])
        k = min(int(k), self.ntotal)
        if k <= 0:
            return empty_results(nq, 0)
        return results_to_host(*self.search_device(Q, k))

    def memory_footprint(self) -> int:
        if self._index is None:
            return 0
        # the reference's formula: codes, 8 bytes of id per row (faiss' int64), the f32 centroids
        return self.ntotal * self.code_size + self.ntotal * 8 + self._nlist * self._D * 4

    def reconstruction_mse(self, X, sample_ids: Optional[np.ndarray] = None) -> Optional[float]:
        return None  # as the reference: no batched reconstruct for this layout

    def save(self, path: str | Path) -> None:
        if self._index is None or self._index.lists is None:
            raise RuntimeError("RaBitQIVFIndex.save() called before fit()")
        save_npz(path, coarse=_arrays.to_host(self._index.coarse), **self._index.lists.to_arrays(),
                 nlist=np.array(self._nlist), nprobe=np.array(self._nprobe), qb=np.array(self._qb),
                 metric=np.array(self._metric), D=np.array(self._D))

    def load(self, path: str | Path) -> None:
        with np.load(Path(path), allow_pickle=False) as z:
            self._nlist = int(z["nlist"])
            self._nprobe = int(z["nprobe"])
            self._qb = int(z["qb"])
            self._metric = str(z["metric"])
            self._D = int(z["D"])
            index = IvfRaBitQ(self._D, self._nlist, METRIC[self._metric])
            index.coarse = _arrays.to_device(np.array(z["coarse"]), torch.float32)
            index.lists = IvfLists.from_arrays(z, _arrays.device())
            index.ntotal = int(index.lists.ids.shape[0])
        self._index = index
