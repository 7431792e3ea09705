"""RefinedIndex — two-stage search: over-fetch from a cheap index, re-rank on a finer copy of the rows.

The quantisation error of a single-stage index caps its ranking, whatever is spent on probes.
``RefinedIndex`` asks its base index for ``r = k * refine_factor`` candidates per query and ranks
them again by the exact distance to a finer store of the same rows (faiss' ``IndexRefine`` /
``IndexRefineFlat``, SVS' LVQ re-ranking):

* ``refine=None``: the f32 rows themselves, kept on the device;
* ``refine=ScalarQuantizer(4 | 8 | 16)``: the quantizer's codes, fitted on the f32 cast of X
  (an f64-fitted SQ has no code-domain chain, see ``search_codes``);
* ``refine=LVQQuantizer(1..8)``: the quantizer's codes.

The second stage is ``mivq_rerank_*`` (include/mivq.h): a candidate's distance is the chain of the
matching flat search, bit for bit, so the result is ``mivq_*_flat_search`` over the store restricted
to the candidates; no decoded row and no (nq, r, d) block is formed.  The base searches keep at
most 256 results, so ``k * refine_factor`` may not exceed 256.

``search_with_scores`` returns ``(ids uint32, dists float32)`` of shape (nq, k) always: squared L2
ascending, or inner products descending; slots the candidates cannot fill hold id 0xFFFFFFFF and
FLT_MAX (L2) / -FLT_MAX (IP), as in ``IvfQuantizedIndex``.  ``save`` writes an ``.npz`` of plain
arrays and the base index next to it, at ``path + ".base"``.
"""

from __future__ import annotations

from pathlib import Path
from typing import Literal, Optional, Tuple

import numpy as np
import torch

from ... import _arrays, _native
from ..base_quantizer import BaseQuantizer
from ..base_search_index import BaseSearchIndex
from ._common import MAX_CANDIDATES  # noqa: F401  (what a base search returns at most; importable from here)
from ._common import FLT_MAX, METRIC, candidate_count, check_metric, empty_results, results_to_host, save_npz


def _kind_of(refine: Optional[BaseQuantizer]) -> Tuple[str, int]:
    if refine is None:
        return "f32", 0
    if getattr(refine, "code_kind", None) is not None:
        return refine.code_kind, int(refine.num_bits)
    raise ValueError(f"RefinedIndex re-ranks on f32 rows (refine=None), ScalarQuantizer (4 / 8 / 16 bits) or "
                     f"LVQQuantizer (1..8 bits) codes, got {type(refine).__name__}")


def _base_path(path: Path) -> Path:
    return path.with_name(path.name + ".base")


class RefinedIndex(BaseSearchIndex):
    """``base`` proposes ``k * refine_factor`` candidates, the store of ``refine`` ranks them."""

    def __init__(self, base: BaseSearchIndex, refine: Optional[BaseQuantizer] = None, refine_factor: int = 10) -> None:
        self._kind, self._bits = _kind_of(refine)
        if int(refine_factor) < 1:
            raise ValueError(f"refine_factor must be at least 1, got {refine_factor}")
        self._base = base
        self._refine = refine
        self._factor = int(refine_factor)
        self._store: Optional[torch.Tensor] = None
        self._params: Tuple[torch.Tensor, ...] = ()
        self._metric: Literal["l2", "ip"] = "l2"
        self._N = 0
        self._D = 0

    @property
    def base(self) -> BaseSearchIndex:
        return self._base

    @property
    def refine_factor(self) -> int:
        return self._factor

    @property
    def ntotal(self) -> int:
        return self._N

    def fit(self, X, metric: Literal["l2", "ip"] = "l2") -> None:
        check_metric(metric)
        self._base.fit(X, metric)
        Xd = _arrays.to_device(X, torch.float32)
        if self._kind == "f32":
            self._store, self._params = Xd, ()
        else:
            self._refine.fit(Xd)
            self._store = self._refine.compress(Xd)
            self._params = self._refine.code_params()
        self._metric = metric
        self._N, self._D = int(Xd.shape[0]), int(Xd.shape[1])

    def candidate_count(self, k: int) -> int:
        """r, the candidates asked of the base index per query: min(k * refine_factor, N)."""
        return candidate_count(k, self._factor, self._N)

    def search(self, Q, k: int) -> np.ndarray:
        ids, _ = self.search_with_scores(Q, k)
        return ids

    def search_with_scores(self, Q, k: int) -> Tuple[np.ndarray, np.ndarray]:
        r = self.candidate_count(k)
        if self._store is None:
            raise RuntimeError("RefinedIndex must be fit (or loaded) before a search")
        nq = int(Q.shape[0])
        if int(k) <= 0 or nq == 0:
            return empty_results(nq, k)
        sentinel = -FLT_MAX if self._metric == "ip" else FLT_MAX
        cand = self._base.search(Q, r) if r > 0 else np.empty((nq, 0), dtype=np.uint32)
        if _arrays.is_tensor(cand):
            cand = _arrays.to_host(cand)
        cand = np.ascontiguousarray(cand).astype(np.uint32, copy=False).view(np.int32)
        if cand.shape[1] == 0:  # an empty database
            return np.full((nq, int(k)), _native.NO_ID, dtype=np.uint32), np.full((nq, int(k)), sentinel, dtype=np.float32)
        d, i = _native.rerank(self._kind, _arrays.to_device(Q, torch.float32), _arrays.to_device(cand, torch.int32),
                              self._store, self._params, self._bits, int(k), METRIC[self._metric])
        return results_to_host(d, i, negate=self._metric == "ip", sentinel=sentinel)

    def _store_bytes(self) -> int:
        if self._store is None:
            return 0
        return int(self._store.numel() * self._store.element_size()
                   + sum(t.numel() * t.element_size() for t in self._params))

    def memory_footprint(self) -> int:
        """The base's footprint plus the store's bytes, its per-dimension parameters included."""
        return int(self._base.memory_footprint()) + self._store_bytes()

    def reconstruction_mse(self, X, sample_ids: Optional[np.ndarray] = None) -> Optional[float]:
        return self._base.reconstruction_mse(X, sample_ids)

    # --------------------------------------------------------------- persistence
    def save(self, path: str | Path) -> None:
        if self._store is None:
            raise RuntimeError("RefinedIndex.save() called before fit()")
        path = Path(path)
        save_npz(path, store=_arrays.to_host(self._store), kind=np.array(self._kind), bits=np.array(self._bits),
                 metric=np.array(self._metric), refine_factor=np.array(self._factor), N=np.array(self._N),
                 D=np.array(self._D), **{f"param{i}": _arrays.to_host(t) for i, t in enumerate(self._params)})
        self._base.save(_base_path(path))

    def load(self, path: str | Path) -> None:
        path = Path(path)
        with np.load(path, allow_pickle=False) as z:
            kind, bits = str(z["kind"]), int(z["bits"])
            if (kind, bits) != (self._kind, self._bits):
                raise ValueError(f"load(): {path} holds a {kind} store of {bits} bits, this index was built for "
                                 f"{self._kind} of {self._bits} bits")
            nparams = {"f32": 0, "sq": 2, "lvq": 1}[kind]
            store = np.array(z["store"])
            params = [np.array(z[f"param{i}"], dtype=np.float32) for i in range(nparams)]
            metric, factor, N, D = str(z["metric"]), int(z["refine_factor"]), int(z["N"]), int(z["D"])
        if metric not in METRIC or factor < 1 or store.ndim != 2 or store.shape[0] != N or any(p.shape != (D,) for p in params):
            raise ValueError(f"load(): {path} is not a consistent RefinedIndex file")
        self._base.load(_base_path(path))
        dt = torch.float32 if kind == "f32" else torch.int16 if store.dtype.itemsize == 2 else torch.uint8
        self._store = _arrays.to_device(store.view(np.int16) if dt == torch.int16 else store, dt)
        self._params = tuple(_arrays.to_device(p, torch.float32) for p in params)
        self._metric, self._factor, self._N, self._D = metric, factor, N, D
