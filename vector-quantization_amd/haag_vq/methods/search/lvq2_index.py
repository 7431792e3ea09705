"""LVQ2Index — two-level LVQ searched in two stages, both on the device.

``fit`` encodes the rows once with ``mivq_lvq2_encode`` into two arrays: the primary LVQ rows
(B1 bits per dimension, ``lo``, ``delta``) and the residual stream (B2 bits per dimension, no
per-row constants).  A search scans the primary rows alone (``mivq_lvq_flat_search``) for
``r = min(k * refine_factor, N)`` candidates per query and ranks them again on both levels
(``mivq_rerank_lvq2``): a candidate's distance is the chain of ``mivq_flat_search`` over the
two-level reconstruction, bit for bit.  The candidate ids go from the first kernel to the second
as the device tensor they are; nothing but the (nq, k) result leaves the device.

Unlike ``RefinedIndex(FlatQuantizedIndex(LVQQuantizer(B1)), LVQQuantizer(8))`` the second stage
keeps no second, independent copy of the rows: the residual bits refine the primary ones.

The result conventions are ``RefinedIndex``'s: (nq, k) always, uint32 ids, float32 squared L2
ascending or inner products descending, id 0xFFFFFFFF and FLT_MAX (L2) / -FLT_MAX (IP) in slots
that cannot be filled; the first stage keeps at most 256 results, so ``k * refine_factor`` may not
exceed 256.  ``save`` writes an ``.npz`` of plain arrays.
"""

from __future__ import annotations

from pathlib import Path
from typing import Literal, Optional, Tuple

import numpy as np
import torch

from ... import _arrays, _native
from ..base_search_index import BaseSearchIndex
from ..lvq2_quantization import TwoLevelLVQQuantizer
from ._common import FLT_MAX, METRIC, candidate_count, check_metric, empty_results, results_to_host, save_npz


class LVQ2Index(BaseSearchIndex):
    """LVQ-B1 scan for ``k * refine_factor`` candidates, LVQ-B1xB2 re-rank of them."""

    def __init__(self, primary_bits: int = 4, residual_bits: int = 8, refine_factor: int = 10) -> None:
        self._quantizer = TwoLevelLVQQuantizer(primary_bits, residual_bits)  # refuses bad widths
        if int(refine_factor) < 1:
            raise ValueError(f"refine_factor must be at least 1, got {refine_factor}")
        self._factor = int(refine_factor)
        self._codes1: Optional[torch.Tensor] = None
        self._codes2: Optional[torch.Tensor] = None
        self._metric: Literal["l2", "ip"] = "l2"
        self._N = 0
        self._D = 0

    @property
    def quantizer(self) -> TwoLevelLVQQuantizer:
        return self._quantizer

    @property
    def primary_bits(self) -> int:
        return self._quantizer.primary_bits

    @property
    def residual_bits(self) -> int:
        return self._quantizer.residual_bits

    @property
    def refine_factor(self) -> int:
        return self._factor

    @property
    def ntotal(self) -> int:
        return self._N

    def fit(self, X, metric: Literal["l2", "ip"] = "l2") -> None:
        check_metric(metric)
        Xd = _arrays.to_device(X, torch.float32)
        self._quantizer.fit(Xd)
        self._codes1, self._codes2 = _native.lvq2_encode(Xd, self._quantizer._mu_device(), self.primary_bits,
                                                         self.residual_bits)
        self._metric = metric
        self._N, self._D = int(Xd.shape[0]), int(Xd.shape[1])

    def candidate_count(self, k: int) -> int:
        """r, the candidates the primary scan keeps per query: min(k * refine_factor, N)."""
        return candidate_count(k, self._factor, self._N)

    def search(self, Q, k: int) -> np.ndarray:
        ids, _ = self.search_with_scores(Q, k)
        return ids

    def search_device(self, Qd: torch.Tensor, k: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """Both stages on device tensors: (keys f32 (nq, k) ascending, IP keys negated inner products;
        ids int32 (nq, k) holding uint32 ids), missing slots (+inf, 0xFFFFFFFF).  1 <= k, N >= 1."""
        mt = METRIC[self._metric]
        mu = self._quantizer._mu_device()
        _, cand = _native.lvq_flat_search(Qd, self._codes1, mu, self.primary_bits, self.candidate_count(k), mt)
        return _native.rerank_lvq2(Qd, cand, self._codes1, self._codes2, mu, self.primary_bits, self.residual_bits,
                                   int(k), mt)

    def search_with_scores(self, Q, k: int) -> Tuple[np.ndarray, np.ndarray]:
        r = self.candidate_count(k)
        if self._codes1 is None:
            raise RuntimeError("LVQ2Index must be fit (or loaded) before a search")
        nq = int(Q.shape[0])
        if int(k) <= 0 or nq == 0:
            return empty_results(nq, k)
        sentinel = -FLT_MAX if self._metric == "ip" else FLT_MAX
        if r == 0:  # an empty database
            return np.full((nq, int(k)), _native.NO_ID, dtype=np.uint32), np.full((nq, int(k)), sentinel, dtype=np.float32)
        return results_to_host(*self.search_device(_arrays.to_device(Q, torch.float32), int(k)),
                               negate=self._metric == "ip", sentinel=sentinel)

    def memory_footprint(self) -> int:
        """Both code arrays plus the mean."""
        if self._codes1 is None:
            return 0
        return int(self._codes1.numel() + self._codes2.numel() + self._D * 4)

    def reconstruction_mse(self, X, sample_ids: Optional[np.ndarray] = None) -> Optional[float]:
        if self._codes1 is None:
            return None
        X = np.asarray(X, dtype=np.float32)
        if sample_ids is None:
            sample_ids = np.arange(self._N)
        ids = torch.from_numpy(np.asarray(sample_ids, dtype=np.int64)).to(self._codes1.device)
        xh = _native.lvq2_decode(self._codes1[ids].contiguous(), self._codes2[ids].contiguous(),
                                 self._quantizer._mu_device(), self.primary_bits, self.residual_bits)
        return float(np.mean((X[np.asarray(sample_ids)] - _arrays.to_host(xh)) ** 2))

    # --------------------------------------------------------------- persistence
    def save(self, path: str | Path) -> None:
        if self._codes1 is None:
            raise RuntimeError("LVQ2Index.save() called before fit()")
        save_npz(path, codes1=_arrays.to_host(self._codes1), codes2=_arrays.to_host(self._codes2),
                 mu=np.asarray(self._quantizer.mu, dtype=np.float32), primary_bits=np.array(self.primary_bits),
                 residual_bits=np.array(self.residual_bits), metric=np.array(self._metric),
                 refine_factor=np.array(self._factor), N=np.array(self._N), D=np.array(self._D))

    def load(self, path: str | Path) -> None:
        path = Path(path)
        with np.load(path, allow_pickle=False) as z:
            b1, b2 = int(z["primary_bits"]), int(z["residual_bits"])
            if (b1, b2) != (self.primary_bits, self.residual_bits):
                raise ValueError(f"load(): {path} holds LVQ-{b1}x{b2} codes, this index was built for "
                                 f"LVQ-{self.primary_bits}x{self.residual_bits}")
            codes1, codes2 = np.array(z["codes1"], dtype=np.uint8), np.array(z["codes2"], dtype=np.uint8)
            mu = np.array(z["mu"], dtype=np.float32)
            metric, factor, N, D = str(z["metric"]), int(z["refine_factor"]), int(z["N"]), int(z["D"])
        s1, s2 = _native.lvq2_code_sizes(D, b1, b2)
        if metric not in METRIC or factor < 1 or codes1.shape != (N, s1) or codes2.shape != (N, s2) or mu.shape != (D,):
            raise ValueError(f"load(): {path} is not a consistent LVQ2Index file")
        self._quantizer.mu = mu
        self._codes1 = _arrays.to_device(codes1, torch.uint8)
        self._codes2 = _arrays.to_device(codes2, torch.uint8)
        self._metric, self._factor, self._N, self._D = metric, factor, N, D
