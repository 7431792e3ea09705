"""Flat (brute-force) search over quantized codes, on the MI355X.

``FlatQuantizedIndex`` keeps the interface of the reference's class
(/root/reference/src/haag_vq/methods/search/flat_quantized_index.py:17-154): fit compresses
the database, ``search_with_scores`` returns ``(ids uint32, dists float32)`` sorted best
first (squared L2 ascending, or inner product descending), ``memory_footprint`` is the code
bytes, ``save`` / ``load`` round-trip the index.  The reference decodes every code and runs
``scipy.cdist`` + ``argpartition``; here the quantizer ranks its own codes
(``BaseQuantizer.flat_keys``).  Which quantizer takes which kernel chain is written on the classes,
not here: the default decodes on the device and searches exactly (``mivq_flat_search``), and a
class whose codes can be ranked as they are overrides it (PQ / OPQ by ADC; f32-fitted SQ, RaBitQ-1
and LVQ by their code-domain searches, bit for bit the default's result).  So is the saved state
(``to_state`` / ``from_state``); ``QUANTIZER_TYPES`` names the classes a file can hold.

``RankAwareFlatIndex`` / ``ExtendedRaBitQFlatIndex`` rank by the quantizer's own ``search_codes``
(methods/_rotated.py); a ``FlatQuantizedIndex`` over the same quantizers takes the default.

Ties are broken by the smaller id.  Saved indices are ``.npz`` archives of plain arrays
(loaded with ``allow_pickle=False``).
"""

from __future__ import annotations

from pathlib import Path
from typing import Literal, Optional, Tuple

import numpy as np
import torch

from ... import _arrays, _native
from ..base_quantizer import BaseQuantizer
from ..base_search_index import BaseSearchIndex
from ..extended_rabitq import ExtendedRaBitQuantizer
from ..lvq_quantization import LVQQuantizer
from ..optimized_product_quantization import OptimizedProductQuantizer
from ..product_quantization import ProductQuantizer
from ..rabit_quantization import RaBitQuantizer
from ..rank_aware_quantization import RankAwareQuantizer
from ..scalar_quantization import ScalarQuantizer
from ._common import MAX_K as MAX_KERNEL_K  # the wave-resident top-k of the scan kernels
from ._common import METRIC, check_metric, empty_results, results_to_host, save_npz


def search_codes(model: BaseQuantizer, codes, Q, k: int, metric: str = "l2",
                 id_offset: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """Top-k of queries Q against encoded database ``codes`` of ``model`` (device tensors).

    Returns (dists f32 (nq, k), ids int32 (nq, k) holding uint32 ids); IP distances are
    returned as inner products (descending).  ``id_offset`` is added to every id (the first
    global row of a database shard, parallel/sharded.py).
    """
    mt = METRIC[metric]
    Qd = _arrays.to_device(Q)
    cd = codes if _arrays.is_tensor(codes) else torch.from_numpy(np.ascontiguousarray(codes))
    cd = cd.to(_arrays.device())
    if k > MAX_KERNEL_K:
        d, i = _search_large_k(model, cd, Qd, k, mt)
        if id_offset:
            # ids are uint32 bit patterns in int32: mask before adding, and keep the
            # 0xFFFFFFFF sentinel as it is
            g = ((i.to(torch.int64) & 0xFFFFFFFF) + id_offset) & 0xFFFFFFFF
            i = torch.where(i == -1, i, (g - (g >= 2 ** 31).to(torch.int64) * 2 ** 32).to(torch.int32))
        return d, i
    d, i = model.flat_keys(cd, Qd, k, mt, id_offset)
    if mt == _native.METRIC_INNER_PRODUCT:
        d = -d
    return d, i


def _search_large_k(model, cd, Qd, k: int, mt: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """k > 256 (the reference's cdist + argpartition has no limit): decode once, exact
    (query, row) distances with mivq_pairwise_distances in query blocks, and a stable
    device sort, so ties keep the smaller id first."""
    xh = _arrays.to_device(model.decompress(cd), torch.float32)
    n = xh.shape[0]
    k = min(k, n)
    block = max(1, (1 << 28) // max(1, n))
    ds, is_ = [], []
    for s in range(0, Qd.shape[0], block):
        D = _native.pairwise_distances(Qd[s:s + block].contiguous(), xh, mt)
        v, i = torch.sort(D, dim=1, stable=True)
        ds.append(v[:, :k].contiguous())
        is_.append(i[:, :k].to(torch.int32).contiguous())
    d, i = torch.cat(ds), torch.cat(is_)
    if mt == _native.METRIC_INNER_PRODUCT:
        d = -d
    return d, i


def ids_to_numpy(i: torch.Tensor) -> np.ndarray:
    return _arrays.to_host(i).view(np.uint32)


# what an index file or the sharded broadcast can hold, by the "qtype" member of the state
QUANTIZER_TYPES = {"pq": ProductQuantizer, "opq": OptimizedProductQuantizer, "sq": ScalarQuantizer,
                   "rabitq": RaBitQuantizer, "lvq": LVQQuantizer, "rankaware": RankAwareQuantizer,
                   "extrabitq": ExtendedRaBitQuantizer}


def quantizer_state(q: BaseQuantizer) -> dict:
    """A fitted quantizer as plain numpy arrays (index files; the rank-0 -> all-ranks
    broadcast of parallel/sharded.py)."""
    return q.to_state()


def quantizer_from_state(z) -> BaseQuantizer:
    """Inverse of quantizer_state (z: a mapping of numpy arrays, e.g. an open .npz)."""
    qt = str(z["qtype"])
    if qt not in QUANTIZER_TYPES:
        raise ValueError(f"load(): unknown quantizer type {qt!r}")
    return QUANTIZER_TYPES[qt].from_state(z)


class FlatQuantizedIndex(BaseSearchIndex):
    """Brute-force search over the codes of any BaseQuantizer (GPU ADC for PQ / OPQ)."""

    def __init__(self, quantizer: BaseQuantizer) -> None:
        self._quantizer = quantizer
        self._codes: Optional[torch.Tensor] = None
        self._metric: Literal["l2", "ip"] = "l2"
        self._N = 0
        self._D = 0

    @property
    def quantizer(self) -> BaseQuantizer:
        return self._quantizer

    def fit(self, X, metric: Literal["l2", "ip"] = "l2") -> None:
        check_metric(metric)
        Xd = _arrays.to_device(X, torch.float32)
        self._metric = metric
        self._N, self._D = Xd.shape
        self._quantizer.fit(Xd)
        self._codes = self._quantizer.compress(Xd)

    def search(self, Q, k: int) -> np.ndarray:
        ids, _ = self.search_with_scores(Q, k)
        return ids

    def _search_codes(self, Q, k: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """The device search of search_with_scores, 1 <= k <= N."""
        return search_codes(self._quantizer, self._codes, Q, k, self._metric)

    def search_with_scores(self, Q, k: int) -> Tuple[np.ndarray, np.ndarray]:
        Q = np.ascontiguousarray(Q, dtype=np.float32) if not _arrays.is_tensor(Q) else Q
        k = min(int(k), self._N)
        if k <= 0:
            return empty_results(Q.shape[0], 0)
        return results_to_host(*self._search_codes(Q, k))

    def memory_footprint(self) -> int:
        return int(self._codes.numel() * self._codes.element_size()) if self._codes is not None else 0

    def reconstruction_mse(self, X, sample_ids: Optional[np.ndarray] = None) -> Optional[float]:
        if self._codes is None:
            return None
        X = np.asarray(X, dtype=np.float32)
        if sample_ids is None:
            sample_ids = np.arange(self._N)
        ids = torch.from_numpy(np.asarray(sample_ids, dtype=np.int64)).to(self._codes.device)
        xh = self._quantizer.decompress(self._codes[ids].contiguous())
        xh = _arrays.to_host(xh).astype(np.float32)
        return float(np.mean((X[np.asarray(sample_ids)] - xh) ** 2))

    # --------------------------------------------------------------- persistence
    def _state(self) -> dict:
        st = {"codes": _arrays.to_host(self._codes), "metric": np.array(self._metric),
              "N": np.array(self._N), "D": np.array(self._D)}
        st.update(quantizer_state(self._quantizer))
        return st

    def save(self, path: str | Path) -> None:
        save_npz(path, **self._state())

    def load(self, path: str | Path) -> None:
        with np.load(Path(path), allow_pickle=False) as z:
            q = quantizer_from_state(z)
            self._quantizer = q
            self._codes = torch.from_numpy(np.array(z["codes"])).to(_arrays.device())
            self._metric = str(z["metric"])
            self._N = int(z["N"])
            self._D = int(z["D"])


class FlatADCIndex(FlatQuantizedIndex):
    """FlatQuantizedIndex restricted to PQ / OPQ codes (pure LUT-sum ADC search)."""

    def __init__(self, quantizer: BaseQuantizer) -> None:
        if not isinstance(quantizer, (ProductQuantizer, OptimizedProductQuantizer)):
            raise ValueError("FlatADCIndex needs a ProductQuantizer or OptimizedProductQuantizer")
        super().__init__(quantizer)


class _RotatedFlatIndex(FlatQuantizedIndex):
    """FlatQuantizedIndex over the codes of ``QUANTIZER``, searched in the rotated domain.

    ``FlatQuantizedIndex`` decodes the whole database on every call (dequantize, an N x D x D fp64
    product, N x D intermediates).  Here only the queries are rotated (the quantizer's
    ``search_codes``, methods/_rotated.py): ||q - x_hat||^2 = ||(q - centre) R - y_hat||^2 for the
    orthogonal R.  Distances differ from the decode path's by fp32 rounding (the sum runs over the
    rotated coordinates), so near-ties may rank differently; k > 256 takes the inherited path.
    Index files are those of FlatQuantizedIndex: either class loads the other's."""

    def __init__(self, quantizer: BaseQuantizer) -> None:
        if not isinstance(quantizer, self.QUANTIZER):
            raise ValueError(f"{type(self).__name__} needs {self._NEEDS}")
        super().__init__(quantizer)

    def _search_codes(self, Q, k: int) -> Tuple[torch.Tensor, torch.Tensor]:
        if k > MAX_KERNEL_K:
            return super()._search_codes(Q, k)
        return self._quantizer.search_codes(self._codes, Q, k, self._metric)

    def load(self, path: str | Path) -> None:
        got = FlatQuantizedIndex(self._quantizer)
        got.load(path)
        if not isinstance(got._quantizer, self.QUANTIZER):
            raise ValueError(f"load(): {path} holds a {type(got._quantizer).__name__}, not {self._NEEDS}")
        self._quantizer, self._codes, self._metric = got._quantizer, got._codes, got._metric
        self._N, self._D = got._N, got._D


class RankAwareFlatIndex(_RotatedFlatIndex):
    """RankAwareQuantizer codes against (q - mu) V: ``mivq_rankaware_flat_search``."""

    QUANTIZER, _NEEDS = RankAwareQuantizer, "a RankAwareQuantizer"


class ExtendedRaBitQFlatIndex(_RotatedFlatIndex):
    """ExtendedRaBitQuantizer codes against (q - c) P: ``mivq_extrabitq_flat_search``."""

    QUANTIZER, _NEEDS = ExtendedRaBitQuantizer, "an ExtendedRaBitQuantizer"

    def search_with_scores(self, Q, k: int) -> Tuple[np.ndarray, np.ndarray]:
        if self._codes is None:
            raise RuntimeError("ExtendedRaBitQFlatIndex must be fit (or loaded) before a search")
        return super().search_with_scores(Q, k)

    def save(self, path: str | Path) -> None:
        if self._codes is None:
            raise RuntimeError("ExtendedRaBitQFlatIndex must be fit (or loaded) before save()")
        super().save(path)
