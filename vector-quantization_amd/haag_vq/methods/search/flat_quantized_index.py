"""Flat (brute-force) search over quantized codes, on the MI355X.

``FlatQuantizedIndex`` keeps the interface of the reference's class
(/root/reference/src/haag_vq/methods/search/flat_quantized_index.py:17-154): fit compresses
the database, ``search_with_scores`` returns ``(ids uint32, dists float32)`` sorted best
first (squared L2 ascending, or inner product descending), ``memory_footprint`` is the code
bytes, ``save`` / ``load`` round-trip the index.  The reference decodes every code and runs
``scipy.cdist`` + ``argpartition``; here:

* PQ / OPQ codes are ranked by ADC — per-query lookup tables (``mivq_adc_lut``) summed over
  the codes (``mivq_adc_search``).  sum_m ||q_m - c_{m,code_m}||^2 equals ||q - x_hat||^2
  (OPQ: for the rotated query, which the orthonormal rotation preserves), so the ranking is
  the reference's up to fp32 rounding on near-ties, without materialising x_hat.
* SQ codes of an f32 fit and RaBitQ-1 codes are searched exactly as they are
  (``mivq_sq_flat_search`` / ``mivq_rabitq_flat_search``: dequantised in registers, the ids and
  distances of decode + ``mivq_flat_search`` bit for bit, no fp32 copy of the database).
* LVQ codes likewise (``mivq_lvq_flat_search``: the MSB-first bit stream and the per-row
  ``lo`` / ``delta`` read in the scan, the ids and distances of ``mivq_lvq_decode`` +
  ``mivq_flat_search`` bit for bit).
* other quantizers (f64-fitted SQ, Extended RaBitQ, rank-aware, ...) are decoded on the device
  and searched exactly (``mivq_flat_search``).

``RankAwareFlatIndex`` searches rank-aware codes without decoding them: the queries are rotated
onto the PCA axes and the packed fields are scanned against the per-dimension level tables
(``mivq_rankaware_flat_search``).  ``ExtendedRaBitQFlatIndex`` does the same for Extended RaBitQ
codes: the queries are rotated by P and the bit fields are scanned against the shared level
table and each row's ``nrm`` / ``t`` (``mivq_extrabitq_flat_search``).

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
from ..optimized_product_quantization import OptimizedProductQuantizer, OPQHandle
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
    if isinstance(model, (ProductQuantizer, OptimizedProductQuantizer)):
        pq = model if isinstance(model, ProductQuantizer) else model.inner
        if isinstance(model, OptimizedProductQuantizer):
            Qd = model.opq.apply(Qd)
        cd = cd.to(torch.uint8).contiguous()
        u8 = cd if pq.B == 8 else _native.pq_unpack(cd, pq.M, pq.B)
        lut = _native.adc_lut(Qd, pq.centroids_device, pq.B, mt)
        d, i = _native.adc_search(lut, u8, k, pq.B, id_offset=id_offset)
    elif isinstance(model, ScalarQuantizer) and model.min is not None and np.asarray(model.min).dtype == np.float32:
        # f32-fitted SQ: the codes are scanned as they are (an f64 fit decodes in f64 and rounds
        # to f32 afterwards, which the f32 dequantisation of the kernel does not reproduce)
        lo, den = model._params(torch.float32)
        d, i = _native.sq_flat_search(Qd, cd.contiguous(), len(model.min), lo, den, model.num_bits, k, mt,
                                      id_offset=id_offset)
    elif isinstance(model, RaBitQuantizer) and model.rabitq is not None:
        d, i = _native.rabitq_flat_search(Qd, _arrays.to_device(cd, torch.uint8).contiguous(), model.rabitq.d, None, k,
                                          mt, id_offset=id_offset)
    elif isinstance(model, LVQQuantizer) and model.mu is not None:
        d, i = _native.lvq_flat_search(Qd, _arrays.to_device(cd, torch.uint8).contiguous(), model._mu_device(),
                                       model.num_bits, k, mt, id_offset=id_offset)
    else:
        xh = model.decompress(cd)
        xh = _arrays.to_device(xh, torch.float32)
        d, i = _native.flat_search(Qd, xh, k, mt, id_offset=id_offset)
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


def quantizer_state(q: BaseQuantizer) -> dict:
    """A fitted quantizer as plain numpy arrays (index files; the rank-0 -> all-ranks
    broadcast of parallel/sharded.py)."""
    if isinstance(q, ProductQuantizer):
        return dict(qtype=np.array("pq"), M=np.array(q.M), B=np.array(q.B), centroids=_arrays.to_host(q._C))
    if isinstance(q, OptimizedProductQuantizer):
        return dict(qtype=np.array("opq"), M=np.array(q.M), B=np.array(q.B), A=_arrays.to_host(q.opq.A_device),
                    centroids=_arrays.to_host(q.inner._C))
    if isinstance(q, ScalarQuantizer):
        return dict(qtype=np.array("sq"), num_bits=np.array(q.num_bits), min=np.asarray(q.min), max=np.asarray(q.max))
    if isinstance(q, RaBitQuantizer):
        return dict(qtype=np.array("rabitq"), metric_type=np.array(int(q.metric_type)), d=np.array(q.rabitq.d))
    if isinstance(q, LVQQuantizer):
        return dict(qtype=np.array("lvq"), num_bits=np.array(q.num_bits), mu=np.asarray(q.mu, dtype=np.float32))
    if isinstance(q, RankAwareQuantizer):
        if q.V is None:
            raise ValueError("save(): the RankAwareQuantizer is not fitted")
        st = dict(qtype=np.array("rankaware"), avg_bits=np.array(q.avg_bits), alpha=np.array(q.alpha),
                  max_bits=np.array(q.max_bits), seed=np.array(q.seed), packing=np.array(q.packing),
                  mu=np.asarray(q.mu, dtype=np.float64), V=np.ascontiguousarray(q.V, dtype=np.float64),
                  var=np.asarray(q.var, dtype=np.float64), bits=np.asarray(q.bits, dtype=np.int64),
                  cb=np.concatenate(q.cb).astype(np.float64), levels=np.concatenate(q._levels).astype(np.float64),
                  Dg=np.asarray(q._Dg, dtype=np.float64))
        # written only when not the defaults: a gaussian quantizer's file keeps its bytes
        if q.codebook != "gaussian":
            st["codebook"] = np.array(q.codebook)
        if q.codebook_engine != "saq":
            st["codebook_engine"] = np.array(q.codebook_engine)
        return st
    if isinstance(q, ExtendedRaBitQuantizer):
        if q.P is None:
            raise ValueError("save(): the ExtendedRaBitQuantizer is not fitted")
        return dict(qtype=np.array("extrabitq"), num_bits=np.array(q.num_bits), seed=np.array(q.seed), D=np.array(q.D),
                    c=np.asarray(q.c, dtype=np.float64), P=np.ascontiguousarray(q.P, dtype=np.float64),
                    levels=np.asarray(q.levels, dtype=np.float64))
    raise ValueError(f"save(): unsupported quantizer {type(q).__name__}")


def quantizer_from_state(z) -> BaseQuantizer:
    """Inverse of quantizer_state (z: a mapping of numpy arrays, e.g. an open .npz)."""
    qt = str(z["qtype"])
    if qt == "pq":
        q = ProductQuantizer(M=int(z["M"]), B=int(z["B"]))
        q.set_codebooks(z["centroids"])
    elif qt == "opq":
        q = OptimizedProductQuantizer(M=int(z["M"]), B=int(z["B"]))
        q.opq = OPQHandle(_arrays.to_device(z["A"]))
        inner = ProductQuantizer(M=int(z["M"]), B=int(z["B"]))
        inner.set_codebooks(z["centroids"])
        q._inner = inner
        q.pq = inner.pq
    elif qt == "sq":
        q = ScalarQuantizer(num_bits=int(z["num_bits"]))
        q.min = np.array(z["min"])
        q.max = np.array(z["max"])
    elif qt == "rabitq":
        from ...utils.faiss_utils import MetricType
        q = RaBitQuantizer(metric_type=MetricType(int(z["metric_type"])))
        q.fit(np.empty((0, int(z["d"])), dtype=np.float32))
    elif qt == "lvq":
        q = LVQQuantizer(num_bits=int(z["num_bits"]))
        q.mu = np.array(z["mu"])
    elif qt == "rankaware":
        q = RankAwareQuantizer(avg_bits=float(z["avg_bits"]), alpha=float(z["alpha"]), max_bits=int(z["max_bits"]),
                               seed=int(z["seed"]), packing=str(z["packing"]),
                               codebook=str(z["codebook"]) if "codebook" in z else "gaussian",
                               codebook_engine=str(z["codebook_engine"]) if "codebook_engine" in z else "saq")
        q.mu, q.V, q.var = np.array(z["mu"]), np.array(z["V"]), np.array(z["var"])
        q.bits = np.array(z["bits"], dtype=np.int64)
        q.D = int(q.bits.shape[0])
        ends = np.cumsum(2 ** q.bits)
        cb = np.array(z["cb"], dtype=np.float64)
        if cb.shape != (int(ends[-1]),) or q.V.shape != (q.D, q.D) or q.mu.shape != (q.D,):
            raise ValueError("load(): inconsistent rank-aware quantizer state")
        q.cb = [cb[e - 2 ** b:e] for e, b in zip(ends, q.bits)]
        lv = np.array(z["levels"], dtype=np.float64)
        q._levels = [lv[2 ** b - 1:2 ** (b + 1) - 1] for b in range(q.max_bits + 1)]
        q._Dg = np.array(z["Dg"])
        q._layout()
    elif qt == "extrabitq":
        q = ExtendedRaBitQuantizer(num_bits=int(z["num_bits"]), seed=int(z["seed"]))
        q.D = int(z["D"])
        q.c, q.P, q.levels = (np.array(z[nm], dtype=np.float64) for nm in ("c", "P", "levels"))
        if q.c.shape != (q.D,) or q.P.shape != (q.D, q.D) or q.levels.shape != (2 ** q.num_bits,):
            raise ValueError("load(): inconsistent Extended RaBitQ quantizer state")
    else:
        raise ValueError(f"load(): unknown quantizer type {qt!r}")
    return q


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


class RankAwareFlatIndex(FlatQuantizedIndex):
    """FlatQuantizedIndex over RankAwareQuantizer codes, searched in the rotated domain.

    ``FlatQuantizedIndex`` decodes the whole database on every call (dequantize, an N x D x D
    fp64 product, two N x D fp64 intermediates).  Here only the queries are rotated
    (``RankAwareQuantizer.search_codes``): ||q - x_hat||^2 = ||(q - mu) V - y_hat||^2 for the
    orthogonal V.  Distances differ from the decode path's by fp32 rounding (the sum runs over the
    rotated coordinates), so near-ties may rank differently; k > 256 takes the inherited path.
    Index files are those of FlatQuantizedIndex: either class loads the other's."""

    def __init__(self, quantizer: BaseQuantizer) -> None:
        if not isinstance(quantizer, RankAwareQuantizer):
            raise ValueError("RankAwareFlatIndex needs a RankAwareQuantizer")
        super().__init__(quantizer)

    def _search_codes(self, Q, k: int) -> Tuple[torch.Tensor, torch.Tensor]:
        if k > MAX_KERNEL_K:
            return super()._search_codes(Q, k)
        return self._quantizer.search_codes(self._codes, Q, k, self._metric)

    def load(self, path: str | Path) -> None:
        got = FlatQuantizedIndex(self._quantizer)
        got.load(path)
        if not isinstance(got._quantizer, RankAwareQuantizer):
            raise ValueError(f"load(): {path} holds a {type(got._quantizer).__name__}, not a RankAwareQuantizer")
        self._quantizer, self._codes, self._metric = got._quantizer, got._codes, got._metric
        self._N, self._D = got._N, got._D


class ExtendedRaBitQFlatIndex(FlatQuantizedIndex):
    """FlatQuantizedIndex over ExtendedRaBitQuantizer codes, searched in the rotated domain.

    ``FlatQuantizedIndex`` decodes the whole database on every call (dequantize, an N x D x D
    fp64 product, an N x D fp32 copy).  Here only the queries are rotated
    (``ExtendedRaBitQuantizer.search_codes``): ||q - x_hat||^2 = ||(q - c) P - y_hat||^2 for the
    orthogonal P.  Distances differ from the decode path's by fp32 rounding (the sum runs over the
    rotated coordinates), so near-ties may rank differently; k > 256 takes the inherited path.
    Index files are those of FlatQuantizedIndex: either class loads the other's."""

    def __init__(self, quantizer: BaseQuantizer) -> None:
        if not isinstance(quantizer, ExtendedRaBitQuantizer):
            raise ValueError("ExtendedRaBitQFlatIndex needs an ExtendedRaBitQuantizer")
        super().__init__(quantizer)

    def search_with_scores(self, Q, k: int) -> Tuple[np.ndarray, np.ndarray]:
        if self._codes is None:
            raise RuntimeError("ExtendedRaBitQFlatIndex must be fit (or loaded) before a search")
        return super().search_with_scores(Q, k)

    def _search_codes(self, Q, k: int) -> Tuple[torch.Tensor, torch.Tensor]:
        if k > MAX_KERNEL_K:
            return super()._search_codes(Q, k)
        return self._quantizer.search_codes(self._codes, Q, k, self._metric)

    def save(self, path: str | Path) -> None:
        if self._codes is None:
            raise RuntimeError("ExtendedRaBitQFlatIndex must be fit (or loaded) before save()")
        super().save(path)

    def load(self, path: str | Path) -> None:
        got = FlatQuantizedIndex(self._quantizer)
        got.load(path)
        if not isinstance(got._quantizer, ExtendedRaBitQuantizer):
            raise ValueError(f"load(): {path} holds a {type(got._quantizer).__name__}, not an ExtendedRaBitQuantizer")
        self._quantizer, self._codes, self._metric = got._quantizer, got._codes, got._metric
        self._N, self._D = got._N, got._D
