"""Rank-aware quantizer (PCA + greedy bits per dimension) on the MI355X.

Drop-in for the reference's ``RankAwareQuantizer`` (methods/rank_aware_quantization.py) with
its default ``codebook="gaussian"``: rows are centred, rotated onto the PCA axes, and every
rotated dimension d gets ``bits[d]`` bits from a greedy that weights the MSE gain of one more
bit by ``var_d ** alpha``; dimension d is quantized on the ``2 ** bits[d]`` Gaussian-optimal
levels scaled by ``sqrt(var_d)``, and a row's indices are packed as variable-width fields,
either back to back (``packing="dense"``, numpy's packbits order) or whole inside bytes
(``packing="ffd"``, ffd_packing.py).

Where the work runs:

* ``fit``: column sums (fp64) and the Gram matrix X^T X (``mivq_opq_gram``, fp64 MFMA, for
  f32 rows) on the device; everything D-sized (eigh, the allocation greedy, the level tables,
  the layout) on the host exactly as the reference does it.  The N(0,1) Lloyd tables depend only
  on ``(seed + b, 2 ** b)`` and are cached per process.
* ``compress`` / ``decompress``: ``mivq_rankaware_center`` -> ``mivq_extrabitq_rotate`` (the
  fp64 MFMA GEMM) -> ``mivq_rankaware_quantize`` and the mirror image, fp64 throughout.
* ``search_codes``: the queries are rotated (``rotate_queries``, fp64, rounded once) and the
  packed codes are scanned as they are (``mivq_rankaware_flat_search``); no row is decoded.

Parity: the GEMM's summation order differs from numpy's, so an index can differ from the
reference's only by one and only where the rotated value lies within rounding distance of the
boundary between two levels; decoded rows agree to an f32 ulp.

The data-fitted codebooks (``codebook="lloyd"`` / ``"exact"``): the reference fits them with the
SAQ engine, which is out of scope of this build, so with the default ``codebook_engine="saq"``
the constructor accepts them and ``fit`` raises.  ``codebook_engine="device"`` fits them here:
``fit`` takes the reference's sample (all rows, or 200 000 drawn by ``default_rng(0)``), centres
and rotates it on the device, rounds to f32, sorts every column (``torch.sort``) and hands the
(D, n) columns to ``mivq_codebook1d_fit``: the globally optimal 1-D k-means by dynamic
programming (``"exact"``) or k-means++ / Lloyd (``"lloyd"``, the study's own method), one
workgroup per dimension, bit for bit the reference builders' sequential fp64 arithmetic on the
same columns.  A dimension with no more than ``2 ** bits`` distinct sample values gets those
values, padded with the last one to ``2 ** bits`` levels (the reference leaves its Lloyd table
short there); a row beyond the last level then carries another index of the same value.
"""

from __future__ import annotations

import numpy as np
import torch

from .. import _arrays, _native
from ._rotated import RotatedSearch
from .base_quantizer import BaseQuantizer
from .ffd_packing import ffd_layout

_LLOYD_CACHE: dict = {}
CB_SAMPLE = 200_000   # rows the data-fitted codebooks are trained on (the reference's CB_SAMPLE)


def _lloyd_1d_normal(num_levels: int, seed: int, n_samples: int = 200_000, max_iter: int = 100,
                     tol: float = 1e-7):
    """``(levels, dmse)``: the 1-D Lloyd codebook of a seeded N(0,1) sample and its MSE on that
    sample relative to the sample's second moment.  One level: 0.0 and 1.0.  The per-level
    ``samples[sel].mean()`` is the reference's: another summation changes the levels' bits."""
    key = (int(seed), int(num_levels), int(n_samples), int(max_iter), float(tol))
    hit = _LLOYD_CACHE.get(key)
    if hit is not None:
        return hit[0].copy(), hit[1]
    rng = np.random.default_rng(seed)
    samples = rng.standard_normal(n_samples)
    var = float(np.mean(samples ** 2))
    if num_levels == 1:
        levels = np.array([0.0], dtype=np.float64)
        dmse = float(np.mean((samples - 0.0) ** 2) / var)
    else:
        levels = np.quantile(samples, (np.arange(num_levels) + 0.5) / num_levels)
        for _ in range(max_iter):
            idx = np.searchsorted(0.5 * (levels[:-1] + levels[1:]), samples)
            new = levels.copy()
            for k in range(num_levels):
                sel = idx == k
                if np.any(sel):
                    new[k] = samples[sel].mean()
            new.sort()
            shift = float(np.max(np.abs(new - levels)))
            levels = new
            if shift < tol:
                break
        idx = np.searchsorted(0.5 * (levels[:-1] + levels[1:]), samples)
        dmse = float(np.mean((samples - levels[idx]) ** 2) / var)
        levels = levels.astype(np.float64)
    _LLOYD_CACHE[key] = (levels, dmse)
    return levels.copy(), dmse


def allocate_bits(var: np.ndarray, Dg: np.ndarray, avg_bits: float, alpha: float, max_bits: int) -> np.ndarray:
    """The greedy: ``round(avg_bits * D)`` times, one more bit to the dimension whose
    ``var ** (1 + alpha) * (Dg[b] - Dg[b + 1])`` is largest (first index on ties), dimensions at
    ``max_bits`` excluded; stops early when every dimension is at the cap."""
    D = var.shape[0]
    total = int(round(avg_bits * D))
    bits = np.zeros(D, dtype=np.int64)
    var_pow = var ** (1.0 + alpha)
    gain = var_pow * (Dg[0] - Dg[1])  # max_bits >= 1: no dimension starts at the cap
    for _ in range(total):
        d = int(np.argmax(gain))
        if not np.isfinite(gain[d]):
            break
        bits[d] += 1
        b = bits[d]
        gain[d] = var_pow[d] * (Dg[b] - Dg[b + 1]) if b < max_bits else -np.inf
    assert bits.sum() <= total
    return bits


class RankAwareQuantizer(RotatedSearch, BaseQuantizer):
    qtype = "rankaware"

    def __init__(self, avg_bits: float, alpha: float = 1.0, max_bits: int = 8, seed: int = 0,
                 packing: str = "dense", codebook: str = "gaussian", codebook_engine: str = "saq"):
        if max_bits < 1 or max_bits > 8:
            raise ValueError("max_bits must be in [1, 8]")
        if packing not in ("dense", "ffd"):
            raise ValueError("packing must be 'dense' or 'ffd'")
        if codebook not in ("gaussian", "lloyd", "exact"):
            raise ValueError("codebook must be 'gaussian', 'lloyd', or 'exact'")
        if codebook_engine not in ("saq", "device"):
            raise ValueError("codebook_engine must be 'saq' or 'device'")
        self.codebook = codebook
        self.codebook_engine = codebook_engine
        self.avg_bits = float(avg_bits)
        self.alpha = float(alpha)
        self.max_bits = int(max_bits)
        self.seed = int(seed)
        self.packing = packing
        self.mu: np.ndarray | None = None
        self.V: np.ndarray | None = None
        self.var: np.ndarray | None = None
        self.bits: np.ndarray | None = None
        self.cb: list[np.ndarray] | None = None
        self.D: int | None = None
        self._offsets: np.ndarray | None = None
        self.code_size: int | None = None
        self._levels = None
        self._Dg = None
        self._ffd_byte_idx: np.ndarray | None = None
        self._ffd_bit_off: np.ndarray | None = None
        self._ffd_n_bytes: int | None = None
        self._dev = None
        self._stage_bytes = _arrays.STAGE_BYTES  # device bytes one chunk of a numpy input may take

    # ------------------------------------------------------------------ fit
    def _moments(self, X):
        """(N, S = column sums, G = X^T X) in fp64, summed on the device."""
        if _arrays.is_tensor(X):
            dt = X.dtype if X.dtype in (torch.float32, torch.float64) else torch.float64
            chunks = [_arrays.to_device(X, dt)]
            N, D = X.shape
        else:
            X = np.asarray(X)
            N, D = X.shape
            dt = torch.float32 if X.dtype == np.float32 else torch.float64
            width = 4 if dt == torch.float32 else 8
            chunks = (_arrays.to_device(X[s:e], dt) for s, e in _arrays.row_chunks(N, D * width, self._stage_bytes))
        dev = _arrays.device()
        S = torch.zeros(D, dtype=torch.float64, device=dev)
        G = torch.zeros((D, D), dtype=torch.float64, device=dev)
        for x in chunks:
            S += x.sum(dim=0, dtype=torch.float64)
            G += _native.opq_gram(x, x) if dt == torch.float32 else x.T @ x
        return int(N), _arrays.to_host(S), _arrays.to_host(G)

    def fit(self, X) -> None:
        if self.codebook != "gaussian" and self.codebook_engine == "saq":
            raise ValueError(f"codebook={self.codebook!r} is fitted by the SAQ engine, which is out of scope of the "
                             "MI355X build; use codebook='gaussian'")
        if not _arrays.is_tensor(X):
            X = np.asarray(X)
        if len(X.shape) != 2 or X.shape[0] < 1:
            raise ValueError(f"fit() needs a non-empty (N, D) array, got shape {tuple(X.shape)}")
        N, S, G = self._moments(X)
        D = S.shape[0]
        self.D = int(D)
        self.mu = S / N
        C = G / N - np.outer(self.mu, self.mu)
        w, Vt = np.linalg.eigh(C)
        order = np.argsort(w)[::-1]
        self.var = np.clip(w[order], 1e-12, None)
        self.V = Vt[:, order]

        self._levels = [None] * (self.max_bits + 1)
        Dg = np.empty(self.max_bits + 1, dtype=np.float64)
        for b in range(self.max_bits + 1):
            self._levels[b], Dg[b] = _lloyd_1d_normal(2 ** b, seed=self.seed + b)
        Dg[0] = 1.0
        self._Dg = Dg
        self.bits = allocate_bits(self.var, Dg, self.avg_bits, self.alpha, self.max_bits)
        if self.codebook == "gaussian":
            scale = np.sqrt(self.var)
            self.cb = [self._levels[int(b)] * scale[d] for d, b in enumerate(self.bits)]
        else:
            self.cb = self._fit_codebooks(X)
        self._layout()

    def _sample_projection(self, X) -> torch.Tensor:
        """The sample the fitted codebooks are trained on, rotated: (D, n) f32 on the device, all
        rows of X or CB_SAMPLE of them drawn by ``default_rng(0)``; ``(x - mu) V`` in fp64 on the
        device, rounded to f32."""
        N = int(X.shape[0])
        if N > CB_SAMPLE:
            idx = np.random.default_rng(0).choice(N, CB_SAMPLE, replace=False)
            X = X[torch.from_numpy(idx).to(X.device)] if _arrays.is_tensor(X) else np.asarray(X)[idx]
        n = int(X.shape[0])
        dev = _arrays.device()
        mu = _arrays.to_device(np.ascontiguousarray(self.mu, dtype=np.float64), torch.float64)
        V = _arrays.to_device(np.ascontiguousarray(self.V, dtype=np.float64), torch.float64)
        cols = torch.empty((self.D, n), dtype=torch.float32, device=dev)
        for s, e in _arrays.row_chunks(n, self.D * 24, self._stage_bytes):
            x = X[s:e]
            if _arrays.is_tensor(x):
                dt = x.dtype if x.dtype in (torch.float32, torch.float64) else torch.float64
            else:
                dt = torch.float32 if x.dtype == np.float32 else torch.float64
            y = _native.gemm_f64(_native.rankaware_center(_arrays.to_device(x, dt).contiguous(), mu), V, False)
            cols[:, s:e] = y.to(torch.float32).T
        return cols

    def sample_columns(self, X) -> torch.Tensor:
        """What ``_fit_codebooks`` hands to ``mivq_codebook1d_fit``: row d = the sample's rotated
        dimension d (``_sample_projection``) in ascending order."""
        return torch.sort(self._sample_projection(X), dim=1).values.contiguous()

    def _fit_codebooks(self, X) -> list:
        """The reference's step 5 for ``codebook`` "lloyd" / "exact" on the fitted ``mu``, ``V``
        and ``bits``: one table of ``2 ** bits[d]`` f64 levels per dimension ([0.0] for 0 bits)."""
        if self.codebook not in _native.CB1D_METHODS:
            raise ValueError(f"codebook={self.codebook!r} has no fitted tables")
        if not _arrays.is_tensor(X):
            X = np.asarray(X)
        levels, lv_off, _ = _native.codebook1d_fit(self.sample_columns(X), self.bits, self.codebook)
        lv = _arrays.to_host(levels).astype(np.float64)
        return [lv[lv_off[d]:lv_off[d + 1]] if b else np.array([0.0]) for d, b in enumerate(self.bits)]

    def _layout(self) -> None:
        """Bit offsets, the FFD layout and the code size, from ``bits`` and ``packing``."""
        self._offsets = np.concatenate(([0], np.cumsum(self.bits))).astype(np.int64)
        if self.packing == "ffd":
            byte_idx, bit_off, n_bytes = ffd_layout(self.bits)
            self._ffd_byte_idx, self._ffd_bit_off, self._ffd_n_bytes = byte_idx, bit_off, int(n_bytes)
            self.code_size = int(n_bytes)
        else:
            self.code_size = (int(self.bits.sum()) + 7) // 8
        self._dev = None

    def field_positions(self) -> np.ndarray:
        """Bit position of each dimension's field in the code row, MSB-first (0 for width 0)."""
        if self.packing == "ffd":
            pos = 8 * self._ffd_byte_idx + self._ffd_bit_off
        else:
            pos = self._offsets[:-1]
        return np.where(self.bits > 0, pos, 0).astype(np.int64)

    def _state(self) -> _native.RankAwareState:
        if self._dev is None:
            if self.code_size < 1:
                raise ValueError("the bit budget gives every dimension 0 bits: there is no code to write")
            self._dev = _native.rankaware_state(self.mu, self.V, self.cb, self.bits, self.field_positions(),
                                                self.code_size, _arrays.device())
        return self._dev

    # ------------------------------------------------------------- compress
    def compress(self, X):
        if self.V is None:
            raise RuntimeError("Quantizer must be fit before compress().")
        if not _arrays.is_tensor(X):
            X = np.asarray(X)
        if X.shape[1] != self.D:
            raise ValueError(f"compress() got D={X.shape[1]}, but fit() saw D={self.D}")
        st = self._state()
        if _arrays.is_tensor(X):
            dt = X.dtype if X.dtype in (torch.float32, torch.float64) else torch.float64
            return _native.rankaware_encode(_arrays.to_device(X, dt), st)
        dt = torch.float32 if X.dtype == np.float32 else torch.float64
        out = np.empty((X.shape[0], self.code_size), np.uint8)
        for s, e in _arrays.row_chunks(X.shape[0], self.D * 24, self._stage_bytes):
            out[s:e] = _arrays.to_host(_native.rankaware_encode(_arrays.to_device(X[s:e], dt), st))
        return out

    # ----------------------------------------------------------- decompress
    def decompress(self, codes):
        if self.V is None:
            raise RuntimeError("Quantizer must be fit before decompress().")
        st = self._state()
        if _arrays.is_tensor(codes):
            return _native.rankaware_decode(_arrays.to_device(codes, torch.uint8), st)
        codes = np.ascontiguousarray(codes, dtype=np.uint8)
        out = np.empty((codes.shape[0], self.D), np.float32)
        for s, e in _arrays.row_chunks(codes.shape[0], self.D * 24, self._stage_bytes):
            out[s:e] = _arrays.to_host(_native.rankaware_decode(_arrays.to_device(codes[s:e], torch.uint8), st))
        return out

    # --------------------------------------------------------------- search
    # RotatedSearch with centre mu and rotation V (orthogonal, x_hat = y_hat V^T + mu); the packed
    # fields are scanned against the per-dimension level tables
    def _fitted(self) -> bool:
        return self.V is not None

    def _scan(self, Qy, codes, k: int, mt: int, id_offset: int):
        return _native.rankaware_flat_search(Qy, codes, self._state(), k, mt, id_offset=id_offset)

    def to_state(self) -> dict:
        if self.V is None:
            raise ValueError("save(): the RankAwareQuantizer is not fitted")
        st = dict(qtype=np.array(self.qtype), avg_bits=np.array(self.avg_bits), alpha=np.array(self.alpha),
                  max_bits=np.array(self.max_bits), seed=np.array(self.seed), packing=np.array(self.packing),
                  mu=np.asarray(self.mu, dtype=np.float64), V=np.ascontiguousarray(self.V, dtype=np.float64),
                  var=np.asarray(self.var, dtype=np.float64), bits=np.asarray(self.bits, dtype=np.int64),
                  cb=np.concatenate(self.cb).astype(np.float64),
                  levels=np.concatenate(self._levels).astype(np.float64), Dg=np.asarray(self._Dg, dtype=np.float64))
        # written only when not the defaults: a gaussian quantizer's file keeps its bytes
        if self.codebook != "gaussian":
            st["codebook"] = np.array(self.codebook)
        if self.codebook_engine != "saq":
            st["codebook_engine"] = np.array(self.codebook_engine)
        return st

    @classmethod
    def from_state(cls, z) -> "RankAwareQuantizer":
        q = cls(avg_bits=float(z["avg_bits"]), alpha=float(z["alpha"]), max_bits=int(z["max_bits"]),
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
        return q

    def get_compression_ratio(self, X) -> float:
        return float(int(X.shape[1]) * 4 / self.code_size)
