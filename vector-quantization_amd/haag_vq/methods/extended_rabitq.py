"""Multi-bit ("Extended") RaBitQ on the MI355X.

Drop-in for the reference's ``ExtendedRaBitQuantizer``
(/root/reference/src/haag_vq/methods/extended_rabitq.py:47-204), the quantizer the registry's
``rabitq`` method builds (method_registry_saq.py:45-48).  Model state is computed exactly as the
reference does (global fp64 mean, QR of a seeded Gaussian matrix, 1-D Lloyd levels on an N(0,1)
sample — host-side, data independent except the mean); the per-row work runs on the device:
``mivq_extrabitq_normalize`` -> fp64 GEMM (o . P) -> ``mivq_extrabitq_quantize`` (searchsorted,
rescale factor t, MSB-first packing) and the mirror image for decode.  Code rows are
``ceil(D*B/8) + 8`` bytes (indices ++ f32 norm ++ f32 t) and decode row-independently.

Parity: fp64 throughout; the GEMM's summation order differs from numpy/OpenBLAS, so an index
can differ only where s lies within rounding distance of a level midpoint (each such index is
checked to be a midpoint tie against the reference's fixtures in
tests/test_pinning_gpu.py::test_extrabitq_mismatches_are_midpoint_ties), and the decoded
vectors agree to ~1e-12 relative.

``rotation="fht"`` replaces the dense P by the fast Hadamard rotation of include/mivq.h (four
rounds of seeded sign flips and a Walsh-Hadamard transform, as the published RaBitQ library
rotates): O(D log D) per row, 4 D bits of state in place of D x D fp64, and compress / decompress
as one fused kernel each (``mivq_extrabitq_encode_fht`` / ``_decode_fht``).  It is orthogonal, so
the code format, the code search and every index on top are the same; the codes differ from the
dense variant's, which stays the default and is what the registry builds.
"""

from __future__ import annotations

import numpy as np
import torch

from .. import _arrays, _native
from ._rotated import RotatedSearch
from .base_quantizer import BaseQuantizer


def _lloyd_1d_normal(num_levels: int, seed: int, n_samples: int = 200_000, max_iter: int = 100,
                     tol: float = 1e-7) -> np.ndarray:
    """Gaussian-optimal scalar codebook by 1-D Lloyd (extended_rabitq.py:6-44)."""
    rng = np.random.default_rng(seed)
    samples = rng.standard_normal(n_samples)
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
    return levels.astype(np.float64)


class ExtendedRaBitQuantizer(RotatedSearch, BaseQuantizer):
    qtype = "extrabitq"

    def __init__(self, num_bits: int = 4, seed: int = 0, rotation: str = "dense"):
        if num_bits < 1 or num_bits > 8:
            raise ValueError("num_bits must be in [1, 8]")
        if rotation not in ("dense", "fht"):
            raise ValueError(f"rotation must be 'dense' or 'fht', got {rotation!r}")
        self.rotation = rotation
        self.num_bits = int(num_bits)
        self.seed = int(seed)
        self.c: np.ndarray | None = None
        self.P: np.ndarray | None = None  # the rotation: (D, D) fp64, dense
        self.signs: np.ndarray | None = None  # or (rounds, D) u8 of 0 / 1, fht
        self.levels: np.ndarray | None = None
        self.D: int | None = None
        self._eps = 1e-12
        self._dev = None

    def fit(self, X) -> None:
        if _arrays.is_tensor(X):
            self.D = int(X.shape[1])
            self.c = _arrays.to_host(X.to(torch.float64).mean(dim=0))
        else:
            X = np.asarray(X)
            self.D = int(X.shape[1])
            self.c = X.mean(axis=0).astype(np.float64)
        rng = np.random.default_rng(self.seed)
        if self.rotation == "fht":
            self.signs = rng.integers(0, 2, size=(_native.FHT_ROUNDS, self.D)).astype(np.uint8)
        else:
            Q, _ = np.linalg.qr(rng.standard_normal((self.D, self.D)))
            self.P = Q.astype(np.float64)
        self.levels = _lloyd_1d_normal(2 ** self.num_bits, seed=self.seed)
        self._dev = None

    @property
    def _index_bytes(self) -> int:
        return (self.D * self.num_bits + 7) // 8

    @property
    def code_size(self) -> int:
        return self._index_bytes + 8

    def _state(self):
        if self._dev is None:
            dev = _arrays.device()
            rot = self.signs if self.rotation == "fht" else np.ascontiguousarray(self.P, np.float64)
            self._dev = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev)
                              for a in (self.c.astype(np.float64), rot, self.levels.astype(np.float64)))
        return self._dev

    def _encode(self, xt: torch.Tensor) -> torch.Tensor:
        c, R, lv = self._state()
        fn = _native.extrabitq_encode_fht if self.rotation == "fht" else _native.extrabitq_encode
        return fn(xt, c, R, lv, self.num_bits)

    def _decode(self, codes: torch.Tensor) -> torch.Tensor:
        c, R, lv = self._state()
        fn = _native.extrabitq_decode_fht if self.rotation == "fht" else _native.extrabitq_decode
        return fn(codes, c, R, lv, self.num_bits)

    def _rotate(self, Xc: torch.Tensor) -> torch.Tensor:
        if self.rotation == "fht":
            return _native.fht_rotate(Xc, self._state()[1], out=Xc)
        return super()._rotate(Xc)

    def compress(self, X):
        if not self._fitted():
            raise RuntimeError("Quantizer must be fit before compress().")
        if _arrays.is_tensor(X):
            if X.shape[1] != self.D:
                raise ValueError(f"compress() got D={X.shape[1]}, but fit() saw D={self.D}")
            xt = X if X.dtype in (torch.float32, torch.float64) else X.to(torch.float64)
            return self._encode(_arrays.to_device(xt, xt.dtype))
        X = np.asarray(X)
        if X.shape[1] != self.D:
            raise ValueError(f"compress() got D={X.shape[1]}, but fit() saw D={self.D}")
        dt = torch.float64 if X.dtype == np.float64 else torch.float32
        out = np.empty((X.shape[0], self.code_size), np.uint8)
        for s, e in _arrays.row_chunks(X.shape[0], self.D * 24):
            out[s:e] = _arrays.to_host(self._encode(_arrays.to_device(X[s:e], dt)))
        return out

    def decompress(self, codes):
        if not self._fitted():
            raise RuntimeError("Quantizer must be fit before decompress().")
        if _arrays.is_tensor(codes):
            return self._decode(_arrays.to_device(codes, torch.uint8))
        codes = np.ascontiguousarray(codes, dtype=np.uint8)
        out = np.empty((codes.shape[0], self.D), np.float32)
        for s, e in _arrays.row_chunks(codes.shape[0], self.D * 24):
            out[s:e] = _arrays.to_host(self._decode(_arrays.to_device(codes[s:e], torch.uint8)))
        return out

    # RotatedSearch with centre c and rotation P or the fht (orthogonal, x_hat = (o_hat P^T) nrm + c, so
    # y_hat = o_hat nrm); the bit fields are scanned against the shared level table and nrm / t
    def _fitted(self) -> bool:
        return (self.signs if self.rotation == "fht" else self.P) is not None

    def _scan(self, Qy, codes, k: int, mt: int, id_offset: int):
        return _native.extrabitq_flat_search(Qy, codes, self._state()[2], self.num_bits, k, mt, id_offset=id_offset)

    def to_state(self) -> dict:
        if not self._fitted():
            raise ValueError("save(): the ExtendedRaBitQuantizer is not fitted")
        head = dict(qtype=np.array(self.qtype), num_bits=np.array(self.num_bits), seed=np.array(self.seed),
                    D=np.array(self.D), c=np.asarray(self.c, dtype=np.float64))
        if self.rotation == "fht":  # a state without a rotation key is dense
            rot = dict(rotation=np.array("fht"), signs=np.ascontiguousarray(self.signs, dtype=np.uint8))
        else:
            rot = dict(P=np.ascontiguousarray(self.P, dtype=np.float64))
        return dict(**head, **rot, levels=np.asarray(self.levels, dtype=np.float64))

    @classmethod
    def from_state(cls, z) -> "ExtendedRaBitQuantizer":
        q = cls(num_bits=int(z["num_bits"]), seed=int(z["seed"]),
                rotation=str(z["rotation"]) if "rotation" in z else "dense")
        q.D = int(z["D"])
        q.c, q.levels = (np.array(z[nm], dtype=np.float64) for nm in ("c", "levels"))
        if q.rotation == "fht":
            q.signs = np.array(z["signs"], dtype=np.uint8)
            rot_ok = q.signs.ndim == 2 and q.signs.shape[1] == q.D and 1 <= q.signs.shape[0] <= 8 and q.signs.max() <= 1
        else:
            q.P = np.array(z["P"], dtype=np.float64)
            rot_ok = q.P.shape == (q.D, q.D)
        if q.c.shape != (q.D,) or not rot_ok or q.levels.shape != (2 ** q.num_bits,):
            raise ValueError("load(): inconsistent Extended RaBitQ quantizer state")
        return q

    def get_compression_ratio(self, X) -> float:
        return float(int(X.shape[1]) * 4 / self.code_size)
