"""Two-level LVQ (LVQ-B1xB2: the LVQ paper's second level, SVS' ``LVQ4x4`` / ``LVQ4x8``) on the MI355X.

The first level is ``LVQQuantizer(primary_bits)``, byte for byte.  The second level quantises
what the first left over to ``residual_bits`` (4 or 8) on the interval the first level's step
already fixes, ``[-delta / 2, delta / 2]``, so it stores no per-row constants: B1 + B2 bits
behave like one (B1 + B2)-bit code, and a search may scan the primary rows alone and re-rank
on both (``LVQ2Index``).  The arithmetic is fixed in ``include/mivq.h`` ("two-level LVQ"), one
float32 operation per step; the work runs in ``mivq_column_mean`` / ``mivq_lvq2_encode`` /
``mivq_lvq2_decode``.

``compress`` returns one (N, size1 + size2) uint8 array, the primary row (index stream, ``lo``,
``delta``) followed by the residual stream; ``split`` gives the two parts back as the arrays the
kernels take.  ``FlatQuantizedIndex`` serves this quantizer by its generic path (decode, then the
exact f32 search).
"""

from __future__ import annotations

from typing import Tuple

import numpy as np
import torch

from .. import _arrays, _native
from .base_quantizer import BaseQuantizer
from .lvq_quantization import LVQQuantizer


class TwoLevelLVQQuantizer(BaseQuantizer):
    def __init__(self, primary_bits: int = 4, residual_bits: int = 8) -> None:
        if not (1 <= primary_bits <= 8):
            raise ValueError(f"primary_bits must be in [1, 8], got {primary_bits}")
        if residual_bits not in (4, 8):
            raise ValueError(f"residual_bits must be 4 or 8, got {residual_bits}")
        self.primary_bits: int = primary_bits
        self.residual_bits: int = residual_bits
        self._lvq = LVQQuantizer(primary_bits)  # holds the mean, on the host and on the device

    @property
    def mu(self):
        return self._lvq.mu

    @mu.setter
    def mu(self, value) -> None:
        self._lvq.mu = value

    def fit(self, X) -> None:
        """mu = X.mean(axis=0) in float32, as LVQQuantizer.fit."""
        self._lvq.fit(X)

    def primary(self) -> LVQQuantizer:
        """The first level on its own: an LVQQuantizer(primary_bits) sharing this quantizer's mean."""
        return self._lvq

    def _mu_device(self) -> torch.Tensor:
        if self._lvq.mu is None:
            raise RuntimeError("TwoLevelLVQQuantizer.fit() must be called before compress/decompress.")
        return self._lvq._mu_device()

    def code_sizes(self, D: int) -> Tuple[int, int]:
        return _native.lvq2_code_sizes(D, self.primary_bits, self.residual_bits)

    def code_size(self, D: int) -> int:
        return sum(self.code_sizes(D))

    def _encode(self, Xd: torch.Tensor) -> torch.Tensor:
        c1, c2 = _native.lvq2_encode(Xd, self._mu_device(), self.primary_bits, self.residual_bits)
        return torch.cat((c1, c2), dim=1)

    def compress(self, X):
        self._mu_device()
        if _arrays.is_tensor(X):
            return self._encode(_arrays.to_device(X, torch.float32))
        X = np.asarray(X)
        n, d = X.shape
        out = np.empty((n, self.code_size(d)), dtype=np.uint8)
        for s, e in _arrays.row_chunks(n, d * 4):
            out[s:e] = _arrays.to_host(self._encode(_arrays.to_device(X[s:e], torch.float32)))
        return out

    def split(self, codes):
        """(codes1, codes2) of compress()'s rows, each contiguous: numpy in, numpy out; tensor in, tensor out."""
        mu = self.mu
        if mu is None:
            raise RuntimeError("TwoLevelLVQQuantizer.fit() must be called before split.")
        s1, s2 = self.code_sizes(mu.shape[0])
        if codes.ndim != 2 or codes.shape[1] != s1 + s2:
            raise ValueError(f"codes have shape {tuple(codes.shape)}, expected (n, {s1} + {s2})")
        if _arrays.is_tensor(codes):
            return codes[:, :s1].contiguous(), codes[:, s1:].contiguous()
        return np.ascontiguousarray(codes[:, :s1]), np.ascontiguousarray(codes[:, s1:])

    def _decode(self, cd: torch.Tensor) -> torch.Tensor:
        c1, c2 = self.split(cd)
        return _native.lvq2_decode(c1, c2, self._mu_device(), self.primary_bits, self.residual_bits)

    def decompress(self, codes):
        mu = self._mu_device()
        d = mu.numel()
        if _arrays.is_tensor(codes):
            return self._decode(_arrays.to_device(codes, torch.uint8))
        codes = np.ascontiguousarray(codes, dtype=np.uint8)
        n = codes.shape[0]
        out = np.empty((n, d), dtype=np.float32)
        for s, e in _arrays.row_chunks(n, d * 4):
            out[s:e] = _arrays.to_host(self._decode(_arrays.to_device(codes[s:e], torch.uint8)))
        return out

    def get_compression_ratio(self, X) -> float:
        """Original float32 bytes per vector over the code bytes per vector (both levels)."""
        D = X.shape[1]
        return D * 4 / self.code_size(D)
