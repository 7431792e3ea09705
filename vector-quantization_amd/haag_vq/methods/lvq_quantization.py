"""Locally-adaptive vector quantization (LVQ, single level, 1..8 bits) on the MI355X.

Drop-in for the reference's ``LVQQuantizer``
(/root/reference/src/haag_vq/methods/lvq_quantization.py:23-151): ``fit`` learns the global
mean, ``compress`` quantizes every residual row on its own ``[min, max]`` range to B-bit
indices and packs them MSB-first, followed by the row's ``lo`` and ``delta`` as float32
(``code_size = ceil(D * B / 8) + 8``), ``decompress`` is row-independent.  Means, codes and
reconstructions are bit-identical to numpy's float32 arithmetic on float32 inputs (other input
dtypes are converted to float32 first, as ``FlatQuantizedIndex.fit`` does).  The work runs in
``mivq_column_mean`` / ``mivq_lvq_encode`` / ``mivq_lvq_decode``; ``FlatQuantizedIndex``
searches the codes as they are (``mivq_lvq_flat_search``).
"""

from __future__ import annotations

import numpy as np
import torch

from .. import _arrays, _native
from .base_quantizer import BaseQuantizer


class LVQQuantizer(BaseQuantizer):
    qtype = "lvq"
    code_kind = "lvq"

    def __init__(self, num_bits: int = 8) -> None:
        if not (1 <= num_bits <= 8):
            raise ValueError(f"num_bits must be in [1, 8], got {num_bits}")
        self.num_bits: int = num_bits
        self._mu = None      # global mean, numpy float32 (D,)
        self._mu_dev = None  # the same on the device

    @property
    def mu(self):
        return self._mu

    @mu.setter
    def mu(self, value) -> None:
        self._mu = None if value is None else np.ascontiguousarray(value, dtype=np.float32)
        self._mu_dev = None

    def fit(self, X) -> None:
        """mu = X.mean(axis=0) in float32 (column sums in ascending row order, as numpy)."""
        self.mu = _arrays.to_host(_native.column_mean(_arrays.to_device(X, torch.float32)))

    def _mu_device(self) -> torch.Tensor:
        if self._mu is None:
            raise RuntimeError("LVQQuantizer.fit() must be called before compress/decompress.")
        if self._mu_dev is None or self._mu_dev.device != _arrays.device():
            self._mu_dev = _arrays.to_device(self._mu, torch.float32)
        return self._mu_dev

    def code_size(self, D: int) -> int:
        return _native.lvq_code_size(D, self.num_bits)

    def compress(self, X):
        mu = self._mu_device()
        if _arrays.is_tensor(X):
            return _native.lvq_encode(_arrays.to_device(X, torch.float32), mu, self.num_bits)
        X = np.asarray(X)
        n, d = X.shape
        out = np.empty((n, self.code_size(d)), dtype=np.uint8)
        for s, e in _arrays.row_chunks(n, d * 4):
            out[s:e] = _arrays.to_host(_native.lvq_encode(_arrays.to_device(X[s:e], torch.float32), mu, self.num_bits))
        return out

    def decompress(self, codes):
        mu = self._mu_device()
        d = mu.numel()
        if _arrays.is_tensor(codes):
            return _native.lvq_decode(_arrays.to_device(codes, torch.uint8), mu, self.num_bits)
        codes = np.ascontiguousarray(codes, dtype=np.uint8)
        n = codes.shape[0]
        out = np.empty((n, d), dtype=np.float32)
        for s, e in _arrays.row_chunks(n, d * 4):
            out[s:e] = _arrays.to_host(_native.lvq_decode(_arrays.to_device(codes[s:e], torch.uint8), mu, self.num_bits))
        return out

    def flat_keys(self, codes_dev, Q_dev, k: int, mt: int, id_offset: int = 0):  # = decode + search, bit for bit
        if self._mu is None:
            return super().flat_keys(codes_dev, Q_dev, k, mt, id_offset)
        return _native.lvq_flat_search(Q_dev, _arrays.to_device(codes_dev, torch.uint8).contiguous(), self._mu_device(),
                                       self.num_bits, k, mt, id_offset=id_offset)

    def code_params(self) -> tuple:  # (mu,)
        return (self._mu_device(),)

    def to_state(self) -> dict:
        return dict(qtype=np.array(self.qtype), num_bits=np.array(self.num_bits), mu=np.asarray(self.mu, dtype=np.float32))

    @classmethod
    def from_state(cls, z) -> "LVQQuantizer":
        q = cls(num_bits=int(z["num_bits"]))
        q.mu = np.array(z["mu"])
        return q

    def get_compression_ratio(self, X) -> float:
        """Original float32 bytes per vector over the code bytes per vector."""
        D = X.shape[1]
        return D * 4 / self.code_size(D)
