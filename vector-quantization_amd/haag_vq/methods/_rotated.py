"""Search in the rotated domain, for the quantizers that code ``(x - centre) R`` with an orthogonal
``R``: x_hat = y_hat R^T + centre, so ||q - x_hat||^2 = ||(q - centre) R - y_hat||^2 and
<q, x_hat> = <q R, y_hat> + <q, centre>.  Only the queries are rotated; no row is decoded.

A quantizer supplies ``D``, ``_fitted()``, a ``_state()`` that begins with (centre (D,), R (D, D))
in fp64 on the device, and ``_scan(Qy, codes, k, mt, id_offset)``: its ``mivq_*_flat_search`` of
rotated queries over packed codes (kernel keys ascending, IP negated and without <q, centre>).
"""

from __future__ import annotations

import numpy as np
import torch

from .. import _arrays, _native


class RotatedSearch:
    def _queries(self, Q) -> torch.Tensor:
        if not self._fitted():
            raise RuntimeError("Quantizer must be fit before a search.")
        if not _arrays.is_tensor(Q):
            Q = np.ascontiguousarray(Q)
        if len(Q.shape) != 2 or Q.shape[1] != self.D:
            raise ValueError(f"queries must be (nq, {self.D}), got shape {tuple(Q.shape)}")
        dt = torch.float64 if str(Q.dtype).endswith("float64") else torch.float32
        return _arrays.to_device(Q, dt).contiguous()

    def rotate_queries(self, Q, metric: str = "l2") -> torch.Tensor:
        """The queries in the rotated domain, (nq, D) f32 on the device: ``(Q - centre) R`` for L2
        and ``Q R`` for IP, computed in fp64 and rounded once."""
        if metric not in ("l2", "ip"):
            raise ValueError(f"metric must be 'l2' or 'ip', got {metric!r}")
        Qd = self._queries(Q)
        c, R = self._state()[:2]
        return _native.gemm_f64(_native.rankaware_center(Qd, c if metric == "l2" else torch.zeros_like(c)), R,
                                False).to(torch.float32)

    def search_codes(self, codes, Q, k: int, metric: str = "l2", id_offset: int = 0):
        """Top-k of Q over ``codes`` without decoding them (``_scan``, k <= 256).  Returns device
        tensors (dists f32 (nq, k), ids int32 (nq, k) holding uint32 ids): squared L2 distances
        ascending, or inner products descending (the kernel's key negated plus f32(<q, centre>),
        the product in fp64, one f32 add per query)."""
        Qy = self.rotate_queries(Q, metric)
        cd = codes if _arrays.is_tensor(codes) else torch.from_numpy(np.ascontiguousarray(codes, dtype=np.uint8))
        cd = _arrays.to_device(cd, torch.uint8).contiguous()
        mt = _native.METRIC_L2 if metric == "l2" else _native.METRIC_INNER_PRODUCT
        d, i = self._scan(Qy, cd, int(k), mt, int(id_offset))
        if metric == "ip":
            qc = (self._queries(Q).to(torch.float64) @ self._state()[0]).to(torch.float32)
            d = -d + qc[:, None]
        return d, i
