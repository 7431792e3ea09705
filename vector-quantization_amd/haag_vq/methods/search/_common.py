"""What the search indexes share on the host: the metric map, the kernels' limits, the (nq, k)
result conventions and the ``.npz`` writer.  Private to this package; every index file takes
these from here and defines none of them itself."""

from __future__ import annotations

from pathlib import Path
from typing import Callable, Optional, Tuple

import numpy as np
import torch

from ... import _arrays, _native

METRIC = {"l2": _native.METRIC_L2, "ip": _native.METRIC_INNER_PRODUCT}
MAX_K = 256  # the wave-resident top-k of the scan kernels
MAX_CANDIDATES = MAX_K  # so a first stage proposes at most this many candidates per query
FLT_MAX = np.finfo(np.float32).max
DECODE_BYTES = 1 << 28  # sampled_mse: decoded rows per step


def check_metric(metric: str) -> int:
    """The library's code of 'l2' / 'ip'; anything else raises."""
    if metric not in METRIC:
        raise ValueError(f"metric must be 'l2' or 'ip', got {metric!r}")
    return METRIC[metric]


def empty_results(nq: int, k: int) -> Tuple[np.ndarray, np.ndarray]:
    """(ids uint32, dists f32) of shape (nq, max(k, 0)) for a search with nothing to compute."""
    k = max(int(k), 0)
    return np.empty((nq, k), dtype=np.uint32), np.empty((nq, k), dtype=np.float32)


def results_to_host(d: torch.Tensor, i: torch.Tensor, *, negate: bool = False,
                    sentinel: Optional[float] = None) -> Tuple[np.ndarray, np.ndarray]:
    """The (dists f32, ids int32 holding uint32) of a search as the caller's (ids uint32, dists f32)
    arrays.  ``negate`` flips the sign (kernel keys of 'ip' are negated inner products);
    ``sentinel`` is written where a slot could not be filled (id 0xFFFFFFFF), None keeps the
    kernel's value there."""
    ids = _arrays.to_host(i).view(np.uint32)
    dists = _arrays.to_host(d)
    if negate:
        dists = -dists
    if sentinel is not None:
        dists[ids == _native.NO_ID] = sentinel
    return ids, dists


def candidate_count(k: int, factor: int, n: int) -> int:
    """r, the candidates a first stage is asked for per query: min(k * factor, n)."""
    want = int(k) * factor
    if want > MAX_CANDIDATES:
        raise ValueError(f"k * refine_factor = {int(k)} * {factor} = {want}: the base searches keep at most "
                         f"{MAX_CANDIDATES} results")
    return min(want, n)


def save_npz(path: str | Path, **arrays) -> None:
    path = Path(path)
    path.parent.mkdir(parents=True, exist_ok=True)
    with open(path, "wb") as f:
        np.savez(f, **arrays)


def sampled_mse(reconstruct: Callable[[torch.Tensor], torch.Tensor], X, n: int, d: int,
                sample_ids: Optional[np.ndarray]) -> Optional[float]:
    """Mean over the sampled rows (all n when None; ids outside [0, n) dropped) of the per-row
    mean squared error of ``reconstruct(ids)`` against X, DECODE_BYTES of decoded rows at a time."""
    if sample_ids is None:
        sample_ids = np.arange(n)
    sample_ids = np.asarray(sample_ids, dtype=np.int64)
    sample_ids = sample_ids[(sample_ids >= 0) & (sample_ids < n)]
    if sample_ids.size == 0:
        return None
    total = 0.0
    step = max(1, DECODE_BYTES // (4 * d))
    for s in range(0, sample_ids.size, step):
        rows = sample_ids[s:s + step]
        xh = _arrays.to_host(reconstruct(torch.from_numpy(rows)))
        x = np.asarray(_arrays.to_host(X[rows]) if _arrays.is_tensor(X) else X[rows], dtype=np.float32)
        total += float(np.mean((x - xh) ** 2, axis=1).astype(np.float64).sum())
    return total / sample_ids.size
