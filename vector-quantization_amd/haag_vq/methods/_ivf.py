"""Inverted-file (IVF) machinery on the MI355X: coarse k-means, list assignment, IVF-PQ.

Replaces what faiss ``IndexIVFPQ`` does inside FaissIvfPqIndex
(/root/reference/src/haag_vq/methods/search/faiss_ivfpq_index.py:46-76) and the IVF build
of benchmarks/ivf_benchmark.py:170-204:

* ``train_coarse``  the coarse quantizer's k-means (faiss' IVF clustering shape: a random
  sample of at most 256 points per centroid, seed 1234, centroids initialised from the
  sample, 10 Lloyd iterations, empty clusters re-seeded by splitting).  Assignment is the
  exact pairwise-distance kernel + a per-row argmin; the update is the ascending-row
  centroid sum over a stable bucket sort, so a fit is bit-reproducible.
* ``IvfPq``  residual product quantization (faiss' ``by_residual``): PQ codebooks trained on
  residuals x - coarse[list(x)], codes from the bit-exact PQ encode of the residuals, lists
  in bucket order, and the per-vector L2 term tau_i that turns faiss' per-list
  precomputed table into one number per code, so a query needs only its own M x ksub LUT:
      ||q - c_l - r_i||^2 = ||q - c_l||^2 + tau_i - 2 q.r_i,  tau_i = ||r_i||^2 + 2 c_l.r_i.
  IP (IndexFlatIP quantizer): score = q.c_l + q.r_i, ranked as its negation.
* ``IvfRaBitQ``  RaBitQ-1 codes of x - coarse[list(x)] (faiss ``IVF{nlist},RaBitQ``): the encode
  whose centre is the row's list centroid, lists in bucket order, and the estimator search over
  the probed lists with the query residual re-quantised per (query, list) pair.
* ``IvfCodes``  per-list SQ / LVQ codes of x - coarse[list(x)] (the reference's IvfQuantizedIndex:
  one quantizer per list, fitted on the list's residuals): the parameters of all lists as
  (nlist, d) tensors, lists in bucket order, and the exact search over the probed lists.
* ``IvfListPq``  one PQ codebook per list, trained on the list's residuals (the reference's
  IvfQuantizedIndex around a ProductQuantizer, run_benchmarks' ``pq_ivf``): (nlist, M, ksub, dsub)
  codebooks, lists in bucket order, and the ADC search whose lookup table belongs to a (query,
  probed list) pair.

faiss itself is absent here, so coarse centroids, codebooks and results are not claimed to
equal faiss'; the arithmetic is the canonical one of include/mivq.h and oracle/.
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch

from .. import _native
from ._kmeans import EPS, train_pq

_MAT_BYTES = 1 << 30  # per-chunk (rows x K) distance matrix budget


def _rows_per_chunk(K: int) -> int:
    return max(1, _MAT_BYTES // (4 * max(1, K)))


def assign(X: torch.Tensor, C: torch.Tensor, metric: int = _native.METRIC_L2) -> Tuple[torch.Tensor, torch.Tensor]:
    """Nearest coarse centroid of every row: (dist f32 (n,), list int32 (n,))."""
    n = X.shape[0]
    K = C.shape[0]
    dd = torch.empty(n, dtype=torch.float32, device=X.device)
    ll = torch.empty(n, dtype=torch.int32, device=X.device)
    step = _rows_per_chunk(K)
    buf = None
    for s in range(0, n, step):
        e = min(n, s + step)
        if buf is None or buf.shape[0] != e - s:
            buf = torch.empty((e - s, K), dtype=torch.float32, device=X.device)
        _native.pairwise_distances(X[s:e], C, metric, out=buf)
        d1, i1 = _native.topk_rows(buf, 1)
        dd[s:e] = d1[:, 0]
        ll[s:e] = i1[:, 0]
    return dd, ll


def _split_empty(C: np.ndarray, cnt: np.ndarray, rng: np.random.Generator, n: int) -> int:
    """faiss-style split of empty clusters of a (K, d) codebook, in place."""
    K, d = C.shape
    cnt = cnt.astype(np.float64)
    nsplit = 0
    sign = np.where(np.arange(d) % 2 == 0, 1.0, -1.0).astype(np.float32)
    for ci in range(K):
        if cnt[ci] != 0:
            continue
        cj = 0
        denom = max(1.0, float(n - K))
        for _ in range(64 * K):
            if rng.random() < (cnt[cj] - 1.0) / denom:
                break
            cj = (cj + 1) % K
        else:
            cj = int(np.argmax(cnt))
        C[ci] = C[cj]
        C[ci] *= (1.0 + EPS * sign).astype(np.float32)
        C[cj] *= (1.0 - EPS * sign).astype(np.float32)
        cnt[ci] = np.floor(cnt[cj] / 2)
        cnt[cj] -= cnt[ci]
        nsplit += 1
    return nsplit


def train_coarse(X: torch.Tensor, K: int, niter: int = 10, seed: int = 1234, max_points_per_centroid: int = 256,
                 metric: int = _native.METRIC_L2) -> torch.Tensor:
    """(K, d) f32 coarse centroids by Lloyd iterations on a sample of device rows X."""
    n, d = X.shape
    if n < K:
        raise RuntimeError(f"Number of training points ({n}) should be at least as large as number of clusters ({K})")
    rng = np.random.default_rng(seed)
    max_n = max_points_per_centroid * K
    if n > max_n:
        sel = np.sort(rng.permutation(n)[:max_n])
        Xt = X[torch.from_numpy(sel).to(X.device)].contiguous()
    else:
        Xt = X.contiguous()
    nt = Xt.shape[0]
    pick = np.sort(rng.permutation(nt)[:K])
    C = Xt[torch.from_numpy(pick).to(X.device)].contiguous().clone()
    counts = torch.empty(K, dtype=torch.int32, device=X.device)
    for _ in range(niter):
        _, a = assign(Xt, C, metric)
        offsets, order = _native.bucket_sort(a, K)
        _native.centroid_update(Xt, offsets, order, C, counts)
        cnt = counts.cpu().numpy()
        if (cnt == 0).any():
            Ch = C.cpu().numpy()
            _split_empty(Ch, cnt, rng, nt)
            C = torch.from_numpy(Ch).to(X.device).contiguous()
    return C


@dataclass
class IvfLists:
    """Inverted lists in bucket order (device tensors)."""
    offsets: torch.Tensor     # (K+1,) int64
    codes: torch.Tensor       # (N, M) uint8, one byte per sub-code (IvfRaBitQ: RaBitQ-1 code rows)
    ids: torch.Tensor         # (N,) int32 holding uint32 ids
    tau: Optional[torch.Tensor]  # (N,) f32, L2 only

    def to_arrays(self) -> dict:
        """The lists as the numpy arrays an index file holds (``tau`` only where there is one)."""
        arrays = {name: getattr(self, name).detach().cpu().numpy() for name in ("offsets", "codes", "ids")}
        if self.tau is not None:
            arrays["tau"] = self.tau.detach().cpu().numpy()
        return arrays

    @classmethod
    def from_arrays(cls, z, device) -> "IvfLists":
        """Inverse of to_arrays (z: a mapping of numpy arrays, e.g. an open .npz); 2-byte codes are
        the int16 rows of 16-bit SQ, every other code array is bytes."""
        def put(a, dtype):
            return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(device)

        codes = np.asarray(z["codes"])
        return cls(offsets=put(z["offsets"], np.int64),
                   codes=put(codes, np.int16 if codes.dtype.itemsize == 2 else np.uint8),
                   ids=put(z["ids"], np.int32), tau=put(z["tau"], np.float32) if "tau" in z else None)


class _IvfEngine:
    """What the engines share: the coarse quantizer, the assignment of rows, the probe selection
    and the lists in bucket order."""

    def __init__(self, d: int, K: int, metric: int) -> None:
        self.d, self.K, self.metric = d, K, metric
        self.coarse: Optional[torch.Tensor] = None
        self.lists: Optional[IvfLists] = None
        self.ntotal = 0

    def train(self, X: torch.Tensor, coarse_iters: int = 10, seed: int = 1234) -> None:
        self.coarse = train_coarse(X, self.K, niter=coarse_iters, seed=seed, metric=self.metric)

    def _assign(self, X: torch.Tensor) -> torch.Tensor:
        """The list of every row, int32 (n,)."""
        return assign(X, self.coarse, self.metric)[1]

    def _probe(self, Q: torch.Tensor, nprobe: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """The nprobe nearest lists of every query: (coarse dists f32, lists int32), both (nq, nprobe)."""
        nprobe = max(1, min(int(nprobe), self.K))
        if nprobe > 256:
            raise ValueError(f"nprobe={nprobe}: the probe selection (mivq_topk_rows) supports at most 256 lists")
        return _native.topk_rows(_native.pairwise_distances(Q, self.coarse, self.metric), nprobe)

    def probes(self, Q: torch.Tensor, nprobe: int) -> torch.Tensor:
        """The lists of _probe alone, int32 (nq, nprobe)."""
        return self._probe(Q, nprobe)[1]

    def _list_of(self) -> torch.Tensor:
        """The list of every stored row in bucket order, from the offsets."""
        off = self.lists.offsets
        return torch.repeat_interleave(torch.arange(self.K, dtype=torch.int32, device=off.device), off[1:] - off[:-1])

    @staticmethod
    def _gather(rows: torch.Tensor, order: torch.Tensor) -> torch.Tensor:
        """rows[order]; mivq_gather_rows moves rows of whole 4-byte words."""
        rows = rows.contiguous()
        if rows[:1].numel() * rows.element_size() % 4 == 0:
            return _native.gather_rows(rows, order)
        return rows[order.long()].contiguous()

    def _append(self, a: torch.Tensor, codes: torch.Tensor, tau: Optional[torch.Tensor] = None) -> None:
        """Append rows with lists a (ids continue from ntotal); the lists are rebuilt in bucket order."""
        n = a.shape[0]
        ids = torch.arange(self.ntotal, self.ntotal + n, dtype=torch.int64, device=a.device).to(torch.int32)
        if self.lists is not None and self.ntotal > 0:
            old = self.lists
            a = torch.cat([self._list_of(), a])
            codes = torch.cat([old.codes, codes])
            ids = torch.cat([old.ids, ids])
            if tau is not None:
                tau = torch.cat([old.tau, tau])
        offsets, order = _native.bucket_sort(a.contiguous(), self.K)
        self.lists = IvfLists(offsets=offsets, codes=self._gather(codes, order), ids=self._gather(ids, order),
                              tau=None if tau is None else self._gather(tau, order))
        self.ntotal += n


class IvfPq(_IvfEngine):
    """IVF with residual PQ (device-resident); the engine behind FaissIvfPqIndex."""

    def __init__(self, d: int, K: int, M: int, nbits: int = 8, metric: int = _native.METRIC_L2) -> None:
        if d % M != 0:
            raise AssertionError("D must be divisible by M (number of subquantizers)")
        super().__init__(d, K, metric)
        self.M, self.nbits = M, nbits
        self.pq: Optional[torch.Tensor] = None    # (M, ksub, dsub)
        self.prep: Optional[torch.Tensor] = None

    def train(self, X: torch.Tensor, coarse_iters: int = 10, pq_iters: int = 25, seed: int = 1234) -> None:
        super().train(X, coarse_iters, seed)
        ksub = 1 << self.nbits
        rng = np.random.default_rng(seed + 1)
        n = X.shape[0]
        cap = 256 * ksub
        Xs = X if n <= cap else X[torch.from_numpy(np.sort(rng.permutation(n)[:cap])).to(X.device)].contiguous()
        R = _native.ivf_residuals(Xs, self.coarse, self._assign(Xs))
        self.pq = train_pq(R, self.M, self.nbits, niter=pq_iters, seed=seed)
        self.prep = _native.pq_prepare(self.pq, self.nbits)

    def add(self, X: torch.Tensor) -> None:
        """Append rows (ids continue from ntotal); lists are rebuilt in bucket order."""
        n = X.shape[0]
        a = self._assign(X)
        codes = torch.empty((n, self.M), dtype=torch.uint8, device=X.device)
        tau = torch.empty(n, dtype=torch.float32, device=X.device) if self.metric == _native.METRIC_L2 else None
        step = max(1, (1 << 30) // (4 * self.d))  # the residual buffer
        for s in range(0, n, step):
            e = min(n, s + step)
            c = _native.pq_encode(_native.ivf_residuals(X[s:e], self.coarse, a[s:e]), self.pq, self.prep, self.nbits)
            codes[s:e] = c if self.nbits == 8 else _native.pq_unpack(c, self.M, self.nbits)
            if tau is not None:
                tau[s:e] = _native.ivfpq_terms(codes[s:e], self.pq, self.prep, self.coarse, a[s:e], self.nbits)
        self._append(a, codes, tau)

    def search(self, Q: torch.Tensor, k: int, nprobe: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """(dists f32 (nq, k), ids int32 (nq, k)); L2 ascending, IP as negated scores."""
        pd, pl = self._probe(Q, nprobe)
        lut = _native.adc_lut(Q, self.pq, self.nbits, _native.METRIC_INNER_PRODUCT)
        L = self.lists
        return _native.ivfpq_search(lut, pd, pl, L.offsets, L.codes, L.ids, L.tau, self.metric, k, self.nbits)


class IvfRaBitQ(_IvfEngine):
    """IVF over RaBitQ-1 codes (device-resident); the engine behind RaBitQIVFIndex."""

    def __init__(self, d: int, K: int, metric: int = _native.METRIC_L2) -> None:
        super().__init__(d, K, metric)

    def add(self, X: torch.Tensor) -> None:
        """Append rows (ids continue from ntotal); lists are rebuilt in bucket order."""
        a = self._assign(X)
        self._append(a, _native.ivf_rabitq_encode(X, self.coarse, a, self.metric))

    def search(self, Q: torch.Tensor, k: int, nprobe: int, qb: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """(keys f32 (nq, k), ids int32 (nq, k)); L2 estimates ascending, IP as negated estimates."""
        L = self.lists
        return _native.ivf_rabitq_search(Q, self.coarse, self.probes(Q, nprobe), L.offsets, L.codes, L.ids, qb,
                                         self.metric, k)


class _IvfRowEngine(_IvfEngine):
    """An engine whose lists are laid out once, by ``fit_lists`` (ids 0 .. N - 1), and that finds a
    row by its id: ``pos[id]`` is the bucket position of row ``id``, ``list_of[p]`` the list of the
    row at bucket position ``p``."""

    def __init__(self, d: int, K: int, metric: int) -> None:
        super().__init__(d, K, metric)
        self.pos: Optional[torch.Tensor] = None
        self.list_of: Optional[torch.Tensor] = None

    def _set_lists(self, offsets: torch.Tensor, codes: torch.Tensor, order: torch.Tensor) -> None:
        """The tail of fit_lists: codes are in bucket order, order[p] is the row at position p."""
        self.lists = IvfLists(offsets=offsets, codes=codes, ids=order.clone(), tau=None)
        self.ntotal = order.shape[0]
        self._index_rows()

    def _index_rows(self) -> None:
        ids = self.lists.ids.long() & 0xFFFFFFFF
        self.pos = torch.empty(ids.numel(), dtype=torch.int64, device=ids.device)
        self.pos[ids] = torch.arange(ids.numel(), dtype=torch.int64, device=ids.device)
        self.list_of = self._list_of().contiguous()

    def _rows(self, rows: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """(code rows, lists) of the rows with these ids."""
        p = self.pos[rows.to(self.pos.device).long()]
        return self.lists.codes[p].contiguous(), self.list_of[p].contiguous()


class IvfCodes(_IvfRowEngine):
    """IVF over per-list SQ ('sq': 4 / 8 / 16 bits) or LVQ ('lvq': 1..8 bits) codes of the residuals
    (device-resident); the engine behind IvfQuantizedIndex.  ``params`` are (nlist, d) f32 tensors:
    (lo, den) for SQ, (mu,) for LVQ."""

    def __init__(self, d: int, K: int, kind: str, nbits: int, metric: int = _native.METRIC_L2) -> None:
        if kind not in ("sq", "lvq"):
            raise ValueError(f"kind must be 'sq' or 'lvq', got {kind!r}")
        super().__init__(d, K, metric)
        self.kind, self.nbits = kind, int(nbits)
        self.params: Optional[Tuple[torch.Tensor, ...]] = None

    def _lvq_means(self, X: torch.Tensor, a: torch.Tensor, offsets: torch.Tensor, order: torch.Tensor) -> torch.Tensor:
        """mu (K, d): the ascending-row f32 mean of every list's residuals (0 for an empty list):
        ivf_residuals + centroid_update on a zeroed output, whole lists at a time."""
        n, d = X.shape
        mu = torch.zeros((self.K, d), dtype=torch.float32, device=X.device)
        counts = torch.empty(self.K, dtype=torch.int32, device=X.device)
        budget = max(1, _MAT_BYTES // (4 * d))
        if n <= budget:
            _native.centroid_update(_native.ivf_residuals(X, self.coarse, a), offsets, order, mu, counts)
            return mu
        off = offsets.cpu().numpy()
        l0 = 0
        while l0 < self.K:
            l1 = l0 + 1
            while l1 < self.K and off[l1 + 1] - off[l0] <= budget:
                l1 += 1
            rows = order[int(off[l0]):int(off[l1])].contiguous()
            if rows.numel():
                R = _native.ivf_residuals(_native.gather_rows(X, rows), self.coarse, a[rows.long()].contiguous())
                _native.centroid_update(R, (offsets[l0:l1 + 1] - offsets[l0]).contiguous(),
                                        torch.arange(rows.numel(), dtype=torch.int32, device=X.device),
                                        mu[l0:l1], counts[l0:l1])
            l0 = l1
        return mu

    def _fit_params(self, X: torch.Tensor, a: torch.Tensor, offsets: torch.Tensor, order: torch.Tensor):
        if self.kind == "sq":
            return _native.ivf_sq_fit(X, self.coarse, offsets, order)
        return (self._lvq_means(X, a, offsets, order),)

    def _encode(self, X: torch.Tensor, a: torch.Tensor) -> torch.Tensor:
        if self.kind == "sq":
            lo, den = self.params
            return _native.ivf_sq_encode(X, self.coarse, a, lo, den, self.nbits)
        return _native.ivf_lvq_encode(X, self.coarse, a, self.params[0], self.nbits)

    def fit_lists(self, X: torch.Tensor) -> None:
        """Assign every row, fit each list's quantizer on its residuals, encode, and lay the
        lists out in bucket order (ids 0 .. N - 1)."""
        a = self._assign(X)
        offsets, order = _native.bucket_sort(a, self.K)
        self.params = tuple(self._fit_params(X, a, offsets, order))
        self._set_lists(offsets, self._gather(self._encode(X, a), order), order)

    def reconstruct(self, rows: torch.Tensor) -> torch.Tensor:
        """x^ (len(rows), d) f32 of the rows with these ids, through the decode entry points."""
        codes, a = self._rows(rows)
        if self.kind == "sq":
            lo, den = self.params
            return _native.ivf_sq_decode(codes, self.coarse, a, lo, den, self.nbits)
        return _native.ivf_lvq_decode(codes, self.coarse, a, self.params[0], self.nbits)

    def search(self, Q: torch.Tensor, k: int, nprobe: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """(keys f32 (nq, k), ids int32 (nq, k)); L2 ascending, IP as negated inner products."""
        L = self.lists
        return _native.ivf_code_search(self.kind, Q, self.coarse, self.probes(Q, nprobe), L.offsets, L.codes,
                                       L.ids, self.params, self.nbits, self.metric, k)


def short_list_error(counts: np.ndarray, nbits: int) -> Optional[str]:
    """The message for lists that hold rows, but fewer than the 2^nbits a codebook is trained on
    (None when there is none); faiss' wording, as the reference's per-list fit raises it."""
    ksub = 1 << nbits
    short = np.flatnonzero((counts > 0) & (counts < ksub))
    if short.size == 0:
        return None
    l = int(short[0])
    return (f"Number of training points ({int(counts[l])}) should be at least as large as number of clusters ({ksub}): "
            f"list {l} of {counts.size} ({short.size} non-empty list{'s hold' if short.size > 1 else ' holds'} fewer than "
            f"{ksub} rows); use a smaller K or B")


class IvfListPq(_IvfRowEngine):
    """IVF with one PQ codebook per list, fitted on the list's residuals (device-resident); the
    engine behind IvfListPqIndex.  ``codebooks`` is (K, M, ksub, dsub) f32 (zeros for an empty
    list), the lists hold (N, M) uint8 codes in bucket order.  ``fit_lists`` trains the K codebooks
    one after the other (a host loop)."""

    def __init__(self, d: int, K: int, M: int, nbits: int = 8, metric: int = _native.METRIC_L2, niter: int = 25,
                 seed: int = 1234) -> None:
        if d % M != 0:
            raise AssertionError("D must be divisible by M (number of subquantizers)")
        super().__init__(d, K, metric)
        self.M, self.nbits, self.niter, self.seed = int(M), int(nbits), int(niter), int(seed)
        self.codebooks: Optional[torch.Tensor] = None

    def fit_lists(self, X: torch.Tensor) -> None:
        """Assign every row, train each non-empty list's codebook on its residuals (ascending
        row order), encode them, and lay the lists out in bucket order (ids 0 .. N - 1).  A
        non-empty list with fewer than 2^nbits rows raises before any training."""
        a = self._assign(X)
        offsets, order = _native.bucket_sort(a, self.K)
        off = offsets.cpu().numpy()
        msg = short_list_error(np.diff(off), self.nbits)
        if msg is not None:
            raise RuntimeError(msg)
        n = X.shape[0]
        ksub = 1 << self.nbits
        cb = torch.zeros((self.K, self.M, ksub, self.d // self.M), dtype=torch.float32, device=X.device)
        codes = torch.empty((n, self.M), dtype=torch.uint8, device=X.device)
        for l in range(self.K):
            b, e = int(off[l]), int(off[l + 1])
            if e == b:
                continue
            rows = order[b:e].contiguous()
            R = _native.ivf_residuals(_native.gather_rows(X, rows), self.coarse, a[rows.long()].contiguous())
            C = train_pq(R, self.M, self.nbits, niter=self.niter, seed=self.seed)
            cb[l] = C
            c = _native.pq_encode(R, C, _native.pq_prepare(C, self.nbits), self.nbits)
            codes[b:e] = c if self.nbits == 8 else _native.pq_unpack(c, self.M, self.nbits)
        self.codebooks = cb
        self._set_lists(offsets, codes, order)

    def reconstruct(self, rows: torch.Tensor) -> torch.Tensor:
        """x^ (len(rows), d) f32 of the rows with these ids: pq_decode with the list's codebook + centroid."""
        codes, a = self._rows(rows)
        return _native.ivf_listpq_decode(codes, self.codebooks, self.coarse, a, self.nbits)

    def search(self, Q: torch.Tensor, k: int, nprobe: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """(keys f32 (nq, k), ids int32 (nq, k)); L2 ascending, IP as negated inner products."""
        L = self.lists
        return _native.ivf_listpq_search(Q, self.codebooks, self.coarse, self.probes(Q, nprobe), L.offsets, L.codes,
                                         L.ids, self.nbits, self.metric, k)
