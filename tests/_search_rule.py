"""Search fixtures: the cases, their inputs, and the acceptance rule of tests/test_search_golden.py.

Shared by the fixture generator (tests/golden/make_golden.py `search`, which runs the reference's
FlatQuantizedIndex) and by the tests, so both build the same inputs and judge a result the same
way.  Everything here is numpy on the host; nothing of the reference is imported.

The rule.  For one query every row r of the database gets, in fp64 from the reconstruction x_hat,

    key[r] = sum (q - x_hat_r)^2          (L2)        -q . x_hat_r            (IP)
    mag[r] = key[r]                       (L2)        sum |q_t x_hat_r,t|     (IP)
    e[r]   = (D + M + 2) 2^-24 mag[r]     (M = number of sub-quantizers, 0 for non-PQ)

e[r] bounds the error of any fp32 evaluation of that sum in any order: one rounding of every
term (two for (q - x)^2), at most D - 1 (ADC: M - 1 on top of the dsub - 1 of a table entry)
roundings of partial sums each no larger than mag, all of relative size 2^-24 -- which also
covers scipy's fp64 cdist cast to fp32 and an fp32 BLAS product.  OPQ adds what the rotation
of the query contributes (`opq_terms`).  With r_j the row at position j of the fp64 order by
(key, id), position j is *settled* if every other row o has |key[o] - key[r_j]| > e[o] +
e[r_j] -- no correct fp32 implementation can put another row there -- and *open* otherwise.
`check` accepts a result (ids, dists) when

 1. ids[j] == r_j at every settled position,
 2. |key[ids[j]] - key[r_j]| <= 2 max_r e[r] at every open position,
 3. a row's ids have no duplicates,
 4. |dist[j] - key[ids[j]]| <= e[ids[j]] (IP: the returned score is +inner product),
 5. the returned distances do not decrease along a row (IP scores do not increase),
 6. shape (nq, min(k, N)), ids uint32, dists float32,
 7. (tie_order, the index's documented tie-break) neighbours that return the same distance for
    rows with the same fp64 key come in ascending id order.
"""

from __future__ import annotations

import hashlib

import numpy as np

U24 = 2.0 ** -24
OPEN_CAP = 0.10      # share of open positions a fixture case may have
OPQ_ROT_TOL = 1e-5   # tests/test_opq_gpu.py TOL: |y_t - y64_t| <= TOL ||q|| ||A_t||

# name -> kind, bits (SQ / ERQ) or (M, B) (PQ), N, D, nq, k, seed
CASES = {
    "sq4_w3072": dict(kind="sq", bits=4, N=256, D=3072, nq=16, k=10, seed=5404, data="shells", r0=2.0, gamma=1.01),
    "sq8_w3072": dict(kind="sq", bits=8, N=256, D=3072, nq=16, k=10, seed=5608, data="shells", r0=2.0, gamma=1.015),
    "sq16_w3072": dict(kind="sq", bits=16, N=256, D=3072, nq=16, k=10, seed=6216, data="shells", r0=2.0, gamma=1.015),
    "sq8_d128": dict(kind="sq", bits=8, N=4099, D=128, nq=33, k=10, seed=5, data="scaled"),
    "sq4_d37_k300": dict(kind="sq", bits=4, N=1000, D=37, nq=16, k=300, seed=5, data="scaled"),
    "sq8_tiny": dict(kind="sq", bits=8, N=7, D=16, nq=3, k=10, seed=5, data="scaled"),
    "erq1": dict(kind="erq", bits=1, N=200, D=64, nq=16, k=10, seed=5, data="erq"),
    "erq4": dict(kind="erq", bits=4, N=200, D=64, nq=16, k=10, seed=5, data="erq"),
    "pq_M8_b8": dict(kind="pq", M=8, B=8, N=4099, D=64, nq=33, k=10, seed=5, data="scaled15"),
    "pq_M16_b4": dict(kind="pq", M=16, B=4, N=4099, D=64, nq=33, k=10, seed=5, data="scaled15"),
    "opq_M8_b8": dict(kind="opq", M=8, B=8, N=4099, D=64, nq=33, k=10, seed=5, data="scaled15"),
}
METRICS = ("l2", "ip")
# The D = 3072 cases are "shells": X_i = q0 + r_i g_i with r_i = r0 gamma^perm(i), Q = q0 + 0.01
# noise.  Plain Gaussian rows concentrate at D = 3072, where the fp32 bound then leaves a large
# part of the top-10 open.  Even on shells the 16 queries see nearly the same ranking, so a
# case's open share moves in steps of about 1/10 with the draw (IP: ~0.18 on average, the outer shells' projections
# on q0 being Gaussian); r0, gamma and the seed of each case were searched on the CPU, with the
# reference alone, for a draw that meets OPEN_CAP under both metrics (seeds 5300 + bits + 100 s,
# s = 0..11; gamma is limited by the bit width, since the outermost shell sets the range and so
# the quantization step the innermost shells must exceed).  The generator enforces the cap.


def sha(a) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


# ------------------------------------------------------------------------------ inputs
def inputs(name: str, erq_X=None):
    """(X, Q) float32 of a case, from its seed (`erq*`: X is the one of extrabitq_golden.npz)."""
    c = CASES[name]
    rng = np.random.default_rng(c["seed"])
    N, D, nq = c["N"], c["D"], c["nq"]
    if c["data"] == "shells":
        q0 = rng.standard_normal(D)
        r = c["r0"] * c["gamma"] ** rng.permutation(N).astype(np.float64)
        X = q0 + r[:, None] * rng.standard_normal((N, D))
        Q = q0 + 0.01 * rng.standard_normal((nq, D))
        return X.astype(np.float32), Q.astype(np.float32)
    if c["data"] == "erq":
        g = rng.standard_normal((nq, D))
        return np.ascontiguousarray(erq_X, np.float32), (g * rng.uniform(0.1, 3.0, D)).astype(np.float32)
    g = rng.standard_normal((N, D))
    s = rng.uniform(0.1, 3.0, D)
    X, Q = g * s, rng.standard_normal((nq, D)) * s
    if c["data"] == "scaled15":
        X, Q = X / 1.5, Q / 1.5
    return X.astype(np.float32), Q.astype(np.float32)


def table_centroids(name: str) -> np.ndarray:
    """Seeded (M, 2^B, dsub) float32 codebooks of a PQ / OPQ case: rows of a Gaussian with the
    spread of the data, so every centroid is used."""
    c = CASES[name]
    rng = np.random.default_rng(c["seed"] + 100)
    return (rng.standard_normal((c["M"], 1 << c["B"], c["D"] // c["M"])) * 1.2).astype(np.float32)


def table_rotation(name: str) -> np.ndarray:
    """Seeded orthonormal A (D, D) float32 of an OPQ case (QR of a Gaussian).  numpy's QR is not
    bit-reproducible across CPUs: the fixture stores A, this only generates it."""
    c = CASES[name]
    q, _ = np.linalg.qr(np.random.default_rng(c["seed"] + 200).standard_normal((c["D"], c["D"])))
    return q.astype(np.float32)


def matmul_seq(X, B) -> np.ndarray:
    """fp64 X . B with a fixed summation order (term k added k-th): no BLAS, so the same bits
    on every CPU."""
    X, B = np.asarray(X, np.float64), np.asarray(B, np.float64)
    out = np.zeros((X.shape[0], B.shape[1]))
    for k in range(X.shape[1]):
        out += X[:, k, None] * B[None, k, :]
    return out


def table_compress(X, C, A=None) -> np.ndarray:
    """fp64 nearest centroid per subspace, smallest index on ties: (n, M) uint8.  With A the
    rows are rotated first, y = x . A^T."""
    Y = matmul_seq(X, np.asarray(A, np.float64).T) if A is not None else np.asarray(X, np.float64)
    M, ksub, dsub = C.shape
    Ys = Y.reshape(len(Y), M, dsub)
    codes = np.empty((len(Y), M), np.uint8)
    for m in range(M):
        acc = np.zeros((len(Y), ksub))
        for t in range(dsub):  # fixed order, as matmul_seq
            acc += (Ys[:, m, t, None] - C[m, :, t].astype(np.float64)[None, :]) ** 2
        codes[:, m] = np.argmin(acc, axis=1)
    return codes


def table_decompress(codes, C, A=None) -> np.ndarray:
    """Gather the centroids ((n, D) float32, exact); with A rotate back, x_hat = y_hat . A
    (fp64, fixed order, then float32)."""
    M = C.shape[0]
    yh = np.concatenate([C[m][codes[:, m]] for m in range(M)], axis=1)
    return yh if A is None else matmul_seq(yh, A).astype(np.float32)


# ------------------------------------------------------------------------------ the rule
def keys(q, xh, metric):
    """(key, mag) of one query against every row, fp64."""
    q, xh = np.asarray(q, np.float64), np.asarray(xh, np.float64)
    if metric == "l2":
        key = ((xh - q) ** 2).sum(axis=1)
        return key, key
    p = xh * q
    return -p.sum(axis=1), np.abs(p).sum(axis=1)


def opq_terms(q, xh, yh, A, metric, key):
    """What the rotated-query ADC of an OPQ index may add to |dist - key|, per row.

    The device ranks by key_rot = ||y - y_hat||^2 (-y . y_hat) with y its rotation of q, where
    |y_t - y*_t| <= OPQ_ROT_TOL ||q|| ||A_t|| =: delta_t around the exact y* = q . A^T (the bound
    tests/test_opq_gpu.py asserts for the split-f16 rotation).  Hence
      L2: |sum (y - y_hat)^2 - key_rot*| <= 2 ||y* - y_hat|| ||delta|| + ||delta||^2
      IP: |y . y_hat - y* . y_hat|       <= sum_t delta_t |y_hat_t|
    and key_rot* differs from the fixture's key (fp64 on x_hat = float32(y_hat . A)) by a
    fixed amount, because the float32 A is orthonormal only to rounding and x_hat is rounded:
    that difference is computed here in fp64 and added as it is."""
    A64 = np.asarray(A, np.float64)
    ys = matmul_seq(np.asarray(q, np.float64)[None, :], A64.T)[0]
    delta = OPQ_ROT_TOL * np.linalg.norm(np.asarray(q, np.float64)) * np.linalg.norm(A64, axis=1)
    yh = np.asarray(yh, np.float64)
    if metric == "l2":
        krot = ((yh - ys) ** 2).sum(axis=1)
        rot = 2.0 * np.sqrt(krot) * np.linalg.norm(delta) + float(delta @ delta)
        mag_rot = krot + rot
    else:
        krot = -(yh * ys).sum(axis=1)
        rot = np.abs(yh) @ delta
        mag_rot = (np.abs(yh) * (np.abs(ys) + delta)).sum(axis=1)
    return rot + np.abs(krot - key), mag_rot


class Judge:
    """The rule for one (case, metric): keys, error bounds, the fp64 order and the open mask of
    every query, from Q and the reconstruction x_hat alone."""

    def __init__(self, Q, xh, metric, k, M=0, opq=None):
        """opq: (y_hat (N, D) rotated-space reconstruction, A) for an OPQ case."""
        self.metric, self.nq = metric, len(Q)
        N, D = xh.shape
        self.k = min(int(k), N)
        self.key, self.err, self.order, self.open = [], [], [], np.zeros((self.nq, self.k), bool)
        f = (D + M + 2) * U24
        for i, q in enumerate(Q):
            key, mag = keys(q, xh, metric)
            e = f * mag
            if opq is not None:
                extra, mag_rot = opq_terms(q, xh, opq[0], opq[1], metric, key)
                e = f * np.maximum(mag, mag_rot) + extra
            order = np.lexsort((np.arange(N), key))
            for j in range(self.k):
                r = order[j]
                near = np.abs(key - key[r]) <= e + e[r]
                near[r] = False
                self.open[i, j] = near.any()
            self.key.append(key)
            self.err.append(e)
            self.order.append(order[:self.k])

    @property
    def open_share(self) -> float:
        return float(self.open.mean()) if self.open.size else 0.0

    def ratio(self, ids, dists) -> float:
        """max |dist - key| / e over a result (reported next to the assertions)."""
        sign = -1.0 if self.metric == "ip" else 1.0
        worst = 0.0
        for i in range(self.nq):
            r = np.asarray(ids[i], np.int64)
            err = np.abs(sign * np.asarray(dists[i], np.float64) - self.key[i][r])
            with np.errstate(divide="ignore", invalid="ignore"):
                q = np.where(err == 0.0, 0.0, err / self.err[i][r])
            worst = max(worst, float(q.max()) if q.size else 0.0)
        return worst

    def problems(self, ids, dists, tie_order=True):
        """The clauses a result breaks, as strings (empty: accepted)."""
        out = []
        ids, dists = np.asarray(ids), np.asarray(dists)
        if ids.shape != (self.nq, self.k) or dists.shape != (self.nq, self.k):
            return [f"6: shapes {ids.shape} {dists.shape}, expected {(self.nq, self.k)}"]
        if ids.dtype != np.uint32 or dists.dtype != np.float32:
            return [f"6: dtypes {ids.dtype} {dists.dtype}"]
        N = len(self.key[0]) if self.nq else 0
        sign = -1.0 if self.metric == "ip" else 1.0
        for i in range(self.nq):
            key, e, rj = self.key[i], self.err[i], self.order[i]
            got = ids[i].astype(np.int64)
            if (got >= N).any():
                out.append(f"q{i}: id out of range {got.max()}")
                continue
            d = sign * dists[i].astype(np.float64)  # on the key's scale
            st = ~self.open[i]
            if (got[st] != rj[st]).any():
                j = int(np.flatnonzero(st & (got != rj))[0])
                out.append(f"1: q{i} settled position {j}: id {got[j]}, expected {rj[j]}")
            op = self.open[i]
            if (np.abs(key[got[op]] - key[rj[op]]) > 2.0 * e.max()).any():
                out.append(f"2: q{i} open position holds a row beyond 2 max e")
            if len(np.unique(got)) != len(got):
                out.append(f"3: q{i} duplicate ids")
            bad = np.abs(d - key[got]) > e[got]
            if bad.any():
                j = int(np.flatnonzero(bad)[0])
                out.append(f"4: q{i} position {j}: dist {d[j]!r} vs key {key[got[j]]!r} (e {e[got[j]]:.3e})")
            if (np.diff(dists[i]) * sign < 0).any() or np.isnan(dists[i]).any():
                out.append(f"5: q{i} distances out of order")
            if tie_order:
                same = (dists[i][1:] == dists[i][:-1]) & (key[got[1:]] == key[got[:-1]])
                if (same & (got[1:] <= got[:-1])).any():
                    out.append(f"7: q{i} tied rows out of id order")
        return out

    def check(self, ids, dists, what="", tie_order=True):
        p = self.problems(ids, dists, tie_order)
        assert not p, f"{what}: {len(p)} violations, first: {p[:3]}"
