"""The PQ encode filter window, restated in numpy fp64, and the input families that reach its edges.

`mivq_pq_encode` promises the canonical fp32 codes of include/mivq.h; it gets there through an
fp16-MFMA filter whose window W = a Xs + b is derived in the comment above
pq_encode_mfma_kernel (csrc/pq.hip) and whose constants pq_prep_mfma_kernel builds.  This module
states that derivation once more, in plain numpy, with nothing imported from the library:

    e      = ceil(log2 max|c|) of the subspace's codebook, clamped to [-100, 100]
    tau    = 2^(14 - e)                          c~ = f16(tau c)
    sigma  = 1 if -8 <= e <= 8 else 2^(12 - e)   x~ = f16(sigma x)
    p_k    = <x~, c~_k> - sigma tau |c_k|^2 / 2  (the filter score, maximised)
    Xs     = sigma ||x_m||
    W      = 1.0625 (a Xs + b),  a = u_h Dmax + DDmax + a_rest,  b = 1.001 eta sqrt(dsub) Dmax + b_rest
    a_rest = Cs (2.004 g_{dsub+2} + 2.004 2^-15 + 2 (g_dsub + u)),   Cs = tau max||c||
    b_rest = Hs (g_{dsub+2} + 2 g_dsub + 2^-15 + u),                 Hs = sigma tau max||c||^2
    Dmax = max_ij ||c~_i - c~_j||,  DDmax = max_ij ||(c~_i - tau c_i) - (c~_j - tau c_j)||

The derivation says that the canonical winner k* has p_k* >= p_max - (a Xs + b) for every row
whose x~ is finite and whose Xs < 65000 (the other rows take the exact path).  `slack` measures
how much of the window the oracle's own codes use; tests/test_pq_filter_rule_cpu.py holds it
to <= 1 on every family below, and tests/test_pq_scale_gpu.py holds the kernels to the oracle
on the same inputs.

Multiplying rows and codebook by one power of two changes nothing in the canonical fp32 chains
(until squares underflow, near 2^-60), so the expected codes of `scaled(s)` are both the
oracle's at that scale and the codes at scale 1.
"""

from __future__ import annotations

import math

import numpy as np

F32 = np.float32
U32 = 2.0 ** -24      # fp32 unit roundoff
K_UH = 2.0 ** -11     # f32 -> f16 round to nearest even
K_ETA = 2.0 ** -24    # bound taken for the error of an f16 subnormal result (it is 2^-25)
K_PACK = 2.0 ** -15   # the 8 low mantissa bits replaced by the centroid index
K_SCALE_C = 14
K_SCALE_X = 12
SAFETY = 1.0625
XS_LIMIT = 65000.0


# ------------------------------------------------------------------------------- the rule
def scale_exp(Cm: np.ndarray) -> int:
    """e = ceil(log2 max|c|) of one subspace's codebook (ksub, dsub); 0 when the maximum is 0
    or not finite; clamped to [-100, 100].  (frexp: exact, also on powers of two.)"""
    cmax = float(np.abs(np.asarray(Cm, np.float64)).max())
    if not (cmax > 0.0 and math.isfinite(cmax)):
        return 0
    f, ex = math.frexp(cmax)  # cmax = f 2^ex, f in [0.5, 1)
    e = ex - 1 if f == 0.5 else ex
    return max(-100, min(100, e))


def sigma_tau(e: int):
    """(sigma, tau) of a subspace with scale exponent e."""
    tau = 2.0 ** (K_SCALE_C - e)
    sigma = 1.0 if -8 <= e <= 8 else 2.0 ** (K_SCALE_X - e)
    return sigma, tau


def _image(Cm: np.ndarray, tau: float):
    """c~ = f16(tau c) and dc = c~ - tau c, in fp64 (tau c is formed in fp32, as the kernels do)."""
    t = (np.asarray(Cm, F32) * F32(tau)).astype(F32)
    with np.errstate(over="ignore"):
        h = t.astype(np.float16).astype(np.float64)
    return h, h - t.astype(np.float64)


def _max_pair_norm(V: np.ndarray) -> float:
    """max_ij ||v_i - v_j|| in fp64, by direct differences (the residuals cancel in a Gram form)."""
    best = 0.0
    for i0 in range(0, V.shape[0], 32):
        d = V[i0:i0 + 32, None, :] - V[None, :, :]
        best = max(best, float((d * d).sum(-1).max()))
    return math.sqrt(best)


def window(Cm: np.ndarray):
    """(a, b) of W = a Xs + b for one subspace, without the 1.0625: the formula of
    pq_prep_mfma_kernel in fp64 on exact norms and spreads."""
    Cm = np.asarray(Cm, F32)
    dsub = Cm.shape[1]
    sigma, tau = sigma_tau(scale_exp(Cm))
    cn_max = float((Cm.astype(np.float64) ** 2).sum(-1).max())
    h, dc = _image(Cm, tau)
    Dm, DDm = _max_pair_norm(h), _max_pair_norm(dc)
    Cs = tau * math.sqrt(cn_max)
    Hs = sigma * tau * cn_max
    gd = dsub * U32 / (1.0 - dsub * U32)
    gn = (dsub + 2) * U32 / (1.0 - (dsub + 2) * U32)
    a_rest = Cs * (2.004 * gn + 2.004 * K_PACK + 2.0 * (gd + U32))
    b_rest = Hs * (gn + 2.0 * gd + K_PACK + U32)
    a = K_UH * Dm + DDm + a_rest
    b = 1.001 * K_ETA * math.sqrt(dsub) * Dm + b_rest
    return a, b


def filter_scores(Xm: np.ndarray, Cm: np.ndarray):
    """(P, Xs): P[i, k] = <f16(sigma x_i), f16(tau c_k)> - sigma tau |c_k|^2 / 2 in fp64 and
    Xs[i] = sigma ||x_i||, for rows Xm (n, dsub) against Cm (ksub, dsub).  A row whose x~ is not
    finite gets NaN scores."""
    Xm = np.asarray(Xm, F32)
    Cm = np.asarray(Cm, F32)
    sigma, tau = sigma_tau(scale_exp(Cm))
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        xt = (Xm * F32(sigma)).astype(F32).astype(np.float16).astype(np.float64)
    h, _ = _image(Cm, tau)
    half = 0.5 * sigma * tau * (Cm.astype(np.float64) ** 2).sum(-1)
    finite = np.isfinite(xt).all(-1)
    P = np.where(finite[:, None], np.where(finite[:, None], xt, 0.0) @ h.T - half[None, :], np.nan)
    with np.errstate(invalid="ignore", over="ignore"):
        Xs = sigma * np.sqrt((Xm.astype(np.float64) ** 2).sum(-1))
    return P, Xs


def slack(X: np.ndarray, C: np.ndarray, codes: np.ndarray):
    """(S, N, covered), each (n, M).  For the (row, subspace) items the window covers (x~ finite,
    Xs < 65000): S = (p_max - p_code) / (1.0625 (a Xs + b)), N = the number of centroids with
    p >= p_max - 1.0625 (a Xs + b).  Elsewhere S is NaN and N is 0."""
    C = np.asarray(C, F32)
    M, _, dsub = C.shape
    n = X.shape[0]
    S = np.full((n, M), np.nan)
    N = np.zeros((n, M), np.int64)
    covered = np.zeros((n, M), bool)
    for m in range(M):
        P, Xs = filter_scores(X[:, m * dsub:(m + 1) * dsub], C[m])
        a, b = window(C[m])
        ok = np.isfinite(P).all(-1) & (Xs < XS_LIMIT)
        W = SAFETY * (a * Xs[ok] + b)
        Pm = P[ok]
        pmax = Pm.max(-1)
        S[ok, m] = (pmax - Pm[np.arange(Pm.shape[0]), codes[ok, m]]) / W
        N[ok, m] = (Pm >= (pmax - W)[:, None]).sum(-1)
        covered[:, m] = ok
    return S, N, covered


def prep_offsets(M, dsub, ksub=256):
    """Byte offsets inside the mivq_pq_prepare buffer (mirror of PqPrepLayout, mivq_common.h)."""
    al = lambda v: (v + 255) // 256 * 256  # noqa: E731
    ks = (dsub + 15) // 16
    L, off = {}, 0
    for name, size in (("cn", 4 * M * ksub), ("ct", 4 * M * dsub * ksub), ("img", M * 8 * ks * 64 * 16),
                       ("hinit", 4 * M * ksub), ("bnd", 16 * M), ("spread", 8 * M),
                       ("pd", M * 256 * 256 * 8 if M <= 64 else 0), ("bnd2", 16 * M)):
        L[name] = off
        off = al(off + size)
    return L


# ------------------------------------------------------------------------------ the cases
def _unit_rows(rng, n, d):
    X = rng.standard_normal((n, d)).astype(F32)
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    return X


def _draw_codebook(rng, X, M, noise):
    """256 centroids per subspace drawn from rows of X plus `noise` (absolute, per component),
    with an exact tie (3, 5: the canonical first index wins) and a 1 + 1e-7 near-tie (6, 7)."""
    n, d = X.shape
    dsub = d // M
    C = X[rng.integers(0, n, size=256)].reshape(256, M, dsub).transpose(1, 0, 2).copy()
    C += rng.standard_normal(C.shape).astype(F32) * F32(noise)
    C[:, 5] = C[:, 3]
    C[:, 7] = C[:, 6] * (1 + 1e-7)
    return np.ascontiguousarray(C, dtype=F32)


def exps(C):
    return [scale_exp(C[m]) for m in range(C.shape[0])]


def base(n=3001, dsub=96, M=2, seed=0):
    """Unit-norm rows, a codebook drawn from them plus 5 % noise with the planted tie and
    near-tie, a row on a centroid and a row between the near-tied pair.  The seed moves on
    until every subspace has the same scale exponent, so that `scaled` puts all of them in one
    regime."""
    while True:
        rng = np.random.default_rng([n, dsub, M, seed])
        X = _unit_rows(rng, n, M * dsub)
        C = _draw_codebook(rng, X, M, 0.05 * np.abs(X).mean())
        if len(set(exps(C))) == 1:
            break
        seed += 1000
    if n > 10:
        X[3] = C[:, 3].reshape(-1)
        X[4] = (0.5 * (C[:, 6] + C[:, 7])).reshape(-1)
    return X, C


def scaled(s, n=3001, dsub=96, M=2, seed=0):
    """base() with rows and codebook times 2^s (exact in fp32)."""
    X, C = base(n, dsub, M, seed)
    f = F32(2.0 ** s)
    return X * f, C * f


def s_for_exp(e, n=3001, dsub=96, M=2, seed=0):
    """The s at which every subspace of scaled(s, ...) has scale exponent e."""
    return e - exps(base(n, dsub, M, seed)[1])[0]


def row_ladder(n=3001, dsub=96, M=2, seed=1, s=0):
    """Codebook of scaled(s), fixed; row i times 2^j(i), j cycling through -30..17, so every
    32-row block holds rows whose x~ is all f16 subnormals, ordinary rows, and rows past the
    Xs < 65000 threshold.  Every fourth row sits on the threshold instead: its subvector in one
    subspace (alternating) is rescaled to sigma ||x_m|| = 65000 (1 + 2^-10) or 65000 (1 - 2^-10)
    by turns, the other subspaces staying ordinary."""
    X, C = scaled(s, n, dsub, M, seed)
    X = X.copy()
    j = (np.arange(n) % 48) - 30
    X *= (2.0 ** j).astype(F32)[:, None]
    X0 = scaled(s, n, dsub, M, seed)[0]
    sig = [sigma_tau(e)[0] for e in exps(C)]
    for t, i in enumerate(range(2, n, 4)):
        m = t % M
        X[i] = X0[i]
        sub = X0[i, m * dsub:(m + 1) * dsub].astype(np.float64)
        target = XS_LIMIT * (1.0 + (2.0 ** -10 if (t // M) % 2 == 0 else -2.0 ** -10)) / sig[m]
        X[i, m * dsub:(m + 1) * dsub] = (sub * (target / np.linalg.norm(sub))).astype(F32)
    return X, C


def mixed_subspaces(n=3001, dsub=96, seed=2):
    """M = 4; subspace m of rows and codebook times 2^-30, 1, 2^9, 2^30: scaled and unscaled
    regimes side by side in one call."""
    M = 4
    X, C = base(n, dsub, M, seed)
    X, C = X.copy(), C.copy()
    for m, s in enumerate((-30, 0, 9, 30)):
        f = F32(2.0 ** s)
        X[:, m * dsub:(m + 1) * dsub] *= f
        C[m] *= f
    return X, C


def offset(n=3001, dsub=96, M=2, seed=3):
    """Rows 8 x + 5 and a codebook drawn from them: every centroid sits near one point far from
    the origin, so Cs Xs 2^-15 dwarfs the score gaps and most rows keep three or more centroids
    inside the window.  x is the leading M dsub columns of unit-norm rows of width 1536 (the
    suite's usual rows; side by side when d > 1536), so the spread about the offset depends on
    neither dsub nor M."""
    rng = np.random.default_rng([n, dsub, M, seed])
    d = M * dsub
    x = np.hstack([_unit_rows(rng, n, 1536) for _ in range((d + 1535) // 1536)])[:, :d]
    X = (F32(8.0) * x + F32(5.0)).astype(F32)
    C = _draw_codebook(rng, X, M, 0.05 * float(X.std()))
    return X, C


def outlier_centroid(n=3001, dsub=96, M=2, seed=4):
    """sigma = 1 with e = -8 set by ONE planted centroid component (0.75 2^-8) while the rows and
    every other centroid value are about 2^-16 times the base: x~ = f16(x) is all f16
    subnormals, and the window's b term carries the bound."""
    X, C = scaled(-16, n, dsub, M, seed)
    C = C.copy()
    C[:, 11, 0] = F32(0.75 * 2.0 ** -8)
    return X, C


def pairs_and_fulls(n=3001, dsub=96, M=2, seed=5):
    """Even rows: the midpoint of the near-tied pair (6, 7) of the offset() codebook, plus a
    little noise (two centroids in the window, too close for the pair window to settle: the
    pair list).  Odd rows: offset() rows (mostly three or more: the full list).  Both lists of
    a workgroup fill from the two ends of its allocation."""
    X, C = offset(n, dsub, M, seed)
    rng = np.random.default_rng([n, dsub, M, seed, 1])
    mid = (0.5 * (C[:, 6].astype(np.float64) + C[:, 7])).reshape(-1)
    ne = (n + 1) // 2
    X = X.copy()
    X[0::2] = (mid[None, :] + 1e-3 * rng.standard_normal((ne, mid.size))).astype(F32)
    return X, C


FAMILIES = {
    "row_ladder": row_ladder,
    "mixed_subspaces": mixed_subspaces,
    "offset": offset,
    "outlier_centroid": outlier_centroid,
    "pairs_and_fulls": pairs_and_fulls,
}


def family(name, n=3001, dsub=96):
    """(X, C) of a family at (n, dsub); M is the family's own (4 for mixed_subspaces, else 2)."""
    return FAMILIES[name](n=n, dsub=dsub)
