"""The rank-aware code search restated in numpy, and the bounds its tests use.

V is orthogonal and x_hat = y_hat . V^T + mu, so for a query q

    ||q - x_hat||^2 = ||(q - mu) V - y_hat||^2        <q, x_hat> = <q V, y_hat> + <q, mu>

The library evaluates the right-hand sides in f32: ``a = f32((q - mu) V)`` (IP: ``f32(q V)``),
``b = f32(y_hat)`` and the chain of mivq_flat_search over t ascending,

    L2   acc <- fma(f32(a_t - b_t), f32(a_t - b_t), acc)         IP   acc <- fma(a_t, b_t, acc)

``chain_l2`` / ``chain_ip`` restate those chains.  numpy has no fma: the product of two f32 is
exact in f64, the sum is rounded to f64 and then to f32, which differs from the fused result
only where the f64 sum falls within 2^-53 of an f32 rounding point; the bounds below do not
depend on it (the GPU tests compare the kernel bit for bit with mivq_flat_search instead).
"""

from __future__ import annotations

import numpy as np

import _rankaware_rule as RR
import _search_rule as SR

NQ = 16
K = 10
DRAW_SHIFT = 100    # queries of a case: gaussian_rows(NQ, D, decay, draw + DRAW_SHIFT)


def queries(name: str) -> np.ndarray:
    c = RR.CASES[name]
    return RR.gaussian_rows(NQ, c["D"], c["decay"], c["draw"] + DRAW_SHIFT)


def rotate(Q, st, metric: str = "l2") -> np.ndarray:
    """(nq, D) fp64: (Q - mu) V for L2, Q V for IP, in a fixed summation order."""
    Q = np.asarray(Q, np.float64)
    return SR.matmul_seq(Q - st.mu if metric == "l2" else Q, st.V)


def levels(codes, st) -> np.ndarray:
    """(N, D) fp64: y_hat of the code rows."""
    return RR.lookup(RR.unpack(codes, st), st)


def chain_l2(a, B) -> np.ndarray:
    """(N,) f32: the L2 chain of one f32 vector a against the f32 rows B."""
    a, B = np.asarray(a, np.float32), np.asarray(B, np.float32)
    acc = np.zeros(B.shape[0], np.float32)
    for t in range(B.shape[1]):
        df = (a[t] - B[:, t]).astype(np.float32).astype(np.float64)
        acc = (df * df + acc.astype(np.float64)).astype(np.float32)
    return acc


def chain_ip(a, B) -> np.ndarray:
    """(N,) f32: the IP chain sum_t a_t b_t (the kernel's key is its negation)."""
    a, B = np.asarray(a, np.float32), np.asarray(B, np.float32)
    acc = np.zeros(B.shape[0], np.float32)
    for t in range(B.shape[1]):
        acc = (np.float64(a[t]) * B[:, t].astype(np.float64) + acc.astype(np.float64)).astype(np.float32)
    return acc


def top_ids(dist, k: int = K) -> np.ndarray:
    """The k smallest by (dist, id)."""
    return np.lexsort((np.arange(len(dist)), dist))[:k]


# ------------------------------------------------------------------ bounds
def l2_slack(a, B, D: int) -> np.ndarray:
    """(N,): (D + 8) 2^-23 (||a|| + ||b||)^2 for every row b of B: what an f32 chain over
    (a, b) may differ by from the fp64 value ||a* - b*||^2 of the unrounded vectors.

    With u = 2^-24: a = a* (1 + e), b = b* (1 + e'), |e|, |e'| <= u (one rounding each; the fp64
    error of the rotation, (D + 2) 2^-53 ||q - mu||, is far below u ||a*||), so
    | ||a - b||^2 - ||a* - b*||^2 | <= (2 ||a* - b*|| + w) w with w <= u (||a*|| + ||b*||), which
    is at most 2 u (1 + u) (||a|| + ||b||)^2.  The chain itself rounds every difference once
    (relative 2 u on its square) and every partial sum once, D roundings of sums no larger than
    the total: (D + 2) u ||a - b||^2 (1 + O(D u)) <= (D + 2) u (1 + O(D u)) (||a|| + ||b||)^2.
    Together (D + 4) u (1 + O(D u)) (||a|| + ||b||)^2 = (D + 4) / 2 in units of 2^-23: the bound
    is twice that.  The same holds for the chain over (q, f32(x_hat)) in the original domain:
    x_hat is rounded once, and V^T V = I to (D + 2) 2^-53.
    """
    a, B = np.asarray(a, np.float64), np.asarray(B, np.float64)
    return (D + 8) * 2.0 ** -23 * (np.linalg.norm(a) + np.linalg.norm(B, axis=1)) ** 2


def ip_slack(a, B, D: int, shift: float = 0.0) -> np.ndarray:
    """(N,): (D + 8) 2^-23 ||a|| (||b|| + shift): the IP form.

    The chain sum_t a_t b_t rounds D partial sums no larger than sum |a_t b_t| <= ||a|| ||b||
    and takes rounded inputs (2 u ||a|| ||b||): (D + 2) u (1 + O(D u)) ||a|| ||b||.  A score
    returned as f32(<q, mu>) - key adds u |<q, mu>| for the rounded constant and u |score| for
    the add, both at most u ||q|| (||b|| + ||mu||) with ||a|| = ||q V|| = ||q||; `shift` is that
    ||mu||, and it also covers the rounding of x_hat = y_hat V^T + mu to f32 when the truth is
    taken against the reference's reconstruction (u ||q|| ||x_hat||, ||x_hat|| <= ||b|| + ||mu||).
    Together (D + 5) u ||a|| (||b|| + shift): the bound is more than twice that.
    """
    a, B = np.asarray(a, np.float64), np.asarray(B, np.float64)
    return (D + 8) * 2.0 ** -23 * np.linalg.norm(a) * (np.linalg.norm(B, axis=1) + shift)


def l2_problems(ids, dists, truth, slack) -> list:
    """One query's result against the fp64 truth (N,) and the per-row slack (N,): every returned
    distance within the slack of the truth of its id, and no row left out whose truth is below
    the largest returned truth by more than the two rows' slacks (at most 2 max slack)."""
    ids = np.asarray(ids, np.int64)
    out = []
    if len(set(ids.tolist())) != len(ids) or (ids >= len(truth)).any():
        return [f"ids {ids}"]
    err = np.abs(np.asarray(dists, np.float64) - truth[ids])
    if (err > slack[ids]).any():
        j = int(np.argmax(err - slack[ids]))
        out.append(f"position {j}: dist {dists[j]!r}, truth {truth[ids[j]]!r}, slack {slack[ids[j]]:.3e}")
    worst = ids[int(np.argmax(truth[ids]))]
    rest = np.setdiff1d(np.arange(len(truth)), ids)
    bad = truth[rest] < truth[worst] - (slack[rest] + slack[worst])
    if bad.any():
        out.append(f"rows {rest[bad][:4]} are closer than returned row {worst}")
    if (np.diff(np.asarray(dists)) < 0).any():
        out.append("distances out of order")
    return out
