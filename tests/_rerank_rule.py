"""Re-ranking fixtures: the cases, their inputs, and a numpy restatement of mivq_rerank_*.

Shared by tests/test_rerank_cpu.py and tests/test_rerank_gpu.py.  Everything here is numpy on the
host.  One float32 operation per step, in the order include/mivq.h documents:

    x^    : f32 the row itself; SQ (float32(level) / float32(L)) * den + lo; LVQ _lvq_rule.decode,
            (lo + float32(idx) * delta) + mu with the row's lo and delta from its trailer
    chain : L2 acc = fmaf(q_t - x^_t, q_t - x^_t, acc) over t ascending from acc = 0;
            IP acc = fmaf(q_t, x^_t, acc), the key is -acc
    live  : the slots with id_offset <= id < id_offset + n, ids as unsigned numbers; every live
            slot is a candidate of its own (duplicates stay)
    out   : the k smallest (key, id), NaN keys as +inf, padded with (+inf, 0xFFFFFFFF)

fmaf has one rounding.  numpy has no fused multiply-add, so `fma32` forms it in float64: the
product of two float32 is exact there, the sum is rounded to odd (Boldo-Melquiond: the float64
sum, moved to its odd neighbour when it is inexact and even), and a value rounded to odd at 53
bits rounds to float32 as the exact sum does.  tests/test_rerank_cpu.py holds it against the
oracle's C fmaf chains.
"""

from __future__ import annotations

import functools

import numpy as np

import _ivf_quantized_rule as IQ
import _lvq_rule as LR

F32 = np.float32
NO_ID = 0xFFFFFFFF
L2, IP = 1, 0  # MIVQ_METRIC_L2, MIVQ_METRIC_INNER_PRODUCT
METRIC_ID = {"l2": L2, "ip": IP}
METRICS = ("l2", "ip")

# kind, bits of every store format the kernels are instantiated for in the tests
FORMATS = {"f32": ("f32", 0), "sq4": ("sq", 4), "sq8": ("sq", 8), "sq16": ("sq", 16), "lvq1": ("lvq", 1),
           "lvq3": ("lvq", 3), "lvq4": ("lvq", 4), "lvq8": ("lvq", 8)}
# d, and whether the store tensor is sliced so that its base is misaligned.  1: the tail alone;
# 37: element tail, LVQ-3 rows at odd byte offsets; 64 / 256: wide loads, 8-B and 16-B aligned
# rows; 100: every row of an unaligned store goes element by element
SHAPES = {"d1": (1, False), "d37": (37, False), "d64": (64, False), "d256": (256, False), "d100mis": (100, True)}
N, NQ, R, K = 300, 3, 40, 10  # the database, the batch, the list and k of the bit-identity cases


# ------------------------------------------------------------------------------ arithmetic
def fma32(a, b, c) -> np.ndarray:
    """float32 fmaf(a, b, c) of float32 arrays, correctly rounded."""
    a, b, c = (np.asarray(v, F32).astype(np.float64) for v in (a, b, c))
    with np.errstate(invalid="ignore", over="ignore"):
        p = a * b  # exact: 24 x 24 bits, exponents far inside float64's range
        s = p + c
        bb = s - p
        e = (p - (s - bb)) + (c - bb)  # TwoSum: p + c = s + e exactly
        even = (np.ascontiguousarray(s).view(np.int64) & 1) == 0
        move = np.isfinite(s) & np.isfinite(e) & (e != 0.0) & even
        s = np.where(move, np.nextafter(s, np.where(e > 0.0, np.inf, -np.inf)), s)
        return s.astype(F32)


def chain(q, xh, metric: int) -> np.ndarray:
    """The key of q (..., d) against xh (..., d), broadcast over the leading axes."""
    q, xh = np.asarray(q, F32), np.asarray(xh, F32)
    acc = np.zeros(np.broadcast_shapes(q.shape[:-1], xh.shape[:-1]), F32)
    for t in range(q.shape[-1]):
        if metric == L2:
            df = q[..., t] - xh[..., t]
            assert df.dtype == F32
            acc = fma32(df, df, acc)
        else:
            acc = fma32(q[..., t], xh[..., t], acc)
    return acc if metric == L2 else -acc


def sq_levels(codes, d: int, bits: int) -> np.ndarray:
    """(n, d) int64 levels of SQ code rows (4 bits: even dimension in the high nibble)."""
    codes = np.asarray(codes)
    if bits == 4:
        b = codes.astype(np.uint8)
        lv = np.empty((b.shape[0], 2 * b.shape[1]), np.int64)
        lv[:, 0::2], lv[:, 1::2] = b >> 4, b & 0x0F
        return lv[:, :d]
    return codes.view(np.uint16 if bits == 16 else np.uint8).astype(np.int64)[:, :d]


def dequant(kind: str, bits: int, store, params, d: int) -> np.ndarray:
    """x^ (n, d) float32 of a store."""
    if kind == "f32":
        return np.ascontiguousarray(store, F32)
    if kind == "lvq":
        return LR.decode(store, params[0], bits)
    lo, den = (np.asarray(p, F32) for p in params)
    s = sq_levels(store, d, bits).astype(F32) / F32((1 << bits) - 1)
    out = (s * den) + lo
    assert s.dtype == out.dtype == F32
    return out


def encode(kind: str, bits: int, X):
    """(store, params) of float32 rows X: SQ with lo = min, den = (max - min) + 1e-8 per dimension
    (codes uint8, uint16 at 16 bits), LVQ with mu = the sequential column mean."""
    X = np.ascontiguousarray(X, F32)
    if kind == "f32":
        return X, ()
    if kind == "lvq":
        mu = LR.seq_mean(X)
        return LR.encode(X, mu, bits), (mu,)
    lo = X.min(axis=0)
    den = (X.max(axis=0) - lo) + F32(1e-8)
    return IQ.sq_rows(X, lo, den, bits), (lo, den)


# ------------------------------------------------------------------------------ the rule
def rerank(Q, cand, xh, id_offset: int, metric: int, k: int):
    """(dists f32 (nq, k), ids uint32 (nq, k)) of candidate lists cand (nq, r) against the
    reconstructions xh (n, d) of rows id_offset .. id_offset + n - 1."""
    Q = np.ascontiguousarray(Q, F32)
    ids = (np.asarray(cand).astype(np.int64)) & 0xFFFFFFFF
    nq, r = ids.shape
    n = xh.shape[0]
    live = (ids >= id_offset) & (ids < id_offset + n)
    key = np.full((nq, r), np.inf, F32)
    if n > 0 and nq > 0:
        rows = np.where(live, ids - id_offset, 0)
        got = chain(Q[:, None, :], xh[rows], metric)
        got = np.where(np.isnan(got), F32(np.inf), got)
        key = np.where(live, got, F32(np.inf)).astype(F32)
    idk = np.where(live, ids, NO_ID)
    order = np.lexsort((idk, key), axis=1)[:, :k]
    dd = np.full((nq, k), np.inf, F32)
    ii = np.full((nq, k), NO_ID, np.uint32)
    dd[:, :order.shape[1]] = np.take_along_axis(key, order, axis=1)
    ii[:, :order.shape[1]] = np.take_along_axis(idk, order, axis=1).astype(np.uint32)
    return dd, ii


def same(got_d, got_i, want_d, want_i, what="") -> None:
    """Bit for bit: the ids, and the distances as their uint32 patterns."""
    got_d, want_d = np.ascontiguousarray(got_d, F32), np.ascontiguousarray(want_d, F32)
    got_i = np.ascontiguousarray(got_i).view(np.uint32)
    np.testing.assert_array_equal(got_i, np.asarray(want_i, np.uint32), err_msg=f"{what}: ids")
    np.testing.assert_array_equal(got_d.view(np.uint32), want_d.view(np.uint32), err_msg=f"{what}: dists")


# ------------------------------------------------------------------------------ inputs
def rows(n: int, d: int, seed, nq: int = NQ):
    """(X (n, d), Q (nq, d)) float32: Gaussian rows with a per-dimension spread U(0.2, 3) and
    shift, Gaussian queries."""
    rng = np.random.default_rng(seed)
    X = (rng.standard_normal((n, d)) * rng.uniform(0.2, 3.0, d) + rng.standard_normal(d)).astype(F32)
    Q = (rng.standard_normal((nq, d)) * 1.5).astype(F32)
    return X, Q


def lists(nq: int, r: int, n: int, id_offset: int, seed, dead: int = 0) -> np.ndarray:
    """(nq, r) uint32 candidate lists: distinct live ids in random order, `dead` of the slots
    replaced by ids outside [id_offset, id_offset + n): the 0xFFFFFFFF padding, id_offset + n and,
    when id_offset > 0, id_offset - 1."""
    rng = np.random.default_rng(seed)
    out = np.empty((nq, r), np.uint32)
    outside = [NO_ID, id_offset + n] + ([id_offset - 1] if id_offset > 0 else [])
    for a in range(nq):
        row = (rng.permutation(n)[:r] + id_offset).astype(np.int64)
        for j, s in enumerate(rng.permutation(r)[:dead]):
            row[s] = outside[j % len(outside)]
        out[a] = row.astype(np.uint32)
    return out


@functools.lru_cache(maxsize=None)
def case(fmt: str, shape: str):
    """One bit-identity case: dict(kind, bits, d, misaligned, X, Q, cand, store, params, xh)."""
    kind, bits = FORMATS[fmt]
    d, mis = SHAPES[shape]
    X, Q = rows(N, d, [N, d, bits])
    store, params = encode(kind, bits, X)
    return dict(kind=kind, bits=bits, d=d, misaligned=mis, X=X, Q=Q, store=store, params=params,
                cand=lists(NQ, R, N, 0, [R, d, bits], dead=5), xh=dequant(kind, bits, store, params, d))


def cases():
    """(format, shape) of every bit-identity case."""
    return [(f, s) for f in FORMATS for s in SHAPES]


# ------------------------------------------------------------------------------ the index cases
INDEX = dict(N=4096, D=32, nq=64, k=10, factor=10, M=4, seed=20)


def index_inputs():
    """(X, Q) float32 of the RefinedIndex tests: 4096 x 32 Gaussian rows, 64 Gaussian queries."""
    rng = np.random.default_rng(INDEX["seed"])
    X = rng.standard_normal((INDEX["N"], INDEX["D"])).astype(F32)
    Q = rng.standard_normal((INDEX["nq"], INDEX["D"])).astype(F32)
    return X, Q


def hits(ids, truth) -> np.ndarray:
    """Per query, how many of its ids are among the query's true neighbours."""
    return np.array([np.intersect1d(a, b).size for a, b in zip(np.asarray(ids), np.asarray(truth))])
