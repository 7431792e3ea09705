"""The RaBitQ encoders restated in numpy, one stage at a time.

Extended RaBitQ (csrc/extrabitq.hip) is four per-row stages around two fp64 GEMMs:

    normalize  : r = x - c, nrm = ||r||, o = r / max(nrm, 1e-12)
    quantize   : s = s_raw * sqrt(D), idx = searchsorted(midpoints, s) (left), s_hat = levels[idx],
                 t = <s, s_hat> / <s_hat, s_hat> (1 where the denominator <= 1e-12),
                 row = B-bit idx MSB-first (np.packbits) ++ f32 nrm ++ f32 t
    dequantize : o_hat = (levels[idx] / sqrt(D)) * t
    finish     : x_hat = f32(y * nrm + c)

Given its input every stage is one correctly rounded fp64 operation per step, which numpy performs
the same way, except the two reductions (nrm; the two sums behind t).  Those are returned from
exact sums here, so that a test can hold the kernel's tree-ordered sums to a worst-case bound.

RaBitQ-1 (csrc/rabitq_internal.h) is restated by rabitq1_ref: the sign bits of fl32(x - c) and the
two f32 factors, computed in fp64 from exact sums of the f32 residuals.

Everything here is numpy on the host; tests/test_rabitq_encode_cpu.py pins it to the oracle.
"""

from __future__ import annotations

import functools
import math
from decimal import Decimal, localcontext
from fractions import Fraction
from typing import NamedTuple

import numpy as np

import _extrabitq_search_rule as ES

EPS = 1e-12  # the guard of normalize and of t's denominator
FLT_EPSILON = float(np.finfo(np.float32).eps)
U32 = 2.0 ** -24  # unit roundoff of f32
U64 = 2.0 ** -53  # unit roundoff of f64

code_size = ES.code_size


# ------------------------------------------------------------------------------ level tables
@functools.lru_cache(maxsize=None)
def _lloyd(B: int) -> np.ndarray:
    import oracle as O

    return O.lloyd_1d_normal(2 ** B, seed=0)


def lloyd_levels(B: int) -> np.ndarray:
    """The table ExtendedRaBitQuantizer fits for B bits (seed 0); computed once per session."""
    return _lloyd(B).copy()


def synthetic_levels(B: int, seed: int = 0) -> np.ndarray:
    """A cheap strictly increasing table of 2^B levels over [-3, 3]: an even grid, each level moved
    by less than 0.3 of the spacing."""
    L = 2 ** B
    step = 6.0 / (L - 1)
    lv = np.linspace(-3.0, 3.0, L) + np.random.default_rng([B, seed]).uniform(-0.3, 0.3, L) * step
    assert np.all(np.diff(lv) > 0)
    return lv


ZERO_LEVEL_TABLE = np.array([-1.0, 0.0, 1.0, 2.0])  # B = 2; |s| < 0.5 quantises to the 0 level


def midpoints(levels) -> np.ndarray:
    lv = np.asarray(levels, np.float64)
    return 0.5 * (lv[:-1] + lv[1:])


# ------------------------------------------------------------------------------ bit patterns
def bits_of(a) -> np.ndarray:
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def assert_same_bits(got, ref, what: str = "") -> None:
    """Equal bit for bit (so -0.0 != 0.0); a NaN must meet a NaN, whatever its payload."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.dtype == ref.dtype and got.shape == ref.shape, (what, got.dtype, ref.dtype, got.shape, ref.shape)
    gn, rn = np.isnan(got), np.isnan(ref)
    np.testing.assert_array_equal(gn, rn, err_msg=f"{what}: NaN positions")
    np.testing.assert_array_equal(np.where(gn, 0, bits_of(got)), np.where(rn, 0, bits_of(ref)), err_msg=what)


# ------------------------------------------------------------------------------ Extended RaBitQ
def exact_norm(r) -> np.ndarray:
    """||row|| of fp64 rows from the exact rational sum of squares, rounded to fp64 once (through
    a 60-digit square root)."""
    out = np.empty(len(r), np.float64)
    with localcontext() as ctx:
        ctx.prec = 60
        ctx.Emin, ctx.Emax = -999999, 999999
        for i, row in enumerate(np.asarray(r, np.float64)):
            ss = sum((Fraction(float(v)) ** 2 for v in row), Fraction(0))
            out[i] = float((Decimal(ss.numerator) / Decimal(ss.denominator)).sqrt())
    return out


def normalize_ref(X, c):
    """(r, o, nrm): r = X - c in fp64 (one rounding), nrm its exact norm rounded to fp64,
    o = r / max(nrm, 1e-12).  The kernel divides by its own nrm: see o_of."""
    r = np.asarray(X).astype(np.float64) - np.asarray(c, np.float64)
    nrm = exact_norm(r)
    return r, o_of(r, nrm), nrm


def o_of(r, nrm) -> np.ndarray:
    return r / np.maximum(np.asarray(nrm, np.float64), EPS)[:, None]


def norm_bound(D: int, nrm_ref) -> np.ndarray:
    """|nrm_kernel - nrm_ref| at worst: per lane an fma chain of ceil(D / 64) non-negative terms,
    six tree levels, one square root (which halves the sum's relative error and adds one
    rounding), and the reference's own rounding to fp64."""
    return (math.ceil(D / 64) + 8) * U64 * np.asarray(nrm_ref, np.float64)


class Quantized(NamedTuple):
    codes: np.ndarray  # (N, code_size) u8: index bytes, f32 nrm, f32 t
    idx: np.ndarray    # (N, D) int64
    t: np.ndarray      # (N,) fp64, from exact sums of the fp64 products
    sabs: np.ndarray   # (N,) fp64: sum |s * s_hat|
    den: np.ndarray    # (N,) fp64: sum s_hat^2


def quantize_ref(s_raw, levels, B: int, nrm) -> Quantized:
    s_raw = np.asarray(s_raw, np.float64)
    lv = np.asarray(levels, np.float64)
    N, D = s_raw.shape
    assert lv.shape == (2 ** B,)
    s = s_raw * np.sqrt(np.float64(D))
    idx = np.searchsorted(midpoints(lv), s).astype(np.int64)  # side="left": mid < s counts, mid == s does not
    sh = lv[idx]
    num = np.array([math.fsum(row) for row in s * sh])
    den = np.array([math.fsum(row) for row in sh * sh])
    sabs = np.array([math.fsum(row) for row in np.abs(s * sh)])
    t = np.ones(N)
    np.divide(num, den, out=t, where=den > EPS)
    with np.errstate(over="ignore"):
        codes = ES.pack(idx, np.asarray(nrm, np.float64).astype(np.float32), t.astype(np.float32), B)
    return Quantized(codes, idx, t, sabs, den)


def planted_ties(levels, D: int):
    """(s_raw (rows, D), idx (rows, D)): for every midpoint m_q of the table m_q / sqrt(D), the fp64
    above it and the fp64 below it, whose indices are q, q + 1 and q when sqrt(D) is a power of two
    (the kernel's s = s_raw * sqrt(D) is then m_q and its two neighbours exactly).  The values
    repeat to fill a row count that is no multiple of 4."""
    sq = np.sqrt(np.float64(D))
    m = midpoints(levels) / sq
    vals = np.stack([m, np.nextafter(m, np.inf), np.nextafter(m, -np.inf)], axis=1).reshape(-1)
    q = np.arange(len(m))
    want = np.stack([q, q + 1, q], axis=1).reshape(-1)
    rows = -(-len(vals) // D)
    rows += rows % 4 == 0
    return np.resize(vals, (rows, D)), np.resize(want, (rows, D))


def t_bound(D: int, q: Quantized) -> np.ndarray:
    """|f32 t_kernel - t_ref| at worst where den > 1e-12: half an f32 ulp of t, plus the fp64
    reductions (products and tree sums of num and den, D roundings each way at most)."""
    den = np.where(q.den > EPS, q.den, 1.0)
    return U32 * np.abs(q.t) * (1 + 1e-6) + D * 2.0 ** -51 * q.sabs / den


def dequantize_ref(codes, levels, D: int, B: int) -> np.ndarray:
    """(levels[idx] / sqrt(D)) * t, t the row's f32 widened."""
    return ES.o_hat(codes, levels, D, B)


def finish_ref(y, codes, c, B: int) -> np.ndarray:
    y = np.asarray(y, np.float64)
    _, nrm, _ = ES.unpack(codes, y.shape[1], B)
    with np.errstate(over="ignore", invalid="ignore"):
        return (y * nrm.astype(np.float64)[:, None] + np.asarray(c, np.float64)).astype(np.float32)


def trailer(codes, D: int, B: int):
    """(nrm, t) f32 of code rows."""
    _, nrm, t = ES.unpack(codes, D, B)
    return nrm, t


def _erq_unpack(cb, D, nb):
    ib = (D * nb + 7) // 8
    bits = np.unpackbits(cb[:, :ib], axis=1)[:, :D * nb].reshape(len(cb), D, nb)
    return (bits.astype(np.int64) << np.arange(nb - 1, -1, -1)).sum(-1)


def _assert_ties_only(got, ref, X, c, P, lv, nbits, max_frac=1e-3):
    """Index mismatches only where s sits on a level midpoint (fp64 rounding), one level apart."""
    N, D = X.shape
    gi, ri = _erq_unpack(got, D, nbits), _erq_unpack(ref, D, nbits)
    bad = np.argwhere(gi != ri)
    r = X.astype(np.float64) - c
    s = (r / np.maximum(np.linalg.norm(r, axis=1), 1e-12)[:, None] @ P) * np.sqrt(D)
    mids = 0.5 * (lv[:-1] + lv[1:])
    for i, j in bad:
        assert np.min(np.abs(mids - s[i, j])) <= 1e-12 * max(1.0, abs(s[i, j])), (i, j)
        assert abs(int(gi[i, j]) - int(ri[i, j])) == 1
    assert len(bad) <= max_frac * N * D
    return bad


def random_orthogonal(D: int, seed: int) -> np.ndarray:
    P, _ = np.linalg.qr(np.random.default_rng(seed).standard_normal((D, D)))
    return np.ascontiguousarray(P, np.float64)


# ------------------------------------------------------------------------------ RaBitQ-1
class RaBitQ1(NamedTuple):
    bits: np.ndarray  # (N, ceil(D / 8)) u8, LSB-first
    f0: np.ndarray    # (N,) fp64
    f1: np.ndarray    # (N,) fp64
    l2: np.ndarray    # (N,) fp64: sum rr^2
    orl2: np.ndarray  # (N,) fp64: sum x^2
    dp: np.ndarray    # (N,) fp64: sum |rr|


def rabitq1_ref(X, c, metric: int) -> RaBitQ1:
    """metric 1 = L2, 0 = inner product (include/mivq.h).  rr = fl32(x - c) as the kernel forms it;
    the three sums are exact sums of the f32 values' fp64 products (an f32 square is exact in fp64),
    the factors follow rabitq_internal.h's epilogue in fp64."""
    X = np.ascontiguousarray(X, np.float32)
    N, D = X.shape
    with np.errstate(over="ignore", invalid="ignore"):
        rr = X if c is None else X - np.asarray(c, np.float32)
        assert rr.dtype == np.float32
        bits = np.packbits(rr > 0, axis=1, bitorder="little")
        r64, x64 = rr.astype(np.float64), X.astype(np.float64)
        l2 = np.array([math.fsum(row) if np.all(np.isfinite(row)) else row.sum() for row in r64 * r64])
        orl2 = np.array([math.fsum(row) if np.all(np.isfinite(row)) else row.sum() for row in x64 * x64])
        dp = np.array([math.fsum(row) if np.all(np.isfinite(row)) else row.sum() for row in np.abs(r64)])
        inv_d_sqrt = 1.0 / np.sqrt(np.float64(D))
        inv_norm = np.where(np.abs(l2) < FLT_EPSILON, 1.0, 1.0 / np.sqrt(np.where(l2 == 0, 1.0, l2)))
        ndp = dp * inv_norm * inv_d_sqrt
        inv_dp = np.where(np.abs(ndp) < FLT_EPSILON, 1.0, 1.0 / np.where(ndp == 0, 1.0, ndp))
        f0 = l2 - orl2 if metric == 0 else l2.copy()
        f1 = inv_dp * np.sqrt(l2)
    return RaBitQ1(bits, f0, f1, l2, orl2, dp)


def rabitq1_split(codes, D: int):
    """(bits (N, nb) u8, f0 (N,) f32, f1 (N,) f32) of RaBitQ-1 code rows."""
    codes = np.ascontiguousarray(codes, np.uint8)
    nb = (D + 7) // 8
    assert codes.shape[1] == nb + 8
    tr = np.ascontiguousarray(codes[:, nb:]).view("<f4")
    return codes[:, :nb], tr[:, 0].copy(), tr[:, 1].copy()


def gamma_wave(D: int) -> float:
    """Relative error of a kernel sum of non-negative f32 terms: per lane a chain of
    8 * ceil(nb / 64) terms, nb = ceil(D / 8) sign bytes, then six tree levels."""
    return (8 * math.ceil(math.ceil(D / 8) / 64) + 6) * U32


def gamma_seq(D: int) -> float:
    """The same for the oracle's one sequential chain of D terms."""
    return D * U32


def rabitq1_ratios(f0, f1, ref: RaBitQ1, metric: int, gamma: float, rows=None):
    """(|f0 - f0_ref| / bound, |f1 - f1_ref| / bound) per row, 0 where both sides are 0:
    L2 |f0 - l2| <= g l2;  IP |f0 - (l2 - orl2)| <= g (l2 + orl2) + u |f0|;
    |f1 - f1_ref| <= (2 g + 8 u) |f1_ref|."""
    rows = slice(None) if rows is None else rows
    f0, f1 = np.asarray(f0, np.float64)[rows], np.asarray(f1, np.float64)[rows]
    l2, orl2, f0r, f1r = ref.l2[rows], ref.orl2[rows], ref.f0[rows], ref.f1[rows]
    b0 = gamma * (l2 + orl2) + U32 * np.abs(f0) if metric == 0 else gamma * l2
    b1 = (2 * gamma + 8 * U32) * np.abs(f1r)
    e0, e1 = np.abs(f0 - f0r), np.abs(f1 - f1r)

    def ratio(e, b):
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(e == 0, 0.0, e / b)  # e > 0 against b = 0 gives inf and fails

    return ratio(e0, b0), ratio(e1, b1)
