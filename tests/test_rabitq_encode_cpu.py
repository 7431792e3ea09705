"""CPU: tests/_rabitq_encode_rule.py pinned to the oracle, before any GPU number is held to it.

The staged Extended RaBitQ references composed with a numpy rotation must give the oracle's code
rows and reconstructions byte for byte; the RaBitQ-1 reference must give the oracle's sign bits,
and the oracle's sequentially summed factors must lie within the derived bounds of the reference's
exact sums; and the planted-tie construction of the GPU test (s_raw = midpoint / sqrt(D) lands on
the midpoint again after the kernel's multiplication by sqrt(D)) is exact."""

import numpy as np
import pytest

import _rabitq_encode_rule as R

ERQ_DIMS = (1, 7, 9, 37, 100)
N = 11


def _erq_rows(D, seed):
    """Gaussian rows about an f32-representable centroid, one of them the centroid itself."""
    rng = np.random.default_rng([D, seed])
    c = rng.standard_normal(D).astype(np.float32).astype(np.float64)
    X = (c + rng.standard_normal((N, D))).astype(np.float32)
    X[4] = c.astype(np.float32)
    return X, c


@pytest.mark.parametrize("D", ERQ_DIMS)
@pytest.mark.parametrize("B", range(1, 9))
@pytest.mark.parametrize("rot", ["identity", "orthogonal"])
def test_staged_reference_equals_oracle(oracle, B, D, rot):
    X, c = _erq_rows(D, B)
    P = np.eye(D) if rot == "identity" else R.random_orthogonal(D, 7 + D)
    lv = R.lloyd_levels(B) if B <= 4 else R.synthetic_levels(B)
    r, o, nrm = R.normalize_ref(X, c)
    assert nrm[4] == 0.0 and not o[4].any()
    q = R.quantize_ref(o @ P, lv, B, nrm)
    ref = oracle.extrabitq_encode(X, c, P, lv, B)
    np.testing.assert_array_equal(q.codes, ref)
    if B <= 4:  # a Lloyd table has no 0 level: the zero row keeps a denominator and t = <0, s_hat> / den = 0
        assert q.t[4] == 0.0 and q.den[4] > R.EPS
    dec = R.finish_ref(R.dequantize_ref(ref, lv, D, B) @ P.T, ref, c, B)
    R.assert_same_bits(dec, oracle.extrabitq_decode(ref, c, P, lv, B), "decode")


def test_zero_level_table_takes_the_unit_t_branch():
    D = 9
    s_raw = np.random.default_rng(5).uniform(-0.39, 0.39, (N, D)) / np.sqrt(D)
    q = R.quantize_ref(s_raw, R.ZERO_LEVEL_TABLE, 2, np.ones(N))
    assert (q.idx == 1).all() and (q.den == 0).all() and (q.t == 1.0).all()
    assert (R.trailer(q.codes, D, 2)[1] == np.float32(1.0)).all()


def _rq1_rows(D, seed, centroid):
    rng = np.random.default_rng([D, seed])
    X = rng.standard_normal((N, D)).astype(np.float32)
    c = rng.standard_normal(D).astype(np.float32) if centroid else None
    X[2] = 0.0 if c is None else c  # residual exactly zero
    X[5] = (0.0 if c is None else c) - np.abs(X[5])  # every residual <= 0
    return X, c


@pytest.mark.parametrize("D", (1, 7, 9, 37, 520, 1024))
@pytest.mark.parametrize("metric", [1, 0])
@pytest.mark.parametrize("centroid", [False, True])
def test_rabitq1_reference_against_oracle(oracle, D, metric, centroid):
    X, c = _rq1_rows(D, metric, centroid)
    ref = R.rabitq1_ref(X, c, metric)
    bits, f0, f1 = R.rabitq1_split(oracle.rabitq_encode(X, c, metric), D)
    np.testing.assert_array_equal(bits, ref.bits)
    assert not bits[5].any() and ref.f0[2] == (0.0 if metric == 1 else -ref.orl2[2]) and ref.f1[2] == 0.0
    r0, r1 = R.rabitq1_ratios(f0, f1, ref, metric, R.gamma_seq(D))
    assert r0.max() <= 1.0 and r1.max() <= 1.0, (r0, r1)


@pytest.mark.parametrize("D", (4, 16, 64, 256))
def test_planted_tie_construction_is_exact(D):
    sq = np.sqrt(np.float64(D))
    for B in (1, 3, 4):
        lv = R.lloyd_levels(B)
        mids = R.midpoints(lv)
        s_raw = mids / sq
        np.testing.assert_array_equal(s_raw * sq, mids)
        np.testing.assert_array_equal(np.nextafter(s_raw, np.inf) * sq, np.nextafter(mids, np.inf))
        np.testing.assert_array_equal(np.nextafter(s_raw, -np.inf) * sq, np.nextafter(mids, -np.inf))
        planted, want = R.planted_ties(lv, D)
        assert len(planted) % 4 != 0 and planted.size >= 3 * len(mids)
        # mid == s does not count, one ulp above does: the reference puts q, q + 1, q there
        np.testing.assert_array_equal(R.quantize_ref(planted, lv, B, np.ones(len(planted))).idx, want)
