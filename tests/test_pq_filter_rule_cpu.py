"""The PQ filter rule (tests/_pq_filter_rule.py) and its input families, on the CPU oracle alone.

Before a kernel is involved: the canonical codes do not change under a common power-of-two
scale, the regime boundaries sit where pq_prep_mfma_kernel puts them, the oracle's own codes lie
inside the derived window (slack <= 1 follows from the derivation above pq_encode_mfma_kernel,
it is not a measured bound), and every family reaches what it is built to reach.  The kernels
are held to the same inputs in tests/test_pq_scale_gpu.py.

Measured here (n = 3001, M = 2, M = 4 for mixed_subspaces; the largest slack of the oracle's
codes, and the share of covered (row, subspace) items with 1 / 2 / >= 3 centroids inside the
window):

    family            dsub   max slack   1       2       >= 3
    scaled(s), all s    96   0.0198      0.941   0.055   0.005
    row_ladder          96   0.0279      0.970   0.028   0.002    14.6 % of rows past Xs < 65000
    row_ladder          64   0.0003      0.977   0.022   0.001    14.6 %
    row_ladder         192   0.0000      0.969   0.029   0.002    14.6 %
    mixed_subspaces     96   0.0376      0.946   0.051   0.003    e = -32, -2, 7, 28
    mixed_subspaces     64   0.0609      0.951   0.048   0.001    e = -31, -1, 8, 29
    mixed_subspaces    192   0.0391      0.925   0.071   0.004    e = -32, -2, 7, 28
    offset              96   0.2251      0.077   0.004   0.919
    offset              64   0.1816      0.079   0.003   0.918
    offset             192   0.1131      0.079   0.003   0.918
    outlier_centroid    96   0.0005      0       0       1        every |x| < 2^-14
    outlier_centroid    64   0.0003      0       0       1
    outlier_centroid   192   0.0002      0       0       1
    pairs_and_fulls     96   0.1344      0.040   0.502   0.459
    pairs_and_fulls     64   0.1842      0.036   0.503   0.462
    pairs_and_fulls    192   0.1245      0.039   0.501   0.459
"""

import numpy as np
import pytest

import _pq_filter_rule as R

DSUBS = (96, 64, 192)  # the widths the families run at on the device
N = 3001


@pytest.fixture(scope="module")
def measured(oracle):
    """name, dsub -> (X, C, codes, S, N, covered), computed once."""
    cache = {}

    def get(name, dsub):
        if (name, dsub) not in cache:
            X, C = R.family(name, N, dsub)
            codes = oracle.pq_encode(X, C)
            cache[(name, dsub)] = (X, C, codes) + R.slack(X, C, codes)
        return cache[(name, dsub)]

    return get


def test_oracle_codes_are_scale_invariant(oracle):
    ref = oracle.pq_encode(*R.scaled(0))
    # the planted rows: on centroid 3 (tied with 5: first index), between 6 and 7
    assert (ref[3] == 3).all() and np.isin(ref[4], (6, 7)).all()
    for s in (-40, -20, -12, 12, 20, 40):
        X, C = R.scaled(s)
        assert np.isfinite(X).all() and np.isfinite(C).all()
        np.testing.assert_array_equal(oracle.pq_encode(X, C), ref, err_msg=f"s = {s}")


def test_scale_exp_and_regime_boundaries():
    one = np.zeros((256, 8), np.float32)
    for v, e in ((1.0, 0), (1.0000001, 1), (0.99999994, 0), (0.5, -1), (3.0, 2), (2.0 ** -9, -9), (2.0 ** 100, 100),
                 (2.0 ** 120, 100), (2.0 ** -120, -100), (0.0, 0), (np.inf, 0)):
        one[17, 3] = v
        assert R.scale_exp(one) == e, v
    assert R.sigma_tau(0) == (1.0, 2.0 ** 14)
    for dsub in (96, 20):
        for e, scaled_regime in ((-9, True), (-8, False), (8, False), (9, True)):
            _, C = R.scaled(R.s_for_exp(e, N, dsub), N, dsub)
            assert R.exps(C) == [e, e]
            sigma, tau = R.sigma_tau(e)
            assert tau == 2.0 ** (14 - e)
            assert (sigma != 1.0) == scaled_regime
            if scaled_regime:
                assert sigma == 2.0 ** (12 - e)


@pytest.mark.parametrize("s", [-40, -9, 0, 9, 40])
def test_window_bounds_the_oracle_on_scaled(oracle, s):
    X, C = R.scaled(s)
    S, _, cov = R.slack(X, C, oracle.pq_encode(X, C))
    assert cov.all()
    print(f"scaled({s}): e {R.exps(C)} max slack {S.max():.4f}")
    assert S.max() <= 1.0


@pytest.mark.parametrize("dsub", DSUBS)
@pytest.mark.parametrize("name", sorted(R.FAMILIES))
def test_window_bounds_the_oracle(measured, name, dsub):
    _, C, _, S, Nw, cov = measured(name, dsub)
    assert cov.any()
    shares = [(Nw[cov] == 1).mean(), (Nw[cov] == 2).mean(), (Nw[cov] >= 3).mean()]
    print(f"{name} dsub {dsub}: e {R.exps(C)} max slack {np.nanmax(S):.4f} "
          f"in window 1 / 2 / >=3: {shares[0]:.3f} {shares[1]:.3f} {shares[2]:.3f}")
    assert (Nw[cov] >= 1).all()
    assert np.nanmax(S) <= 1.0


@pytest.mark.parametrize("dsub", DSUBS)
def test_offset_fills_the_full_list(measured, dsub):
    _, _, _, _, Nw, cov = measured("offset", dsub)
    assert cov.all()
    assert (Nw >= 3).mean() >= 0.40


@pytest.mark.parametrize("dsub", DSUBS)
def test_pairs_and_fulls_fill_both_lists_everywhere(measured, dsub):
    _, _, _, _, Nw, cov = measured("pairs_and_fulls", dsub)
    assert cov.all()
    for r0 in range(0, N, 1024):
        part = Nw[r0:r0 + 1024]
        assert (part == 2).mean() >= 0.30, r0
        assert (part >= 3).mean() >= 0.30, r0


@pytest.mark.parametrize("dsub", [96, 64])
def test_pairs_and_fulls_wide_call_fills_both_lists(oracle, dsub):
    """The M = 64 call of the device test (several blocks per wave), times 2^10: subspaces 0, 31
    and 63 hold the same floors, and the scale puts every subspace in the scaled regime."""
    X, C = R.pairs_and_fulls(6145, dsub, M=64)
    X, C = X * np.float32(1024.0), C * np.float32(1024.0)
    assert all(R.sigma_tau(e)[0] != 1.0 for e in R.exps(C))
    codes = oracle.pq_encode(X, C)
    for m in (0, 31, 63):
        S, Nw, cov = R.slack(X[:, m * dsub:(m + 1) * dsub], C[m:m + 1], codes[:, m:m + 1])
        assert cov.all() and S.max() <= 1.0
        for r0 in range(0, X.shape[0] - 1023, 1024):
            assert (Nw[r0:r0 + 1024] == 2).mean() >= 0.30 and (Nw[r0:r0 + 1024] >= 3).mean() >= 0.30, (m, r0)


@pytest.mark.parametrize("dsub", DSUBS)
def test_row_ladder_straddles_the_threshold(measured, dsub):
    X, C, _, _, _, cov = measured("row_ladder", dsub)
    assert np.isfinite(X).all()
    assert (~cov).any(1).mean() >= 0.10  # rows with a subspace past Xs < 65000
    assert cov.all(1).mean() >= 0.10
    # every 32-row block mixes both kinds and rows whose x~ is all f16 subnormals or zero
    tiny = np.abs(X).max(1) < 2.0 ** -14
    for b in range(N // 32):
        sl = slice(32 * b, 32 * b + 32)
        assert (~cov[sl]).any() and cov[sl].all(1).any() and tiny[sl].any(), b
    # the threshold rows: sigma ||x_m|| within 2^-9 of 65000 in exactly one subspace, on both sides
    M, dsub_ = C.shape[0], C.shape[2]
    xs = np.stack([R.filter_scores(X[:, m * dsub_:(m + 1) * dsub_], C[m])[1] for m in range(M)], 1)
    near = np.abs(xs / R.XS_LIMIT - 1.0) < 2.0 ** -9
    assert (near.sum(1) <= 1).all()
    assert (near & (xs > R.XS_LIMIT)).any(0).all() and (near & (xs < R.XS_LIMIT)).any(0).all()


@pytest.mark.parametrize("dsub", DSUBS)
def test_outlier_centroid_rows_are_f16_subnormal(measured, dsub):
    X, C, _, _, _, _ = measured("outlier_centroid", dsub)
    assert R.exps(C) == [-8, -8]
    assert all(R.sigma_tau(e)[0] == 1.0 for e in R.exps(C))
    assert (np.abs(X) < 2.0 ** -14).mean() >= 0.5
    # one component sets the exponent: without it the codebook is 2^-16 times the base
    C2 = C.copy()
    C2[:, 11, 0] = 0.0
    assert max(R.exps(C2)) <= -16


@pytest.mark.parametrize("dsub", DSUBS)
def test_mixed_subspaces_hold_both_regimes(measured, dsub):
    _, C, _, _, _, _ = measured("mixed_subspaces", dsub)
    sig = [R.sigma_tau(e)[0] for e in R.exps(C)]
    assert C.shape[0] == 4
    assert any(s == 1.0 for s in sig) and any(s > 1.0 for s in sig) and any(s < 1.0 for s in sig)
