"""GPU: the kernels that write RaBitQ code rows, against tests/_rabitq_encode_rule.py.

Extended RaBitQ (csrc/extrabitq.hip) one stage at a time, each stage fed from numpy: every output
that its input determines (the residual and its division, the level indices and their packing, the
f32 image of the norm, dequantize, finish) is compared bit for bit; the two reductions (the norm;
t) are held to worst-case bounds about exact sums.  Then the whole encode / decode at the bit
widths and ragged D the fixtures never reach.

RaBitQ-1 (csrc/rabitq.hip, rabitq_internal.h): every kernel mivq_rabitq_encode dispatches to, by D
and by the alignment of x and of the centroid, must write the same bytes, and those bytes are held
to the exact-sum reference with bounds derived from the summation shape.

Row counts are 9 to 13 (4 rows per workgroup: the last workgroup is partial) unless stated.
"""

import math

import numpy as np
import pytest
import torch

import _rabitq_encode_rule as R

pytestmark = pytest.mark.gpu

ERQ_DIMS = (1, 7, 9, 37, 64, 100, 520)
FILL = 0xA5


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _h(t):
    return t.cpu().numpy()


def _lv(B):
    return R.synthetic_levels(B)


# ============================================================================== Extended RaBitQ
# ------------------------------------------------------------------------------ normalize
def _normalize_rows(D, dtype):
    """11 rows about a centroid of f32-representable values whose even dimensions are 0 (a tiny
    residual survives only against a 0 centroid entry)."""
    rng = np.random.default_rng([D, 11])
    c = rng.standard_normal(D).astype(np.float32).astype(np.float64)
    c[::2] = 0.0
    X = np.empty((11, D), np.float64)
    X[:] = c + rng.standard_normal((11, D))
    X[2] = c                                                  # all-zero residual
    X[3] = c
    X[3, ::2] = rng.standard_normal(len(c[::2])) * 1e-20 / math.sqrt(D)  # 0 < norm ~ 1e-20 < 1e-12
    X[4] = rng.standard_normal(D) * 1e30
    X[5] = c
    X[5, ::2] = rng.standard_normal(len(c[::2])) * 1e-30
    X[6] = c
    X[6, (D - 1) // 2 * 2] += 1.5                             # one non-zero dimension
    X[7] = c
    X[7, 0] = -0.0 if D > 1 else 0.0
    return X.astype(dtype), c


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("D", ERQ_DIMS)
def test_erq_normalize(dev, D, dtype):
    """o equals r / max(nrm, 1e-12) bit for bit with the kernel's own nrm, r = x - c rounded once;
    nrm within (ceil(D / 64) + 8) * 2^-53 of the exact norm (R.norm_bound)."""
    from haag_vq import _native

    X, c = _normalize_rows(D, dtype)
    o, nrm = _native.extrabitq_normalize(_t(X, dev), _t(c, dev))
    o, nrm = _h(o), _h(nrm)
    r, _, nrm_ref = R.normalize_ref(X, c)
    assert nrm_ref[2] == 0.0 and 0.0 < nrm_ref[3] < 1e-15 and nrm_ref[4] > 1e29 and nrm_ref[6] == 1.5
    err, bound = np.abs(nrm - nrm_ref), R.norm_bound(D, nrm_ref)
    with np.errstate(invalid="ignore"):
        worst = np.nanmax(np.where(err == 0, 0.0, err / bound))
    print(f"\n[erq normalize] D={D} {np.dtype(dtype).name}: worst |nrm - exact| / bound {worst:.3f}")
    assert np.all(err <= bound), (err, bound)
    R.assert_same_bits(o, R.o_of(r, nrm), "o")
    assert not o[2].any() and np.all(np.abs(o[3]) < 1e-7)  # divided by the guard, not by the norm


# ------------------------------------------------------------------------------ quantize
def _quantize_rows(D, B, lv):
    """(s_raw (11, D), nrm (11,)): s Gaussian with entries beyond both outermost midpoints, a row in
    the lowest cell, a row in the highest, a row of zeros, a row that names every level; norms include 0, one that overflows f32."""
    rng = np.random.default_rng([D, B, 3])
    s = rng.standard_normal((11, D))
    far = rng.random((11, D)) < 0.1
    s[far] = np.where(rng.random(far.sum()) < 0.5, lv[0] - 1.0, lv[-1] + 1.0) * rng.uniform(1, 4, far.sum())
    s[0, 0], s[0, D - 1] = lv[0] - 2.0, lv[-1] + 2.0
    s[7] = lv[0] - rng.uniform(0.5, 50.0, D)
    s[8] = lv[-1] + rng.uniform(0.5, 50.0, D)
    s[9] = 0.0
    s[10] = np.resize(lv, D)  # every level once (where D allows), each exactly on itself
    nrm = rng.uniform(0.1, 10.0, 11)
    nrm[1], nrm[2], nrm[3], nrm[4] = 0.0, 1e39, 1e-42, 3.0e38  # f32: 0, inf, subnormal, near the top
    return s / np.sqrt(np.float64(D)), nrm


def _check_quantize(got, ref, D, B, nrm, what):
    ib = (D * B + 7) // 8
    np.testing.assert_array_equal(got[:, :ib], ref.codes[:, :ib], err_msg=f"{what}: index bytes")
    gn, gt = R.trailer(got, D, B)
    with np.errstate(over="ignore"):
        R.assert_same_bits(gn, nrm.astype(np.float32), f"{what}: f32 nrm")
    live = ref.den > R.EPS
    err, bound = np.abs(gt.astype(np.float64) - ref.t), R.t_bound(D, ref)
    assert np.all(err[live] <= bound[live]), (what, err, bound)
    R.assert_same_bits(gt[~live], np.ones((~live).sum(), np.float32), f"{what}: t where den <= 1e-12")
    with np.errstate(invalid="ignore"):
        return float(np.max(np.where(err == 0, 0.0, err / bound)[live], initial=0.0))


@pytest.mark.parametrize("D", ERQ_DIMS)
@pytest.mark.parametrize("B", range(1, 9))
def test_erq_quantize(dev, B, D):
    """Index bytes (pad bits included) byte for byte; f32 nrm exact; t within R.t_bound."""
    from haag_vq import _native

    lv = _lv(B)
    s_raw, nrm = _quantize_rows(D, B, lv)
    ref = R.quantize_ref(s_raw, lv, B, nrm)
    assert (ref.idx[7] == 0).all() and (ref.idx[8] == 2 ** B - 1).all()
    assert D < 2 ** B or len(np.unique(ref.idx)) == 2 ** B
    got = _h(_native.extrabitq_quantize(_t(s_raw, dev), _t(lv, dev), B, _t(nrm, dev)))
    worst = _check_quantize(got, ref, D, B, nrm, f"B={B} D={D}")
    print(f"\n[erq quantize] B={B} D={D}: worst |t - exact| / bound {worst:.3f}")


@pytest.mark.parametrize("D", ERQ_DIMS)
def test_erq_quantize_zero_denominator(dev, D):
    """A table with a 0 level and |s| < 0.4: every index names the 0 level, den = 0, t = 1.0f."""
    from haag_vq import _native

    rng = np.random.default_rng([D, 17])
    s_raw = rng.uniform(-0.39, 0.39, (9, D)) / np.sqrt(np.float64(D))
    nrm = rng.uniform(0.1, 10.0, 9)
    lv = R.ZERO_LEVEL_TABLE
    ref = R.quantize_ref(s_raw, lv, 2, nrm)
    assert (ref.idx == 1).all() and (ref.den == 0).all()
    got = _h(_native.extrabitq_quantize(_t(s_raw, dev), _t(lv, dev), 2, _t(nrm, dev)))
    np.testing.assert_array_equal(got, ref.codes)  # t = 1.0f exactly: whole rows


@pytest.mark.parametrize("B", [1, 3, 4, 8])
@pytest.mark.parametrize("D", [16, 64])
def test_erq_quantize_planted_ties(dev, D, B):
    """s exactly on every midpoint, one fp64 above and one below: indices q, q + 1, q."""
    from haag_vq import _native

    lv = R.lloyd_levels(B) if B <= 4 else _lv(B)
    s_raw, want = R.planted_ties(lv, D)
    n = len(s_raw)
    assert n % 4 != 0
    got = _h(_native.extrabitq_quantize(_t(s_raw, dev), _t(lv, dev), B, _t(np.ones(n), dev)))
    np.testing.assert_array_equal(R._erq_unpack(got, D, B), want)


@pytest.mark.parametrize("D,B", [(37, 3), (100, 5), (9, 7)])
def test_erq_quantize_writes_its_rows_only(dev, D, B):
    """out = buf[:9] of a 17-row buffer of 0xA5: every byte of the 9 rows is written (they equal the
    reference), no byte of the other 8 is."""
    from haag_vq import _native

    lv = _lv(B)
    s_raw, nrm = _quantize_rows(D, B, lv)
    s_raw, nrm = s_raw[:9], nrm[:9]
    ref = R.quantize_ref(s_raw, lv, B, nrm)
    buf = torch.full((17, R.code_size(D, B)), FILL, dtype=torch.uint8, device=dev)
    out = _native.extrabitq_quantize(_t(s_raw, dev), _t(lv, dev), B, _t(nrm, dev), out=buf[:9])
    assert out.data_ptr() == buf.data_ptr()
    got = _h(buf)
    assert (got[9:] == FILL).all()
    _check_quantize(got[:9], ref, D, B, nrm, f"B={B} D={D}")


# ------------------------------------------------------------------------------ dequantize, finish
@pytest.mark.parametrize("D", [7, 37, 100])
@pytest.mark.parametrize("B", range(1, 9))
def test_erq_dequantize_and_finish(dev, B, D):
    """Both bit for bit: (levels[idx] / sqrt(D)) * t and f32(y * nrm + c); a row with nrm = 0 and a
    row whose f32 nrm is inf among them."""
    from haag_vq import _native

    lv = _lv(B)
    s_raw, nrm = _quantize_rows(D, B, lv)
    codes = R.quantize_ref(s_raw, lv, B, nrm).codes
    fn, _ = R.trailer(codes, D, B)
    assert fn[1] == 0.0 and np.isinf(fn[2])
    o_hat = _h(_native.extrabitq_dequantize(_t(codes, dev), _t(lv, dev), B, D))
    R.assert_same_bits(o_hat, R.dequantize_ref(codes, lv, D, B), "o_hat")
    rng = np.random.default_rng([D, B, 5])
    y = rng.standard_normal((11, D))
    y[2, 0] = 0.0  # 0 * inf
    c = rng.standard_normal(D)
    out = _h(_native.extrabitq_finish(_t(y, dev), _t(codes, dev), _t(c, dev), B))
    want = R.finish_ref(y, codes, c, B)
    assert np.isnan(want[2, 0]) and np.isinf(want[2, 1:]).all() and (want[1] == c.astype(np.float32)).all()
    R.assert_same_bits(out, want, "finish")


# ------------------------------------------------------------------------------ end to end
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("D", [37, 100, 520])
@pytest.mark.parametrize("B", [3, 5, 6, 7])
def test_erq_encode_decode_odd_widths(dev, oracle, B, D, dtype):
    """extrabitq_encode against the oracle on Lloyd tables and a random rotation: indices equal
    except proven midpoint ties; the f32 nrm of every row and the f32 t of every row without a tie
    within one f32 ulp (the fp64 values behind them differ by rounding of the sums alone); the
    decode of the oracle's codes within 1e-6."""
    from haag_vq import _native

    rng = np.random.default_rng([D, B, 9])
    c = rng.standard_normal(D).astype(np.float32).astype(np.float64)
    X = (c + rng.standard_normal((11, D))).astype(dtype)
    X[6] = c
    P, lv = R.random_orthogonal(D, D + B), np.array(R.lloyd_levels(B))
    ref = oracle.extrabitq_encode(X, c, P, lv, B)
    got = _h(_native.extrabitq_encode(_t(X, dev), _t(c, dev), _t(P, dev), _t(lv, dev), B))
    bad = R._assert_ties_only(got, ref, X, c, P, lv, B)
    (gn, gt), (rn, rt) = R.trailer(got, D, B), R.trailer(ref, D, B)
    ok = np.setdiff1d(np.arange(len(X)), bad[:, 0])
    np.testing.assert_allclose(gn, rn, rtol=2.0 ** -23, atol=0)
    np.testing.assert_allclose(gt[ok], rt[ok], rtol=2.0 ** -23, atol=0)
    assert gn[6] == 0.0 and (6 not in ok or gt[6] == 0.0)
    want = oracle.extrabitq_decode(ref, c, P, lv, B)
    dec = _h(_native.extrabitq_decode(_t(ref, dev), _t(c, dev), _t(P, dev), _t(lv, dev), B))
    np.testing.assert_allclose(dec, want, rtol=1e-6, atol=1e-6 * np.abs(want).max())


# ============================================================================== RaBitQ-1
# D -> the kernel the aligned launch is meant to reach (rabitq.hip: ni = D / 512, the first of
# 6, 4, 3, 2 that divides ni picks G) and the trips of its `for (i0 = 0; i0 < ni; i0 += G)` loop.
# A centroid one float into its buffer takes every such D to the vector kernel, x one float into
# its buffer to the generic kernel.
WIDE_CASES = {
    512: "vector kernel (ni = 1: none of 6, 4, 3, 2 divides it)",
    1024: "wide<2>, one trip",
    1536: "wide<3>, one trip",
    2048: "wide<4>, one trip",
    2560: "vector kernel (ni = 5)",
    3072: "wide<6>, one trip",
    4096: "wide<4>, two trips",
    4608: "wide<3>, three trips",
    5120: "wide<2>, five trips",
    6144: "wide<6>, two trips",
}
# ragged and small D: the generic kernel, but 520 (d % 4 == 0, aligned x) the vector kernel
SMALL_DIMS = (1, 7, 9, 37, 520)
SPECIAL, ORDINARY = (10, 12), (0, 1, 9, 11, 13)  # rows holding a NaN / overflowing; rows around them


def _rq1_rows(D, metric, centroid):
    """14 rows (9 for the wide D): Gaussian rows, the degenerate rows (each clear of the two
    FLT_EPSILON guards: its sums are exact in any order), and past row 9 a NaN row and a 1e30 row
    between ordinary ones.  c[0] = 0.25 and c[1] = 0 so that the planted residuals are exact."""
    rng = np.random.default_rng([D, metric, int(centroid)])
    X = rng.standard_normal((14, D)).astype(np.float32)
    c = None
    base = np.zeros(D, np.float32)
    if centroid:
        c = rng.standard_normal(D).astype(np.float32)
        c[0] = 0.25
        c[1:2] = 0.0
        base = c
        X += c
    X[2] = base                                   # residual exactly zero
    X[3] = base
    X[3, 0] = base[0] + np.float32(2.0 ** -12)    # l2 = 2^-24 = 0.5 FLT_EPSILON: inv_norm = 1
    X[4] = base
    X[4, 0] = base[0] + np.float32(2.0 ** -11)    # l2 = 2^-22 = 2 FLT_EPSILON: inv_norm = 1 / sqrt(l2)
    X[5] = base - np.abs(rng.standard_normal(D).astype(np.float32)) - np.float32(2.0 ** -10)  # all bits 0, dp > 0
    X[6] = base
    X[6, min(1, D - 1)] = -0.0 if (c is None or D > 1) else base[0]  # x = -0.0 against c = 0: bit 0
    X[7] = base
    X[7, D - 1] = base[D - 1] + np.float32(3.0)   # one non-zero dimension, in the last byte
    X[10, 3 % D] = np.nan
    X[12] = (rng.standard_normal(D) * 1e30).astype(np.float32)
    X[12, 0] = 2e30
    return X, c


def _offset_view(a, dev):
    """The values of a in a tensor that starts one float into its buffer."""
    a = np.ascontiguousarray(a, np.float32)
    buf = torch.zeros(a.size + 1, dtype=torch.float32, device=dev)
    buf[1:] = _t(a.reshape(-1), dev)
    v = buf[1:].view(*a.shape)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def _rq1_launches(dev, X, c, metric):
    """name -> code rows of rabitq_encode on the same values: everything 16-byte aligned, the
    centroid misaligned (with a centroid), x misaligned."""
    from haag_vq import _native

    xa, ca = _t(X, dev), None if c is None else _t(c, dev)
    assert xa.data_ptr() % 16 == 0 and (ca is None or ca.data_ptr() % 16 == 0)
    out = {"aligned": _h(_native.rabitq_encode(xa, ca, metric))}
    if c is not None:
        out["centroid+4B"] = _h(_native.rabitq_encode(xa, _offset_view(c, dev), metric))
    out["x+4B"] = _h(_native.rabitq_encode(_offset_view(X, dev), ca, metric))
    return out


def _check_rq1(dev, oracle, X, c, metric, D, got, what):
    from haag_vq import _native

    n = len(X)
    ref = R.rabitq1_ref(X, c, metric)
    bits, f0, f1 = R.rabitq1_split(got, D)
    np.testing.assert_array_equal(bits, ref.bits, err_msg=what)
    rows = np.array([i for i in range(n) if i not in SPECIAL])
    r0, r1 = R.rabitq1_ratios(f0, f1, ref, metric, R.gamma_wave(D), rows)
    print(f"\n[rabitq-1 encode] D={D} {'L2' if metric == 1 else 'IP'} {what}: worst error / bound "
          f"f0 {r0.max():.3f}, f1 {r1.max():.3f} (bounds {R.gamma_wave(D):.2e}, "
          f"{2 * R.gamma_wave(D) + 8 * R.U32:.2e} relative)")
    assert r0.max() <= 1.0 and r1.max() <= 1.0, (what, r0, r1)
    # the degenerate rows, whose sums are exact in any order: the factors themselves
    z = np.float32(0.0)
    assert f1[2] == z and f1[6] == z and not bits[5].any() and not bits[6].any()
    assert metric == 0 or f0[2] == z
    if n > 12:  # non-finite where the oracle's are, the rows around them untouched by it
        _, o0, o1 = R.rabitq1_split(oracle.rabitq_encode(X, c, metric), D)
        for i in SPECIAL:
            assert np.isfinite(f0[i]) == np.isfinite(o0[i]) and np.isnan(f0[i]) == np.isnan(o0[i]), (what, i)
            assert np.isfinite(f1[i]) == np.isfinite(o1[i]) and np.isnan(f1[i]) == np.isnan(o1[i]), (what, i)
        assert np.isnan(f0[10]) and np.isnan(f1[10]) and not np.isfinite(f0[12]) and np.isinf(f1[12])
        clean = X.copy()
        clean[list(SPECIAL)] = 0.0
        alone = _h(_native.rabitq_encode(_t(clean, dev), None if c is None else _t(c, dev), metric))
        np.testing.assert_array_equal(got[list(ORDINARY)], alone[list(ORDINARY)], err_msg=what)


@pytest.mark.parametrize("centroid", [True, False], ids=["centroid", "none"])
@pytest.mark.parametrize("metric", [1, 0], ids=["l2", "ip"])
@pytest.mark.parametrize("D", sorted(WIDE_CASES))
def test_rabitq1_encode_dispatch(dev, oracle, D, metric, centroid):
    """The three kernel bodies (wide or its fallback; vector; generic) write identical bytes, trailer
    included, and those bytes meet the exact-sum reference: bits exact, factors within the bounds."""
    X, c = _rq1_rows(D, metric, centroid)
    X = np.ascontiguousarray(np.concatenate([X[:8], X[13:14]]))  # n = 9; the NaN / 1e30 rows: see the small D
    got = _rq1_launches(dev, X, c, metric)
    for name, codes in got.items():
        np.testing.assert_array_equal(codes, got["aligned"], err_msg=f"D={D} ({WIDE_CASES[D]}): {name} vs aligned")
    _check_rq1(dev, oracle, X, c, metric, D, got["aligned"], WIDE_CASES[D])


@pytest.mark.parametrize("centroid", [True, False], ids=["centroid", "none"])
@pytest.mark.parametrize("metric", [1, 0], ids=["l2", "ip"])
@pytest.mark.parametrize("D", SMALL_DIMS + tuple(sorted(WIDE_CASES)))
def test_rabitq1_encode_ragged_and_nonfinite(dev, oracle, D, metric, centroid):
    """14 rows, a NaN row and an overflowing row between ordinary ones: ragged D through the generic
    kernel (520: and the vector kernel), and the wide D again, through all their kernels.  The
    launches agree (the payload of a NaN factor aside), then the reference; the non-finite rows
    leave their neighbours' bytes as they are without them."""
    X, c = _rq1_rows(D, metric, centroid)
    got = _rq1_launches(dev, X, c, metric)
    for name, codes in got.items():
        R.assert_same_bits(R.rabitq1_split(codes, D)[1], R.rabitq1_split(got["aligned"], D)[1], f"D={D} {name} f0")
        R.assert_same_bits(R.rabitq1_split(codes, D)[2], R.rabitq1_split(got["aligned"], D)[2], f"D={D} {name} f1")
        np.testing.assert_array_equal(R.rabitq1_split(codes, D)[0], R.rabitq1_split(got["aligned"], D)[0])
    _check_rq1(dev, oracle, X, c, metric, D, got["aligned"], "aligned")


@pytest.mark.parametrize("D", [37, 1024])
def test_rabitq1_encode_writes_its_rows_only(dev, D):
    """out = buf[:9] of a 17-row buffer of 0xA5: the other 8 rows stay untouched."""
    from haag_vq import _native

    X, c = _rq1_rows(D, 1, True)
    X = X[:9]
    want = _h(_native.rabitq_encode(_t(X, dev), _t(c, dev), 1))
    buf = torch.full((17, D // 8 + (D % 8 != 0) + 8), FILL, dtype=torch.uint8, device=dev)
    out = _native.rabitq_encode(_t(X, dev), _t(c, dev), 1, out=buf[:9])
    assert out.data_ptr() == buf.data_ptr()
    got = _h(buf)
    assert (got[9:] == FILL).all()
    np.testing.assert_array_equal(got[:9], want)


@pytest.mark.parametrize("D", [7, 37, 520, 1024])
def test_rabitq1_decode_with_centroid(dev, oracle, D):
    """rabitq_decode with a centroid, D % 8 != 0 among the widths: the oracle's floats bit for bit."""
    from haag_vq import _native

    X, c = _rq1_rows(D, 1, True)
    codes = oracle.rabitq_encode(X[:10], c, 1)
    want = oracle.rabitq_decode(codes, D, c)
    got = _h(_native.rabitq_decode(_t(codes, dev), D, _t(c, dev)))
    R.assert_same_bits(got, want, f"D={D}")
