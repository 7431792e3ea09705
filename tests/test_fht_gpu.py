"""GPU: the fast Hadamard rotation against the rule of _fht_rule.py, the fused Extended RaBitQ
kernels against the staged composition bit for bit, the fht quantizer against the numpy pipeline,
and its search.  D <= 2048 in multiples of 64 with a register layout (256, 768, 1536, 2048 here)
rotate in registers, every other D (2049 is the first past the boundary) in LDS."""

import numpy as np
import pytest
import torch

import _fht_rule as F
import _search_rule as R

pytestmark = pytest.mark.gpu


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@pytest.mark.parametrize("inverse", (False, True))
@pytest.mark.parametrize("n", (1, 67))
@pytest.mark.parametrize("D", (1, 2, 3, 37, 64, 65, 128, 256, 768, 1536, 2048, 2049, 16384))
def test_rotate_matches_the_rule(dev, D, n, inverse):
    from haag_vq import _native

    rng = np.random.default_rng(D + n)
    x = rng.standard_normal((n, D))
    if n > 2:
        x[1] = 0.0
        x[2] = np.eye(D)[D // 3]
    signs = F.draw_signs(7, D)
    want = F.apply(x, signs, inverse)
    got = _native.fht_rotate(_t(x, dev), _t(signs, dev), inverse)
    err = np.abs(got.cpu().numpy() - want).max(axis=1).astype(np.float64)
    tol = F.bound(D) * np.linalg.norm(x, axis=1)
    print(f"D={D} n={n} inverse={inverse}: max err / bound {np.max(err / np.maximum(tol, 1e-300)):.3f}")
    assert np.all(err <= tol)
    buf = _t(x, dev)
    assert _native.fht_rotate(buf, _t(signs, dev), inverse, out=buf) is buf and torch.equal(buf, got)  # in place


@pytest.mark.parametrize("f64", (False, True))
@pytest.mark.parametrize("B", (1, 4, 8))
@pytest.mark.parametrize("D", (37, 64, 1536, 2049))
def test_fused_equals_staged_bit_for_bit(dev, D, B, f64):
    from haag_vq import _native as N

    rng = np.random.default_rng(D * 8 + B)
    X = (rng.standard_normal((67, D)) + 0.5).astype(np.float64 if f64 else np.float32)
    c = X.mean(axis=0).astype(np.float64)
    X[5] = c.astype(X.dtype)
    c = X[5].astype(np.float64)                                  # row 5 is the centroid: nrm = 0
    x, c, signs = _t(X, dev), _t(c, dev), _t(F.draw_signs(B, D), dev)
    lv = _t(np.sort(rng.standard_normal(1 << B)), dev)
    o, nrm = N.extrabitq_normalize(x, c)
    assert nrm[5] == 0
    staged = N.extrabitq_quantize(N.fht_rotate(o, signs), lv, B, nrm)
    codes = N.extrabitq_encode_fht(x, c, signs, lv, B)
    assert torch.equal(codes, staged)
    y = N.fht_rotate(N.extrabitq_dequantize(codes, lv, B, D), signs, inverse=True)
    assert torch.equal(N.extrabitq_decode_fht(codes, c, signs, lv, B).view(torch.int32),
                       N.extrabitq_finish(y, codes, c, B).view(torch.int32))


@pytest.mark.parametrize("D", (37, 1536))
def test_quantizer_matches_the_numpy_pipeline(dev, D):
    from haag_vq.methods.extended_rabitq import ExtendedRaBitQuantizer

    X, c, signs, levels = F.case(D)
    q = ExtendedRaBitQuantizer(4, seed=3, rotation="fht")
    q.fit(X)
    assert np.array_equal(q.signs, signs) and np.array_equal(q.levels, levels)
    codes = q.compress(X)
    ib = D // 2 + D % 2
    assert codes.shape == (len(X), ib + 8)
    got = np.stack((codes[:, :ib] >> 4, codes[:, :ib] & 15), axis=2).reshape(len(X), -1)[:, :D]
    idx, s, nrm, t = F.encode(X, c, signs, levels)
    mids = 0.5 * (levels[:-1] + levels[1:])
    diff = got != idx
    near = np.abs(s[diff].astype(np.float64)[:, None] - mids).min(axis=1) if diff.any() else np.zeros(0)
    assert np.all(near <= F.bound(D) * np.sqrt(D)), "an index differs away from a level midpoint"
    keep = ~diff.any(axis=1)
    print(f"D={D}: {diff.sum()} tie indices in {(~keep).sum()} of {len(X)} rows")
    assert (~keep).sum() <= 0.01 * len(X)
    trailer = np.ascontiguousarray(codes[:, ib:]).view(np.float32)
    assert np.array_equal(trailer[keep, 0], nrm.astype(np.float32)[keep])
    assert np.array_equal(trailer[keep, 1], t.astype(np.float32)[keep])
    want = F.decode(idx, nrm, t, c, signs, levels).astype(np.float32)
    assert np.all(np.abs(q.decompress(codes) - want)[keep] <= np.spacing(np.abs(want))[keep])


@pytest.mark.parametrize("metric", ("l2", "ip"))
@pytest.mark.parametrize("nq", (1, 16))
def test_search_and_files(dev, tmp_path, nq, metric):
    from haag_vq import _native as N
    from haag_vq.methods.extended_rabitq import ExtendedRaBitQuantizer
    from haag_vq.methods.search import ExtendedRaBitQFlatIndex, FlatQuantizedIndex

    rng = np.random.default_rng(nq)
    X = (rng.standard_normal((1000, 37)) + 0.3).astype(np.float32)
    Q = (rng.standard_normal((nq, 37)) + 0.3).astype(np.float32)
    idx = ExtendedRaBitQFlatIndex(ExtendedRaBitQuantizer(4, rotation="fht"))
    idx.fit(X, metric)
    q, codes = idx.quantizer, idx._codes
    ids, dists = idx.search_with_scores(Q, 10)

    c, signs, lv = q._state()
    nrm = codes[:, -8:-4].contiguous().view(torch.float32).to(torch.float64)
    yh = (N.extrabitq_dequantize(codes, lv, 4, 37) * nrm).float()
    d, i = N.flat_search(q.rotate_queries(Q, metric), yh, 10, N.METRIC_L2 if metric == "l2" else N.METRIC_INNER_PRODUCT)
    if metric == "ip":
        d = -d + (_t(Q, dev).to(torch.float64) @ c).to(torch.float32)[:, None]
    assert np.array_equal(i.cpu().numpy().view(np.uint32), ids)
    assert np.array_equal(d.cpu().numpy().view(np.uint32), dists.view(np.uint32))
    R.Judge(Q, q.decompress(codes).cpu().numpy().astype(np.float64), metric, 10).check(ids, dists, f"fht {metric}")

    idx.save(tmp_path / "fht.npz")
    with np.load(tmp_path / "fht.npz") as z:
        assert "signs" in z and "P" not in z and str(z["rotation"]) == "fht"
    back = ExtendedRaBitQFlatIndex(ExtendedRaBitQuantizer(1))
    back.load(tmp_path / "fht.npz")
    b_ids, b_d = back.search_with_scores(Q, 10)
    assert np.array_equal(b_ids, ids) and np.array_equal(b_d.view(np.uint32), dists.view(np.uint32))
    plain, direct = FlatQuantizedIndex(ExtendedRaBitQuantizer(1)), FlatQuantizedIndex(q)
    plain.load(tmp_path / "fht.npz")
    direct._codes, direct._N, direct._D, direct._metric = codes, 1000, 37, metric
    for a, b in zip(plain.search_with_scores(Q, 10), direct.search_with_scores(Q, 10)):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("case", F.BOUNDS_CASES, ids=repr)
def test_buffer_contract(dev, oracle, case):
    """No stray write, no input written, no dependence on what the outputs held, at exact buffer sizes."""
    import _bounds as B

    B.run_case(case, dev, oracle)
