"""GPU: the rank-aware quantizer's kernels bit for bit against the numpy rule
(tests/_rankaware_rule.py), the composed compress / decompress / fit against the reference's
fixture (tests/golden/rankaware_golden.npz), and the round trip through FlatQuantizedIndex."""

import numpy as np
import pytest
import torch

import _rankaware_rule as RR

pytestmark = pytest.mark.gpu

U = RR.U
ROWS = (0, 1, 129)


@pytest.fixture(scope="module")
def z(golden_dir):
    return RR.load_golden(golden_dir)


@pytest.fixture(scope="module")
def X():
    return {name: RR.inputs(name) for name in RR.CASES}


def _dev_state(st, dev):
    from haag_vq import _native

    return _native.rankaware_state(st.mu, st.V, st.cb, st.bits, st.pos, st.code_size, dev)


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _quantize(Y, ds, dev):
    from haag_vq import _native

    return _native.rankaware_quantize(_t(Y, dev), ds).cpu().numpy()


def _dequantize(codes, ds, dev):
    from haag_vq import _native

    return _native.rankaware_dequantize(_t(codes, dev), ds).cpu().numpy()


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ------------------------------------------------------------------ the kernels alone
@pytest.mark.parametrize("d", (64, 37))
@pytest.mark.parametrize("dtype", (np.float32, np.float64))
def test_center_exact(dev, dtype, d):
    from haag_vq import _native

    rng = np.random.default_rng([d, 1])
    mu = rng.standard_normal(d)
    for n in ROWS:
        x = (rng.standard_normal((n, d)) * 3).astype(dtype)
        got = _native.rankaware_center(_t(x, dev), _t(mu, dev)).cpu().numpy()
        assert _same_bits(got, x.astype(np.float64) - mu), (n, d)


@pytest.mark.parametrize("d", (64, 37))
def test_finish_exact(dev, d):
    from haag_vq import _native

    rng = np.random.default_rng([d, 2])
    mu = rng.standard_normal(d)
    for n in ROWS:
        zz = rng.standard_normal((n, d)) * 3
        got = _native.rankaware_finish(_t(zz, dev), _t(mu, dev)).cpu().numpy()
        assert _same_bits(got, (zz + mu).astype(np.float32)), (n, d)


@pytest.mark.parametrize("packing", RR.PACKINGS)
@pytest.mark.parametrize("name", list(RR.CASES))
def test_quantize_equals_the_rule_on_fixture_states(dev, z, X, name, packing):
    st = RR.fixture_state(z, name, packing)
    ds = _dev_state(st, dev)
    Y = RR.project(X[name], st)
    want = RR.pack(RR.indices(Y, st), st)
    assert np.array_equal(_quantize(Y, ds, dev), want)
    for n in ROWS:
        assert np.array_equal(_quantize(Y[:n], ds, dev), want[:n]), n


def _planted(st):
    """Rows that put every boundary of every dimension, and its two fp64 neighbours, into Y,
    then -inf, +inf and NaN rows: (Y, number of finite rows)."""
    nb = max(2 ** int(st.bits.max()) - 1, 1)
    B = np.zeros((nb, st.D))
    for d in np.flatnonzero(st.bits):
        b = RR.boundaries(st, d)
        B[:len(b), d] = b
        B[len(b):, d] = b[-1]
    rows = [B, np.nextafter(B, np.inf), np.nextafter(B, -np.inf)]
    tail = [np.full((1, st.D), v) for v in (-np.inf, np.inf, np.nan)]
    return np.concatenate(rows + tail), 3 * nb


@pytest.mark.parametrize("packing", RR.PACKINGS)
@pytest.mark.parametrize("name", ("w08", "odd37"))
def test_quantize_on_the_boundaries(dev, z, name, packing):
    st = RR.fixture_state(z, name, packing)
    Y, nf = _planted(st)
    got = _quantize(Y, _dev_state(st, dev), dev)
    assert np.array_equal(got, RR.pack(RR.indices(Y, st), st))
    idx = RR.unpack(got, st)
    nb = nf // 3
    for d in np.flatnonzero(st.bits):  # on a boundary: the lower index; one ulp above: the upper
        k = 2 ** int(st.bits[d]) - 1
        assert np.array_equal(idx[:k, d], np.arange(k)) and np.array_equal(idx[nb:nb + k, d], np.arange(k) + 1)
        assert np.array_equal(idx[2 * nb:2 * nb + k, d], np.arange(k))
    top = 2 ** st.bits - 1
    assert np.all(idx[nf] == 0) and np.array_equal(idx[nf + 1], top) and np.array_equal(idx[nf + 2], top)


@pytest.mark.parametrize("packing", RR.PACKINGS)
@pytest.mark.parametrize("name", list(RR.CASES))
def test_dequantize_equals_the_lookup(dev, z, name, packing):
    st = RR.fixture_state(z, name, packing)
    ds = _dev_state(st, dev)
    codes = z[f"{name}_{packing}_codes"]
    want = RR.lookup(RR.unpack(codes, st), st)
    assert _same_bits(_dequantize(codes, ds, dev), want)
    noisy = codes | ~RR.field_mask(st)          # every bit of no field set
    assert _same_bits(_dequantize(noisy, ds, dev), want)
    for n in ROWS:
        assert _same_bits(_dequantize(codes[:n], ds, dev), want[:n]), n


def test_any_byte_pattern_stays_inside_the_tables(dev, z):
    st = RR.fixture_state(z, "w08", "ffd")
    codes = np.random.default_rng(3).integers(0, 256, size=(130, st.code_size), dtype=np.uint8)
    codes[0], codes[1] = 0, 255
    assert _same_bits(_dequantize(codes, _dev_state(st, dev), dev), RR.lookup(RR.unpack(codes, st), st))


@pytest.mark.parametrize("packing", RR.PACKINGS)
def test_wide_synthetic_state(dev, packing):
    """D = 1536, widths cycling 0..8: code rows past 256 bytes, 87,000 levels."""
    st = RR.synthetic_state(np.arange(1536) % 9, packing, seed=1)
    assert st.code_size > 256
    ds = _dev_state(st, dev)
    Y = np.random.default_rng(4).standard_normal((130, 1536)) * 4
    idx = RR.indices(Y, st)
    want = RR.pack(idx, st)
    got = _quantize(Y, ds, dev)
    assert np.array_equal(got, want)
    assert _same_bits(_dequantize(want, ds, dev), RR.lookup(idx, st))


@pytest.mark.parametrize("bits", ([3, 5, 2, 1], [0, 0, 1, 0, 0], [8, 7, 0, 6, 5, 4, 3, 2, 1]))
def test_small_states_and_unaligned_rows(dev, bits):
    """A last field that ends mid-byte; one 1-bit dimension among zeros (code_size 1); and code
    rows that start one byte off a 16-byte line."""
    from haag_vq import _native

    st = RR.synthetic_state(bits, "dense", seed=2)
    assert st.code_size == (sum(bits) + 7) // 8
    ds = _dev_state(st, dev)
    Y = np.random.default_rng(5).standard_normal((130, len(bits))) * 3
    idx = RR.indices(Y, st)
    want = RR.pack(idx, st)
    assert np.array_equal(_quantize(Y, ds, dev), want)
    assert _same_bits(_dequantize(want, ds, dev), RR.lookup(idx, st))
    buf = torch.full((130 * st.code_size + 2,), 0xAA, dtype=torch.uint8, device=dev)
    out = buf[1:-1].view(130, st.code_size)
    _native.rankaware_quantize(_t(Y, dev), ds, out=out)
    host = buf.cpu().numpy()
    assert host[0] == 0xAA and host[-1] == 0xAA and np.array_equal(host[1:-1].reshape(130, -1), want)
    assert _same_bits(_native.rankaware_dequantize(out, ds).cpu().numpy(), RR.lookup(idx, st))


# ------------------------------------------------------------------ composed paths against the fixture
@pytest.mark.parametrize("packing", RR.PACKINGS)
@pytest.mark.parametrize("name", list(RR.CASES))
def test_compress_against_the_reference(dev, z, X, name, packing):
    st = RR.fixture_state(z, name, packing)
    q = RR.fixture_quantizer(z, name, packing)
    x = X[name]
    codes = q.compress(x)
    assert isinstance(codes, np.ndarray) and codes.dtype == np.uint8 and codes.shape == (len(x), st.code_size)
    got = RR.unpack(codes, st)
    assert np.array_equal(RR.pack(got, st), codes)       # bits of no field are 0
    Y = (x.astype(np.float64) - st.mu) @ st.V            # numpy's projection, as the reference's
    ref = RR.unpack(z[f"{name}_{packing}_codes"], st)
    problems = RR.tie_problems(got, ref, Y, x, st)
    print(f"{name} {packing}: {(got != ref).sum()} of {got.size} indices differ from the reference's")
    assert not problems, problems[:5]
    ct = q.compress(torch.from_numpy(x).to(dev))         # tensor in, tensor out
    assert isinstance(ct, torch.Tensor) and ct.is_cuda and np.array_equal(ct.cpu().numpy(), codes)
    assert np.array_equal(q.compress(x.astype(np.float64)), codes)   # f32 values, centred in fp64 either way
    q._stage_bytes = 50 * st.D * 24                      # the chunked host path: 50 rows a chunk
    assert np.array_equal(q.compress(x), codes)


@pytest.mark.parametrize("packing", RR.PACKINGS)
@pytest.mark.parametrize("name", list(RR.CASES))
def test_decompress_against_the_reference(dev, z, name, packing):
    st = RR.fixture_state(z, name, packing)
    q = RR.fixture_quantizer(z, name, packing)
    codes, rec = z[f"{name}_{packing}_codes"], z[f"{name}_rec"]
    got = q.decompress(codes)
    assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.shape == rec.shape
    slack = RR.decode_slack(rec, RR.lookup(RR.unpack(codes, st), st), st.D)
    err = np.abs(got.astype(np.float64) - rec)
    print(f"{name} {packing}: max error / slack {np.max(err / slack):.3f}, {np.count_nonzero(err)} of {err.size} differ")
    assert np.all(err <= slack)
    gt = q.decompress(torch.from_numpy(codes).to(dev))
    assert isinstance(gt, torch.Tensor) and gt.is_cuda and gt.dtype == torch.float32
    assert _same_bits(gt.cpu().numpy(), got)
    q._stage_bytes = 50 * st.D * 24
    assert _same_bits(q.decompress(codes), got)


# ------------------------------------------------------------------ fit on the device
def test_fit_on_the_device(dev, z, X):
    from haag_vq.methods.rank_aware_quantization import RankAwareQuantizer

    name = RR.FIT_CASE
    c, x = RR.CASES[name], X[name]
    N, D = x.shape
    q = RankAwareQuantizer(c["avg_bits"], alpha=c["alpha"], max_bits=c["max_bits"])
    q.fit(x)
    x64 = x.astype(np.float64)
    ax = np.abs(x64)

    # moments: fp64 sums of N terms in any order, against numpy's
    n, S, G = q._moments(x)
    e_mu = (N + 2) * U * ax.mean(axis=0)
    assert n == N and np.all(np.abs(S / N - x64.sum(axis=0) / N) <= e_mu)
    assert _same_bits(q.mu, S / N) and np.all(np.abs(q.mu - z[f"{name}_mu"]) <= e_mu)
    e_G = 2 * (N + 2) * U * (ax.T @ ax)
    assert np.all(np.abs(G - x64.T @ x64) <= e_G)
    for other in (torch.from_numpy(x).to(dev), x64):    # a device tensor, f64 rows (torch's fp64 product)
        n2, S2, G2 = q._moments(other)
        assert n2 == N and np.all(np.abs(S2 - S) <= 2 * N * e_mu) and np.all(np.abs(G2 - G) <= e_G)

    # var: Weyl.  |lambda_k(C) - lambda_k(C')| <= ||C - C'||_2 <= ||E||_F with E the elementwise
    # bound on C = G / N - mu mu^T between the two sides (G, mu as above, then the division, the
    # outer product and the subtraction rounded once on each side), plus the backward error of the
    # two eigh calls, each of order D u ||C||.
    mu = np.abs(q.mu)
    C = G / N - np.outer(q.mu, q.mu)
    E = e_G / N + np.outer(mu, e_mu) + np.outer(e_mu, mu) + 4 * U * (np.abs(G) / N + np.outer(mu, mu))
    w_bound = np.linalg.norm(E) + 4 * D * U * np.linalg.norm(C)
    assert np.all(np.abs(q.var - z[f"{name}_var"]) <= w_bound)
    assert np.array_equal(q.bits, z[f"{name}_bits"]) and q.bits.dtype == np.int64
    assert q.code_size == int(z[f"{name}_dense_code_size"]) and np.array_equal(q._offsets, z[f"{name}_offsets"])
    assert q.D == D and len(q.cb) == D and all(len(t) == 2 ** b for t, b in zip(q.cb, q.bits))
    assert len(q._levels) == c["max_bits"] + 1 and q._Dg.shape == (c["max_bits"] + 1,)

    # V: orthonormal columns (entries of V^T V are length-D dot products of unit vectors, (D + 2) u
    # each, plus eigh's own loss of orthogonality, of the same order), and an eigen-residual no
    # more than 4x the one numpy's eigh leaves on the same C
    assert np.max(np.abs(q.V.T @ q.V - np.eye(D))) <= 8 * (D + 2) * U
    w, Vn = np.linalg.eigh(C)
    own = np.max(np.abs(C @ Vn - Vn * w))
    res = np.max(np.abs(C @ q.V - q.V * q.var))
    print(f"eigen-residual {res:.3e}, numpy's own {own:.3e}")
    assert res <= 4 * own

    # compress with the device-fitted state against the rule on that same state
    st = RR.make_state(q.mu, q.V, q.bits, q.cb, q.field_positions(), q.code_size)
    codes = q.compress(x)
    Y = RR.project(x, st)
    assert not RR.tie_problems(RR.unpack(codes, st), RR.indices(Y, st), Y, x, st)
    rec = q.decompress(codes)
    slack = RR.decode_slack(rec, RR.lookup(RR.unpack(codes, st), st), D)
    assert np.all(np.abs(rec.astype(np.float64) - RR.decompress(codes, st)) <= slack)


def test_zero_budget_has_no_code(dev):
    from haag_vq.methods.rank_aware_quantization import RankAwareQuantizer

    q = RankAwareQuantizer(0.0, max_bits=2)
    q.fit(RR.gaussian_rows(50, 8, 0.1, 0))
    assert q.code_size == 0 and not q.bits.any()
    with pytest.raises(ValueError, match="0 bits"):
        q.compress(np.zeros((1, 8), np.float32))


# ------------------------------------------------------------------ through the index
@pytest.mark.parametrize("packing", RR.PACKINGS)
def test_flat_index_round_trip(dev, tmp_path, packing):
    from haag_vq import _native
    from haag_vq.methods.rank_aware_quantization import RankAwareQuantizer
    from haag_vq.methods.search.flat_quantized_index import FlatQuantizedIndex

    x = RR.gaussian_rows(500, 64, 1e-2, 7)
    Q = RR.gaussian_rows(20, 64, 1e-2, 8)
    idx = FlatQuantizedIndex(RankAwareQuantizer(avg_bits=4, max_bits=4, packing=packing))
    idx.fit(x)
    ids, dists = idx.search_with_scores(Q, 10)
    assert ids.shape == (20, 10) and ids.dtype == np.uint32 and dists.dtype == np.float32
    assert idx.memory_footprint() == 500 * idx.quantizer.code_size
    xh = idx.quantizer.decompress(idx._codes)
    d2, i2 = _native.flat_search(torch.from_numpy(Q).to(dev), xh, 10)
    assert np.array_equal(i2.cpu().numpy().view(np.uint32), ids) and _same_bits(d2.cpu().numpy(), dists)
    mse = float(np.mean((xh.cpu().numpy() - x) ** 2))
    assert mse < 0.05 * float(np.mean((x - x.mean(axis=0)) ** 2)), mse   # 4 bits a dimension: a real reconstruction
    idx.save(tmp_path / "ra.npz")
    back = FlatQuantizedIndex(RankAwareQuantizer(avg_bits=1))
    back.load(tmp_path / "ra.npz")
    assert type(back.quantizer) is RankAwareQuantizer and back.quantizer.packing == packing
    ids2, dists2 = back.search_with_scores(Q, 10)
    assert np.array_equal(ids2, ids) and _same_bits(dists2, dists)
