"""GPU: mivq_extrabitq_flat_search bit for bit against mivq_flat_search over
(float)(mivq_extrabitq_dequantize(codes) * nrm), on the streaming and the tiled path, and
ExtendedRaBitQuantizer.search_codes / ExtendedRaBitQFlatIndex against the reference's fixture
(erq1 / erq4 of tests/golden/search_golden.npz) and the bounds of _rankaware_search_rule."""

import numpy as np
import pytest
import torch

import _extrabitq_search_rule as ES
import _rankaware_search_rule as RS
import _search_rule as R

pytestmark = pytest.mark.gpu

METRICS = ("l2", "ip")
# (B, D): row bytes 22 (tail dimensions, fields across bytes, 2-byte aligned rows), 52 (fields
# across words, 4-byte loads), 40 (8-byte loads), 92 (4-byte loads), and the other widths
STREAM = ((3, 37), (5, 70), (4, 64), (7, 96), (1, 128), (2, 100), (6, 64), (8, 96))
TILED = ((1, 64), (3, 37), (4, 64), (5, 70), (8, 32))


@pytest.fixture(scope="module")
def sg(golden_dir):
    with np.load(golden_dir / "search_golden.npz") as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def erq(golden_dir):
    with np.load(golden_dir / "extrabitq_golden.npz") as z:
        return {k: z[k] for k in z.files}


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _mt(metric):
    from haag_vq import _native

    return _native.METRIC_L2 if metric == "l2" else _native.METRIC_INNER_PRODUCT


def _bits(t):
    return t.cpu().numpy().view(np.uint32)


def _levels(B, dev):
    """2^B ascending levels, irregular like Lloyd's."""
    rng = np.random.default_rng(100 + B)
    return _t(np.sort(rng.standard_normal(1 << B)) * 1.5, dev)


def _y_hat(codes, lv, B, D):
    """(float)(o_hat * nrm), the product in fp64 on the device."""
    from haag_vq import _native

    ib = codes.shape[1] - 8
    nrm = codes[:, ib:ib + 4].reshape(-1).clone().view(torch.float32).to(torch.float64)   # (n,), n = 0 too
    return (_native.extrabitq_dequantize(codes.contiguous(), lv, B, D) * nrm[:, None]).to(torch.float32)


def _same(qy, codes, lv, B, k, metric="l2", id_offset=0):
    """Runs the code search and dequantize + flat_search; asserts ids and distance bit patterns
    equal; returns the code search's (dists, ids) as numpy (ids uint32)."""
    from haag_vq import _native

    D = qy.shape[1]
    d, i = _native.extrabitq_flat_search(qy, codes, lv, B, k, _mt(metric), id_offset=id_offset)
    d2, i2 = _native.flat_search(qy, _y_hat(codes, lv, B, D), k, _mt(metric), id_offset=id_offset)
    assert d.shape == (qy.shape[0], k) and d.dtype == torch.float32 and i.dtype == torch.int32
    what = (B, tuple(qy.shape), tuple(codes.shape), k, metric)
    assert np.array_equal(_bits(i), _bits(i2)), what
    assert np.array_equal(_bits(d), _bits(d2)), what
    return d.cpu().numpy(), _bits(i)


def _random(B, D, n, nq, dev, seed=0):
    """Random fields with random finite nrm > 0 and t, and Gaussian rotated queries."""
    rng = np.random.default_rng([B, D, n, nq, seed])
    codes = ES.pack(rng.integers(0, 1 << B, size=(n, D)), rng.uniform(0.5, 4.0, n), rng.uniform(0.7, 1.3, n), B)
    qy = (rng.standard_normal((nq, D)) * 0.4).astype(np.float32)
    return _t(codes, dev), _t(qy, dev)


def _off_by_one(codes, dev):
    n, cs = codes.shape
    buf = torch.zeros(n * cs + 2, dtype=torch.uint8, device=dev)
    off = buf[1:-1].view(n, cs)
    off.copy_(codes)
    assert off.data_ptr() % 2 == 1 and off.is_contiguous()
    return off


# ------------------------------------------------------------------ the kernel, bit for bit
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("B,D", STREAM)
def test_streaming_path_bit_identical(dev, B, D, metric):
    lv = _levels(B, dev)
    for nq in (1, 3, 9):
        codes, qy = _random(B, D, 300, nq, dev)
        assert codes.shape[1] == ES.code_size(D, B)
        _same(qy, codes, lv, B, 10, metric)


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("B,D", TILED)
def test_tiled_path_bit_identical(dev, B, D, metric):
    codes, qy = _random(B, D, 4099, 33, dev)
    _same(qy, codes, _levels(B, dev), B, 10, metric)


@pytest.mark.parametrize("metric", METRICS)
def test_database_one_byte_off(dev, metric):
    """Rows that start one byte into their buffer: a streaming and a tiled case."""
    for (B, D), n, nq in (((4, 64), 300, 3), ((5, 70), 4099, 33)):
        lv = _levels(B, dev)
        codes, qy = _random(B, D, n, nq, dev)
        d, i = _same(qy, _off_by_one(codes, dev), lv, B, 10, metric)
        d2, i2 = _same(qy, codes, lv, B, 10, metric)
        assert np.array_equal(i, i2) and np.array_equal(d.view(np.uint32), d2.view(np.uint32))


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("B,D", ((3, 37), (8, 32), (1, 9)))
def test_hand_built_rows(dev, B, D, metric):
    """Codes written here, not by compress: all fields 0 and 2^B - 1, padding bits set, nrm = 0,
    t = NaN (ranks last, as +inf), and identical rows (ascending ids)."""
    rng = np.random.default_rng([B, D, 7])
    L = (1 << B) - 1
    lv = _levels(B, dev)
    for n, nq in ((300, 3), (4099, 17)):
        idx = rng.integers(0, L + 1, size=(n, D))
        nrm, t = rng.uniform(0.5, 4.0, n), rng.uniform(0.7, 1.3, n)
        idx[0], idx[1] = 0, L
        nrm[2] = 0.0
        t[3] = np.nan
        idx[5], nrm[5], t[5] = idx[4], nrm[4], t[4]
        idx[n - 1], nrm[n - 1], t[n - 1] = idx[4], nrm[4], t[4]
        codes = ES.pack(idx, nrm, t, B)
        qy = (rng.standard_normal((nq, D)) * 0.4).astype(np.float32)
        yh = ES.y_hat(codes, lv.cpu().numpy(), D, B)
        assert np.all(yh[2] == 0) and np.all(np.isnan(yh[3])) and np.array_equal(yh[4], yh[5])
        qy[0] = yh[4]                                   # query 0 sits on the identical rows
        d, i = _same(_t(qy, dev), _t(codes, dev), lv, B, n if n <= 256 else 256, metric)
        if (D * B) % 8:                                  # bits past D B in the last code byte are ignored
            noisy = ES.pack(idx, nrm, t, B, pad_ones=True)
            assert not np.array_equal(noisy, codes)
            d2, i2 = _same(_t(qy, dev), _t(noisy, dev), lv, B, n if n <= 256 else 256, metric)
            assert np.array_equal(i, i2) and np.array_equal(d.view(np.uint32), d2.view(np.uint32))
        # the rule's reconstruction is the device's
        assert np.array_equal(_y_hat(_t(codes, dev), lv, B, D).cpu().numpy(), yh, equal_nan=True)
        assert not np.any(i == 3)                        # the NaN row is +inf: behind 256 finite rows
        if metric == "l2":
            assert d[0][0] == 0.0 and list(i[0][:3]) == [4, 5, n - 1]
        for row_d, row_i in zip(d, i.astype(np.int64)):
            tied = row_d[1:] == row_d[:-1]
            assert np.all(np.diff(row_d) >= 0) and np.all(row_i[1:][tied] > row_i[:-1][tied])


def test_k_edges_and_missing_slots(dev):
    B, D = 4, 64
    lv = _levels(B, dev)
    codes, qy = _random(B, D, 300, 3, dev)
    for k in (1, 256):
        d, i = _same(qy, codes, lv, B, k)
        assert np.all(np.isfinite(d)) and np.all(i < 300)
    for n in (0, 7):                                     # k > N: (+inf, 0xFFFFFFFF) beyond the rows
        for nq in (2, 17):
            c, q = _random(B, D, n, nq, dev)
            for metric in METRICS:
                d, i = _same(q, c, lv, B, 10, metric)
                assert np.all(np.isinf(d[:, n:])) and np.all(d[:, n:] > 0) and np.all(i[:, n:] == 0xFFFFFFFF)
                assert np.all(np.isfinite(d[:, :n])) and np.all(np.sort(i[:, :n], axis=1) == np.arange(n))


def test_id_offset_up_to_the_last_id(dev):
    from haag_vq import _native

    B, D = 4, 64
    lv = _levels(B, dev)
    for n, nq in ((300, 3), (4099, 17)):
        codes, qy = _random(B, D, n, nq, dev)
        d0, i0 = _same(qy, codes, lv, B, 10)
        off = 2 ** 32 - 1 - n
        d, i = _same(qy, codes, lv, B, 10, id_offset=off)
        assert np.array_equal(i.astype(np.int64), i0.astype(np.int64) + off)
        assert np.array_equal(d.view(np.uint32), d0.view(np.uint32))
        with pytest.raises(ValueError, match="ids overflow"):
            _native.extrabitq_flat_search(qy, codes, lv, B, 10, id_offset=off + 1)


def test_native_argument_checks(dev):
    from haag_vq import _native

    B, D = 4, 64
    lv = _levels(B, dev)
    codes, qy = _random(B, D, 50, 3, dev)
    with pytest.raises(ValueError):
        _native.extrabitq_flat_search(qy[:, :-2].contiguous(), codes, lv, B, 5)   # (d = 63 has 40-byte rows too)
    with pytest.raises(ValueError):
        _native.extrabitq_flat_search(qy, codes[:, :-1].contiguous(), lv, B, 5)
    with pytest.raises(ValueError):
        _native.extrabitq_flat_search(qy, codes[:, ::2], lv, B, 5)
    with pytest.raises(ValueError):
        _native.extrabitq_flat_search(qy, codes.to(torch.int32), lv, B, 5)
    with pytest.raises(ValueError):
        _native.extrabitq_flat_search(qy.double(), codes, lv, B, 5)
    with pytest.raises(ValueError):
        _native.extrabitq_flat_search(qy, codes, lv[:-1].contiguous(), B, 5)
    with pytest.raises(ValueError, match=r"num_bits must be in \[1, 8\], got 9"):
        _native.extrabitq_flat_search(qy, codes, lv, 9, 5)
    with pytest.raises(ValueError):
        _native.extrabitq_flat_search(qy, codes, lv, B, 257)
    with pytest.raises(ValueError):
        _native.extrabitq_flat_search(qy, codes, lv, B, 5, metric=7)


# ------------------------------------------------------------------ the reference's fixture
def _fixture(name, sg, erq):
    from haag_vq.methods.extended_rabitq import ExtendedRaBitQuantizer

    c = R.CASES[name]
    t = f"b{c['bits']}"
    X, Q = R.inputs(name, erq["X"])
    assert R.sha(Q) == str(sg[f"{name}_Q_sha"]) and R.sha(erq[f"{t}_codes"]) == str(sg[f"{name}_codes_sha"])
    q = ExtendedRaBitQuantizer(num_bits=c["bits"], seed=0)      # as tests/test_search_golden.py::_model
    q.c, q.P, q.levels = erq[f"{t}_c"], erq[f"{t}_P"], erq[f"{t}_levels"]
    q.D = c["D"]
    return q, erq[f"{t}_codes"], Q, c


def _index(q, codes, N, D, metric, dev, cls=None):
    from haag_vq.methods.search import ExtendedRaBitQFlatIndex

    idx = (cls or ExtendedRaBitQFlatIndex)(q)
    idx._codes, idx._N, idx._D, idx._metric = _t(codes, dev), N, D, metric
    return idx


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("name", ("erq1", "erq4"))
def test_index_returns_the_reference_ids(dev, oracle, sg, erq, name, metric):
    q, codes, Q, c = _fixture(name, sg, erq)
    ids, dists = _index(q, codes, c["N"], c["D"], metric, dev).search_with_scores(Q, c["k"])
    assert ids.dtype == np.uint32 and dists.dtype == np.float32 and ids.shape == (c["nq"], c["k"])
    assert np.array_equal(ids, sg[f"{name}_{metric}_ids"])
    xh = oracle.extrabitq_decode(codes, q.c, q.P, q.levels, c["bits"])
    judge = R.Judge(Q, xh, metric, c["k"])
    judge.check(ids, dists, f"{name} {metric} ExtendedRaBitQFlatIndex")
    print(f"{name} {metric}: max |dist - key| / e {judge.ratio(ids, dists):.4f}")
    d, i = q.search_codes(_t(codes, dev), Q, c["k"], metric)
    assert isinstance(d, torch.Tensor) and d.is_cuda and d.dtype == torch.float32 and i.dtype == torch.int32
    assert np.array_equal(_bits(i), ids) and np.array_equal(_bits(d), dists.view(np.uint32))


# ------------------------------------------------------------------ the classes
@pytest.fixture(scope="module")
def fitted(dev):
    """2000 x 48 rows, B = 4, fitted once for the class tests: (index, X, Q)."""
    from haag_vq.methods.extended_rabitq import ExtendedRaBitQuantizer
    from haag_vq.methods.search import ExtendedRaBitQFlatIndex

    rng = np.random.default_rng(21)
    s = rng.uniform(0.2, 2.0, 48)
    X = (rng.standard_normal((2000, 48)) * s + 0.5).astype(np.float32)
    Q = (rng.standard_normal((20, 48)) * s + 0.5).astype(np.float32)
    idx = ExtendedRaBitQFlatIndex(ExtendedRaBitQuantizer(num_bits=4, seed=1))
    idx.fit(X)
    return idx, X, Q


def _plain(idx, metric="l2"):
    from haag_vq.methods.search import FlatQuantizedIndex

    plain = FlatQuantizedIndex(idx.quantizer)
    plain._codes, plain._N, plain._D, plain._metric = idx._codes, idx._N, idx._D, metric
    return plain


@pytest.mark.parametrize("metric", METRICS)
def test_fit_and_search_agree_with_the_decode_path(dev, fitted, metric, monkeypatch):
    idx, X, Q = fitted
    q = idx.quantizer
    N, D = 2000, 48
    assert idx.memory_footprint() == N * q.code_size and q.code_size == ES.code_size(D, 4)
    plain = _plain(idx, metric)
    p_ids, p_d = plain.search_with_scores(Q, 10)
    xh = q.decompress(idx._codes).cpu().numpy().astype(np.float64)

    calls = []
    real = type(q).decompress
    monkeypatch.setattr(type(q), "decompress", lambda self, c: (calls.append(len(c)), real(self, c))[1])
    idx._metric = metric
    try:
        ids, dists = idx.search_with_scores(Q, 10)
        assert not calls, "the database was decoded"
        plain.search_with_scores(Q, 10)
        assert calls == [N]                              # (the spy does see the decode path)
    finally:
        idx._metric = "l2"

    codes = idx._codes.cpu().numpy()
    A, Yh = ES.rotate(Q, q.c, q.P, metric), ES.y_hat(codes, q.levels, D, 4).astype(np.float64)
    c_norm = float(np.linalg.norm(q.c))
    for j in range(len(Q)):
        if metric == "l2":
            truth = ((xh - Q[j].astype(np.float64)) ** 2).sum(axis=1)
            slack = RS.l2_slack(A[j], Yh, D)
            assert not RS.l2_problems(ids[j], dists[j], truth, slack), j
            assert not RS.l2_problems(p_ids[j], p_d[j], truth, slack), j
        else:
            truth = xh @ Q[j].astype(np.float64)
            slack = RS.ip_slack(A[j], Yh, D, c_norm)
            # scores descending: the same rule on the negated scores
            assert not RS.l2_problems(ids[j], -dists[j], -truth, slack), j
            assert not RS.l2_problems(p_ids[j], -p_d[j], -truth, slack), j
    print(f"{metric}: id lists equal to the decode path's in {np.mean(ids == p_ids):.3f} of the positions")


def test_inputs_k_edges_large_k_and_files(dev, fitted, tmp_path):
    from haag_vq.methods.extended_rabitq import ExtendedRaBitQuantizer
    from haag_vq.methods.scalar_quantization import ScalarQuantizer
    from haag_vq.methods.search import ExtendedRaBitQFlatIndex, FlatQuantizedIndex

    idx, X, Q = fitted
    q = idx.quantizer
    N, D = 2000, 48
    plain = _plain(idx)
    ids, dists = idx.search_with_scores(Q, 10)

    # numpy and tensor inputs agree
    ids_t, dists_t = idx.search_with_scores(_t(Q, dev), 10)
    assert np.array_equal(ids_t, ids) and np.array_equal(dists_t.view(np.uint32), dists.view(np.uint32))
    assert np.array_equal(idx.search(Q, 10), ids)

    # k = 0 is empty, k > N clamps
    e_ids, e_d = idx.search_with_scores(Q, 0)
    assert e_ids.shape == (20, 0) and e_ids.dtype == np.uint32 and e_d.shape == (20, 0) and e_d.dtype == np.float32
    few = _index(q, idx._codes[:7].cpu().numpy(), 7, D, "l2", dev)
    c_ids, c_d = few.search_with_scores(Q, 50)
    assert c_ids.shape == (20, 7) and np.all(np.sort(c_ids, axis=1) == np.arange(7)) and np.all(np.isfinite(c_d))

    # above the kernel's k the inherited decode path answers: FlatQuantizedIndex's result
    b_ids, b_d = idx.search_with_scores(Q, 300)
    p_ids, p_d = plain.search_with_scores(Q, 300)
    assert b_ids.shape == (20, 300) and np.array_equal(b_ids, p_ids)
    assert np.array_equal(b_d.view(np.uint32), p_d.view(np.uint32))

    # files: a round trip keeps the results, and each class loads the other's file
    idx.save(tmp_path / "erq.npz")
    plain.save(tmp_path / "plain.npz")
    for path in ("erq.npz", "plain.npz"):
        back = ExtendedRaBitQFlatIndex(ExtendedRaBitQuantizer(num_bits=1))
        back.load(tmp_path / path)
        assert type(back.quantizer) is ExtendedRaBitQuantizer and back.quantizer.num_bits == 4
        assert back.memory_footprint() == N * q.code_size
        r_ids, r_d = back.search_with_scores(Q, 10)
        assert np.array_equal(r_ids, ids) and np.array_equal(r_d.view(np.uint32), dists.view(np.uint32)), path
    other = FlatQuantizedIndex(ExtendedRaBitQuantizer(num_bits=1))
    other.load(tmp_path / "erq.npz")
    o_ids, o_d = other.search_with_scores(Q, 10)
    p_ids, p_d = plain.search_with_scores(Q, 10)
    assert np.array_equal(o_ids, p_ids) and np.array_equal(o_d.view(np.uint32), p_d.view(np.uint32))

    # a file of another quantizer is refused and leaves the index as it was
    sq = FlatQuantizedIndex(ScalarQuantizer(8))
    sq.fit(X[:100])
    sq.save(tmp_path / "sq.npz")
    with pytest.raises(ValueError, match="ExtendedRaBitQuantizer"):
        idx.load(tmp_path / "sq.npz")
    assert idx.quantizer is q and np.array_equal(idx.search(Q, 10), ids)


def test_rotate_queries(dev, fitted):
    from haag_vq import _native

    idx, X, Q = fitted
    q = idx.quantizer
    D = 48
    for metric in METRICS:
        got64 = None
        for dt in (np.float32, np.float64):
            got = q.rotate_queries(Q.astype(dt), metric)
            assert isinstance(got, torch.Tensor) and got.is_cuda and got.dtype == torch.float32 and got.shape == Q.shape
            got64 = got if got64 is None else got64
            assert np.array_equal(_bits(got), _bits(got64))          # Q holds f32 values either way
        want = ES.rotate(Q, q.c, q.P, metric)
        shifted = Q.astype(np.float64) - (q.c if metric == "l2" else 0.0)
        # before the rounding: the same two calls, within (D + 2) 2^-53 ||q - c|| of the rule's sum
        c_dev, P_dev, _ = q._state()
        pre = _native.gemm_f64(_native.rankaware_center(_t(Q, dev), c_dev if metric == "l2" else torch.zeros_like(c_dev)),
                               P_dev, False)
        tol = (D + 2) * 2.0 ** -53 * np.linalg.norm(shifted, axis=1)[:, None]
        assert np.all(np.abs(pre.cpu().numpy() - want) <= tol), metric
        assert np.array_equal(_bits(pre.to(torch.float32)), _bits(got))   # rounded once
        assert np.array_equal(_bits(q.rotate_queries(_t(Q, dev), metric)), _bits(got))
    with pytest.raises(ValueError):
        q.rotate_queries(Q, "cosine")
    with pytest.raises(ValueError):
        q.rotate_queries(Q[:, :-1])
