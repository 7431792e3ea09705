"""GPU: mivq_rankaware_flat_search bit for bit against mivq_flat_search over the dequantised
levels, and RankAwareQuantizer.search_codes / RankAwareFlatIndex against the reference's
reconstructions (tests/golden/rankaware_golden.npz) under the bounds of _rankaware_search_rule."""

import numpy as np
import pytest
import torch

import _rankaware_rule as RR
import _rankaware_search_rule as RS

pytestmark = pytest.mark.gpu

METRICS = ("l2", "ip")


@pytest.fixture(scope="module")
def z(golden_dir):
    return RR.load_golden(golden_dir)


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _dev_state(st, dev):
    from haag_vq import _native

    return _native.rankaware_state(st.mu, st.V, st.cb, st.bits, st.pos, st.code_size, dev)


def _mt(metric):
    from haag_vq import _native

    return _native.METRIC_L2 if metric == "l2" else _native.METRIC_INNER_PRODUCT


def _bits(t):
    return t.cpu().numpy().view(np.uint32)


def _same(qy, codes, ds, k, metric="l2", id_offset=0):
    """Runs the code search and decode + flat_search; asserts ids and distance bit patterns
    equal; returns the code search's (dists, ids) as numpy (ids uint32)."""
    from haag_vq import _native

    d, i = _native.rankaware_flat_search(qy, codes, ds, k, _mt(metric), id_offset=id_offset)
    yh = _native.rankaware_dequantize(codes.contiguous(), ds).float()
    d2, i2 = _native.flat_search(qy, yh, k, _mt(metric), id_offset=id_offset)
    assert d.shape == (qy.shape[0], k) and d.dtype == torch.float32 and i.dtype == torch.int32
    assert np.array_equal(_bits(i), _bits(i2)), (tuple(qy.shape), tuple(codes.shape), k, metric)
    assert np.array_equal(_bits(d), _bits(d2)), (tuple(qy.shape), tuple(codes.shape), k, metric)
    return d.cpu().numpy(), _bits(i)


def _random(st, n, nq, dev, seed=0, scale=2.0):
    """Random bytes as codes (every byte pattern is valid) and Gaussian rotated queries."""
    rng = np.random.default_rng([st.D, n, nq, seed])
    codes = rng.integers(0, 256, size=(n, st.code_size), dtype=np.uint8)
    qy = (rng.standard_normal((nq, st.D)) * scale).astype(np.float32)
    return _t(codes, dev), _t(qy, dev)


# ------------------------------------------------------------------ the kernel, bit for bit
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("packing", RR.PACKINGS)
@pytest.mark.parametrize("name", list(RR.CASES))
def test_fixture_states(dev, z, name, packing, metric):
    st = RR.fixture_state(z, name, packing)
    qy = RS.rotate(RS.queries(name), st, metric).astype(np.float32)
    _same(_t(qy, dev), _t(z[f"{name}_{packing}_codes"], dev), _dev_state(st, dev), RS.K, metric)


WIDE = {
    "cycle1536": (np.arange(1536) % 9, 300),        # every width, 87,000 levels
    "all8_1536": (np.full(1536, 8), 200),           # tables of 1.5 MB, 1536-byte rows
    "odd37": (np.arange(37) % 9, 300),
    "one_bit": ([0, 0, 1, 0, 0], 300),              # code_size 1
    "mid_byte": ([3, 5, 2, 1], 300),                # the last field ends mid-byte
}


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("packing", RR.PACKINGS)
@pytest.mark.parametrize("case", list(WIDE))
def test_synthetic_states_random_bytes(dev, case, packing, metric):
    bits, n = WIDE[case]
    st = RR.synthetic_state(bits, packing, seed=11)
    ds = _dev_state(st, dev)
    for nq in (3, 17):
        codes, qy = _random(st, n, nq, dev)
        _same(qy, codes, ds, 10, metric)


@pytest.mark.parametrize("metric", METRICS)
def test_odd_code_size_off_alignment(dev, metric):
    """5-byte rows that start one byte off a 16-byte line, scan and tiled."""
    st = RR.synthetic_state([8, 7, 0, 6, 5, 4, 3, 2, 1], "dense", seed=12)
    assert st.code_size == 5
    ds = _dev_state(st, dev)
    for n, nq in ((301, 3), (4100, 17)):
        codes, qy = _random(st, n, nq, dev)
        buf = torch.zeros(n * 5 + 2, dtype=torch.uint8, device=dev)
        off = buf[1:-1].view(n, 5)
        off.copy_(codes)
        assert off.data_ptr() % 2 == 1 and off.is_contiguous()
        d, i = _same(qy, off, ds, 10, metric)
        d2, i2 = _same(qy, codes, ds, 10, metric)
        assert np.array_equal(i, i2) and np.array_equal(d.view(np.uint32), d2.view(np.uint32))


@pytest.mark.parametrize("metric", METRICS)
def test_sizes(dev, z, metric):
    """nq, k and n at their edges, n < k and n == 0 (missing slots: +inf, 0xFFFFFFFF)."""
    st = RR.fixture_state(z, "w08", "dense")
    ds = _dev_state(st, dev)
    for n in (0, 1, 129):
        for nq in (1, 3, 17):
            codes, qy = _random(st, n, nq, dev)
            for k in (1, 10, 256):
                d, i = _same(qy, codes, ds, k, metric)
                m = min(n, k)
                assert np.all(np.isinf(d[:, m:])) and np.all(d[:, m:] > 0) and np.all(i[:, m:] == 0xFFFFFFFF)
                assert np.all(i[:, :m] < max(n, 1)) and np.all(np.isfinite(d[:, :m]))


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("packing", RR.PACKINGS)
def test_both_paths(dev, packing, metric):
    """Either side of the scan / tiled choice (flat_use_tiled: nq >= 16 and n >= 4096), and scans
    whose workgroups own one tile of rows (n = 5000) and several (n = 200,003: 768 chunks of 261
    rows, tiles of 256)."""
    st = RR.synthetic_state(np.arange(37) % 9, packing, seed=13)
    ds = _dev_state(st, dev)
    for nq, n in ((15, 4095), (16, 4096), (15, 4096), (16, 4095), (3, 5000), (3, 200_003)):
        codes, qy = _random(st, n, nq, dev)
        _same(qy, codes, ds, 10, metric)


def test_long_rows_walk_several_tiles(dev):
    """1536-byte rows: 60-odd rows fit a tile, so 1500 rows of one query block are walked in
    chunks of several tiles when 64 query blocks share the grid."""
    st = RR.synthetic_state(np.full(1536, 8), "dense", seed=14)
    ds = _dev_state(st, dev)
    codes, qy = _random(st, 1500, 250, dev)
    _same(qy, codes, ds, 10, "l2")


@pytest.mark.parametrize("metric", METRICS)
def test_ties_go_to_the_smaller_id(dev, metric):
    st = RR.synthetic_state(np.arange(37) % 9, "dense", seed=15)
    ds = _dev_state(st, dev)
    for n, nq in ((600, 3), (4200, 16)):
        codes, qy = _random(st, n // 3, nq, dev)
        codes = codes.repeat(3, 1).contiguous()               # row r equals rows r + n / 3, r + 2 n / 3
        d, i = _same(qy, codes, ds, 12, metric)
        for row_d, row_i in zip(d, i.astype(np.int64)):
            assert np.all(np.diff(row_d) >= 0)
            tied = row_d[1:] == row_d[:-1]
            assert tied.sum() >= 6 and np.all(row_i[1:][tied] > row_i[:-1][tied])
            assert np.array_equal(row_i[0:3] % (n // 3), np.repeat(row_i[0] % (n // 3), 3))


def test_id_offset_past_2_31(dev):
    st = RR.synthetic_state(np.arange(37) % 9, "ffd", seed=16)
    ds = _dev_state(st, dev)
    off = 2 ** 31 + 5
    for n, nq in ((300, 3), (4100, 16)):
        codes, qy = _random(st, n, nq, dev)
        d0, i0 = _same(qy, codes, ds, 10)
        d, i = _same(qy, codes, ds, 10, id_offset=off)
        assert np.array_equal(i.astype(np.int64), i0.astype(np.int64) + off)
        assert np.array_equal(d.view(np.uint32), d0.view(np.uint32))


@pytest.mark.parametrize("packing", RR.PACKINGS)
def test_bits_of_no_field_are_ignored(dev, z, packing):
    st = RR.fixture_state(z, "odd37", packing)          # 111 bits of fields: spare bits in either packing
    ds = _dev_state(st, dev)
    codes = z[f"odd37_{packing}_codes"]
    noisy = codes | ~RR.field_mask(st)
    assert not np.array_equal(noisy, codes)
    qy = _t(RS.rotate(RS.queries("odd37"), st).astype(np.float32), dev)
    d, i = _same(qy, _t(codes, dev), ds, RS.K)
    d2, i2 = _same(qy, _t(noisy, dev), ds, RS.K)
    assert np.array_equal(i, i2) and np.array_equal(d.view(np.uint32), d2.view(np.uint32))
    big = np.tile(codes, (25, 1))                             # the tiled path
    bigq = _t(np.tile(qy.cpu().numpy(), (2, 1)), dev)
    d, i = _same(bigq, _t(big, dev), ds, RS.K)
    d2, i2 = _same(bigq, _t(big | ~RR.field_mask(st), dev), ds, RS.K)
    assert np.array_equal(i, i2) and np.array_equal(d.view(np.uint32), d2.view(np.uint32))


@pytest.mark.parametrize("metric", METRICS)
def test_nan_query_ranks_as_inf(dev, metric):
    st = RR.synthetic_state(np.arange(37) % 9, "dense", seed=17)
    ds = _dev_state(st, dev)
    for n, nq in ((300, 3), (4100, 16)):
        codes, qy = _random(st, n, nq, dev)
        qy[1, 5] = float("nan")
        d, i = _same(qy, codes, ds, 10, metric)
        assert np.all(np.isinf(d[1])) and np.array_equal(i[1], np.arange(10, dtype=np.uint32))
        assert np.all(np.isfinite(d[0])) and np.all(np.isfinite(d[2]))


def test_state_without_lv32_is_served(dev, z):
    """A state built positionally (without the f32 table) gets it derived and cached."""
    from haag_vq import _native

    st = RR.fixture_state(z, "odd37", "dense")
    ds = _dev_state(st, dev)
    bare = _native.RankAwareState(*ds[:7])
    assert bare.lv32 is None and ds.lv32 is not None and ds.lv32.dtype == torch.float32
    assert np.array_equal(ds.lv32.cpu().numpy(), np.concatenate(st.cb).astype(np.float32))
    codes, qy = _random(st, 200, 3, dev)
    d, i = _same(qy, codes, ds, 10)
    d2, i2 = _same(qy, codes, bare, 10)
    assert np.array_equal(i, i2) and np.array_equal(d.view(np.uint32), d2.view(np.uint32))
    assert _native.rankaware_lv32(bare) is _native.rankaware_lv32(bare)


def test_native_argument_checks(dev, z):
    from haag_vq import _native

    st = RR.fixture_state(z, "odd37", "dense")
    ds = _dev_state(st, dev)
    codes, qy = _random(st, 50, 3, dev)
    with pytest.raises(ValueError):
        _native.rankaware_flat_search(qy[:, :-1].contiguous(), codes, ds, 5)
    with pytest.raises(ValueError):
        _native.rankaware_flat_search(qy, codes[:, :-1].contiguous(), ds, 5)
    with pytest.raises(ValueError):
        _native.rankaware_flat_search(qy, codes.to(torch.int32), ds, 5)
    with pytest.raises(ValueError):
        _native.rankaware_flat_search(qy.double(), codes, ds, 5)
    with pytest.raises(ValueError):
        _native.rankaware_flat_search(qy, codes, ds, 257)
    with pytest.raises(ValueError):
        _native.rankaware_flat_search(qy, codes, ds, 5, metric=7)


# ------------------------------------------------------------------ the public interface
def _index(q, codes, N, D, metric, dev, cls=None):
    from haag_vq.methods.search import RankAwareFlatIndex

    idx = (cls or RankAwareFlatIndex)(q)
    idx._codes, idx._N, idx._D, idx._metric = _t(codes, dev), N, D, metric
    return idx


@pytest.mark.parametrize("packing", RR.PACKINGS)
@pytest.mark.parametrize("name", list(RR.CASES))
def test_distances_against_the_reference(dev, z, name, packing):
    """Truth: the fp64 distance from q to the reference's reconstruction.  Every returned
    distance is within l2_slack of the truth of its id, and no row left out is closer than the
    farthest returned one by more than the two slacks."""
    st = RR.fixture_state(z, name, packing)
    q = RR.fixture_quantizer(z, name, packing)
    codes, rec = z[f"{name}_{packing}_codes"], z[f"{name}_rec"].astype(np.float64)
    Q = RS.queries(name)
    N, D = rec.shape
    A, Yh = RS.rotate(Q, st), RS.levels(codes, st)
    d, i = q.search_codes(_t(codes, dev), Q, RS.K)
    assert isinstance(d, torch.Tensor) and d.is_cuda and d.dtype == torch.float32 and i.dtype == torch.int32
    ids, dists = _index(q, codes, N, D, "l2", dev).search_with_scores(Q, RS.K)
    assert ids.dtype == np.uint32 and dists.dtype == np.float32 and ids.shape == (RS.NQ, RS.K)
    assert np.array_equal(ids, _bits(i)) and np.array_equal(dists.view(np.uint32), _bits(d))
    worst = 0.0
    for j in range(RS.NQ):
        truth = ((rec - Q[j].astype(np.float64)) ** 2).sum(axis=1)
        slack = RS.l2_slack(A[j], Yh, D)
        worst = max(worst, float(np.max(np.abs(dists[j] - truth[ids[j].astype(np.int64)]) / slack[ids[j].astype(np.int64)])))
        problems = RS.l2_problems(ids[j], dists[j], truth, slack)
        assert not problems, (j, problems)
    print(f"{name} {packing}: worst |dist - truth| / slack {worst:.4f}")


@pytest.mark.parametrize("packing", RR.PACKINGS)
@pytest.mark.parametrize("name", list(RR.CASES))
def test_ip_scores_against_the_reference(dev, z, name, packing):
    st = RR.fixture_state(z, name, packing)
    q = RR.fixture_quantizer(z, name, packing)
    codes, rec = z[f"{name}_{packing}_codes"], z[f"{name}_rec"].astype(np.float64)
    Q = RS.queries(name)
    N, D = rec.shape
    truth = Q.astype(np.float64) @ rec.T
    A, Yh = RS.rotate(Q, st, "ip"), RS.levels(codes, st)
    ids, scores = _index(q, codes, N, D, "ip", dev).search_with_scores(Q, RS.K)
    d, i = q.search_codes(codes, Q, RS.K, metric="ip")
    assert np.array_equal(ids, _bits(i)) and np.array_equal(scores.view(np.uint32), _bits(d))
    mu_norm = float(np.linalg.norm(st.mu))
    for j in range(RS.NQ):
        slack = RS.ip_slack(A[j], Yh, D, mu_norm)
        r = ids[j].astype(np.int64)
        assert len(set(r.tolist())) == RS.K and np.all(np.diff(scores[j]) <= 0)
        assert np.all(np.abs(scores[j] - truth[j][r]) <= slack[r]), j
        rest = np.setdiff1d(np.arange(N), r)
        low = r[int(np.argmin(truth[j][r]))]
        assert np.all(truth[j][rest] <= truth[j][low] + slack[rest] + slack[low]), j


def test_rotate_queries(dev, z):
    st = RR.fixture_state(z, "mse100", "dense")
    q = RR.fixture_quantizer(z, "mse100", "dense")
    Q = RS.queries("mse100")
    for metric in METRICS:
        got = q.rotate_queries(Q, metric)
        assert isinstance(got, torch.Tensor) and got.is_cuda and got.dtype == torch.float32 and got.shape == Q.shape
        want = RS.rotate(Q, st, metric)
        # one f32 rounding plus the difference of two fp64 sums of D terms
        tol = 2.0 ** -24 * np.abs(want) + (st.D + 2) * 2.0 ** -52 * np.linalg.norm(Q.astype(np.float64) - st.mu, axis=1)[:, None]
        tol += (st.D + 2) * 2.0 ** -52 * np.linalg.norm(st.mu)
        assert np.all(np.abs(got.cpu().numpy().astype(np.float64) - want) <= tol), metric
        assert np.array_equal(_bits(q.rotate_queries(_t(Q, dev), metric)), _bits(got))
    with pytest.raises(ValueError):
        q.rotate_queries(Q, "cosine")
    with pytest.raises(ValueError):
        q.rotate_queries(Q[:, :-1])


def test_inputs_k_edges_large_k_and_files(dev, z, tmp_path):
    from haag_vq.methods.rank_aware_quantization import RankAwareQuantizer
    from haag_vq.methods.search import FlatQuantizedIndex, RankAwareFlatIndex

    name = "w08"
    q = RR.fixture_quantizer(z, name, "ffd")
    codes = z[f"{name}_ffd_codes"]
    N, D = RR.CASES[name]["N"], RR.CASES[name]["D"]
    Q = RS.queries(name)
    idx = _index(q, codes, N, D, "l2", dev)
    ids, dists = idx.search_with_scores(Q, RS.K)

    # numpy and tensor inputs agree
    ids_t, dists_t = idx.search_with_scores(_t(Q, dev), RS.K)
    assert np.array_equal(ids_t, ids) and np.array_equal(dists_t.view(np.uint32), dists.view(np.uint32))
    assert np.array_equal(idx.search(Q, RS.K), ids)
    d, i = q.search_codes(codes, _t(Q, dev), RS.K)
    assert np.array_equal(_bits(i), ids) and np.array_equal(_bits(d), dists.view(np.uint32))

    # k = 0 is empty, k > N clamps
    e_ids, e_d = idx.search_with_scores(Q, 0)
    assert e_ids.shape == (RS.NQ, 0) and e_ids.dtype == np.uint32 and e_d.shape == (RS.NQ, 0) and e_d.dtype == np.float32
    few = _index(q, codes[:7], 7, D, "l2", dev)
    c_ids, c_d = few.search_with_scores(Q, 50)
    assert c_ids.shape == (RS.NQ, 7) and np.all(np.sort(c_ids, axis=1) == np.arange(7)) and np.all(np.isfinite(c_d))

    # above the kernel's k the inherited decode path answers: FlatQuantizedIndex's result
    plain = _index(q, codes, N, D, "l2", dev, cls=FlatQuantizedIndex)
    b_ids, b_d = idx.search_with_scores(Q, 300)
    p_ids, p_d = plain.search_with_scores(Q, 300)
    assert b_ids.shape == (RS.NQ, 300) and np.array_equal(b_ids, p_ids)
    assert np.array_equal(b_d.view(np.uint32), p_d.view(np.uint32))

    # files: a round trip keeps the results, and each class loads the other's file
    idx.save(tmp_path / "ra.npz")
    plain.save(tmp_path / "plain.npz")
    for path in ("ra.npz", "plain.npz"):
        back = RankAwareFlatIndex(RankAwareQuantizer(avg_bits=1))
        back.load(tmp_path / path)
        assert type(back.quantizer) is RankAwareQuantizer and back.quantizer.packing == "ffd"
        assert back.memory_footprint() == N * q.code_size
        r_ids, r_d = back.search_with_scores(Q, RS.K)
        assert np.array_equal(r_ids, ids) and np.array_equal(r_d.view(np.uint32), dists.view(np.uint32)), path
    other = FlatQuantizedIndex(RankAwareQuantizer(avg_bits=1))
    other.load(tmp_path / "ra.npz")
    o_ids, o_d = other.search_with_scores(Q, RS.K)
    p_ids, p_d = plain.search_with_scores(Q, RS.K)
    assert np.array_equal(o_ids, p_ids) and np.array_equal(o_d.view(np.uint32), p_d.view(np.uint32))
    assert idx.reconstruction_mse(RR.inputs(name)) == plain.reconstruction_mse(RR.inputs(name))

    # a file of another quantizer is refused and leaves the index as it was
    from haag_vq.methods.scalar_quantization import ScalarQuantizer

    sq = FlatQuantizedIndex(ScalarQuantizer(8))
    sq.fit(RR.inputs(name))
    sq.save(tmp_path / "sq.npz")
    with pytest.raises(ValueError, match="RankAwareQuantizer"):
        idx.load(tmp_path / "sq.npz")
    assert idx.quantizer is q and np.array_equal(idx.search(Q, RS.K), ids)


def test_fit_and_search_end_to_end(dev):
    """fit on the device, then the code search agrees with the decode path on every row the fp32
    bound settles."""
    from haag_vq.methods.rank_aware_quantization import RankAwareQuantizer
    from haag_vq.methods.search import FlatQuantizedIndex, RankAwareFlatIndex

    x = RR.gaussian_rows(500, 64, 1e-2, 7)
    Q = RR.gaussian_rows(20, 64, 1e-2, 8)
    idx = RankAwareFlatIndex(RankAwareQuantizer(avg_bits=4, max_bits=4))
    idx.fit(x)
    assert idx.memory_footprint() == 500 * idx.quantizer.code_size
    ids, dists = idx.search_with_scores(Q, 10)
    plain = FlatQuantizedIndex(idx.quantizer)
    plain._codes, plain._N, plain._D, plain._metric = idx._codes, 500, 64, "l2"
    p_ids, p_d = plain.search_with_scores(Q, 10)
    xh = idx.quantizer.decompress(idx._codes).cpu().numpy().astype(np.float64)
    q = idx.quantizer
    st = RR.make_state(q.mu, q.V, q.bits, q.cb, q.field_positions(), q.code_size)
    A, Yh = RS.rotate(Q, st), RS.levels(idx._codes.cpu().numpy(), st)
    for j in range(20):
        truth = ((xh - Q[j].astype(np.float64)) ** 2).sum(axis=1)
        slack = RS.l2_slack(A[j], Yh, 64)
        assert not RS.l2_problems(ids[j], dists[j], truth, slack), j
        assert not RS.l2_problems(p_ids[j], p_d[j], truth, slack), j
    print(f"id lists equal to the decode path's in {np.mean(ids == p_ids):.3f} of the positions")
