"""GPU parity of the IVF / IVF-PQ entry points (libmivq, ivf.hip) against the CPU oracle, and
the reference's FaissIvfPqIndex tests (/root/reference/tests/test_faiss_ivfpq.py) run
against the MI355X class.

Every IVF kernel is deterministic and follows the canonical arithmetic of include/mivq.h,
so the comparisons are bit-exact: coarse distances, list assignment, bucket order, k-means
update, residuals, per-code terms and the final (dist, id) lists.
"""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _h(t):
    return t.detach().cpu().numpy()


def _clustered(rng, n, d, centers=16, spread=0.3):
    C = rng.standard_normal((centers, d)).astype(np.float32)
    X = C[rng.integers(0, centers, n)] + spread * rng.standard_normal((n, d)).astype(np.float32)
    return X.astype(np.float32)


@pytest.mark.parametrize("n,m,d,y_off", [
    pytest.param(*s, 0, id="-".join(map(str, s)))
    for s in [(300, 70, 32), (129, 65, 1536), (5, 3, 7), (1000, 256, 96), (64, 4096, 16)]
] + [pytest.param(129, 65, 64, 1, id="129-65-64-y_one_float_in")])  # y off 16 B: scalar fetches
@pytest.mark.parametrize("metric", [1, 0])
def test_pairwise_distances_bit_exact(dev, oracle, n, m, d, y_off, metric):
    from haag_vq import _native

    rng = np.random.default_rng(n + m + d)
    X = rng.standard_normal((n, d)).astype(np.float32)
    Y = rng.standard_normal((m, d)).astype(np.float32)
    Y[1] = X[0]  # an exact zero distance
    buf = torch.zeros(m * d + y_off, dtype=torch.float32, device=dev)
    buf[y_off:] = _t(Y.reshape(-1), dev)
    Yd = buf[y_off:].view(m, d)
    assert (Yd.data_ptr() % 16 != 0) == bool(y_off)
    got = _h(_native.pairwise_distances(_t(X, dev), Yd, metric))
    np.testing.assert_array_equal(got, oracle.pairwise(X, Y, metric))


@pytest.mark.parametrize("k", [1, 7, 64, 100, 256])
def test_topk_rows(dev, oracle, k):
    from haag_vq import _native

    rng = np.random.default_rng(k)
    D = rng.standard_normal((37, 300)).astype(np.float32)
    D[:, 10] = D[:, 3]          # ties -> smaller column first
    D[0, 5] = np.nan            # NaN ranks as +inf
    D[1, :] = np.inf
    dd, ii = _native.topk_rows(_t(D, dev), k)
    rd, ri = oracle.topk_rows(D, k)
    np.testing.assert_array_equal(_h(ii).view(np.uint32), ri)
    np.testing.assert_array_equal(_h(dd), rd)


def test_topk_rows_short_rows_pad(dev, oracle):
    from haag_vq import _native

    D = np.arange(12, dtype=np.float32).reshape(3, 4)[:, ::-1].copy()
    dd, ii = _native.topk_rows(_t(D, dev), 6)
    rd, ri = oracle.topk_rows(D, 6)
    np.testing.assert_array_equal(_h(ii).view(np.uint32), ri)
    np.testing.assert_array_equal(_h(dd), rd)


@pytest.mark.parametrize("n,K", [(0, 4), (1, 1), (5000, 37), (3000, 4096), (70000, 300), (1024, 2)])
def test_bucket_sort_stable(dev, oracle, n, K):
    from haag_vq import _native

    rng = np.random.default_rng(n + K)
    a = rng.integers(0, K, n).astype(np.int32)
    if n > 10:
        a[: n // 3] = 0  # a heavy bucket spanning many sort blocks
    offsets, order = _native.bucket_sort(_t(a, dev), K)
    ro, rord = oracle.bucket_sort(a, K)
    np.testing.assert_array_equal(_h(offsets), ro)
    np.testing.assert_array_equal(_h(order).view(np.uint32), rord)


@pytest.mark.parametrize("n,d,K", [(2000, 48, 16), (777, 1536, 33), (300, 5, 400)])
def test_centroid_update_bit_exact(dev, oracle, n, d, K):
    from haag_vq import _native

    rng = np.random.default_rng(n)
    X = rng.standard_normal((n, d)).astype(np.float32)
    a = rng.integers(0, K, n).astype(np.int32)
    C0 = rng.standard_normal((K, d)).astype(np.float32)
    offsets, order = _native.bucket_sort(_t(a, dev), K)
    C = _t(C0, dev)
    counts = torch.empty(K, dtype=torch.int32, device=dev)
    _native.centroid_update(_t(X, dev), offsets, order, C, counts)
    rc, rcnt = oracle.centroid_update(X, a.view(np.uint32), C0)
    np.testing.assert_array_equal(_h(counts), rcnt)
    np.testing.assert_array_equal(_h(C), rc)  # empty buckets keep their previous value


def test_residuals_and_gather(dev):
    from haag_vq import _native

    rng = np.random.default_rng(1)
    X = rng.standard_normal((500, 24)).astype(np.float32)
    C = rng.standard_normal((9, 24)).astype(np.float32)
    a = rng.integers(0, 9, 500).astype(np.int32)
    r = _h(_native.ivf_residuals(_t(X, dev), _t(C, dev), _t(a, dev)))
    np.testing.assert_array_equal(r, X - C[a])
    order = rng.permutation(500).astype(np.int32)
    g = _h(_native.gather_rows(_t(X, dev), _t(order, dev)))
    np.testing.assert_array_equal(g, X[order])
    b = rng.integers(0, 255, (500, 16)).astype(np.uint8)
    np.testing.assert_array_equal(_h(_native.gather_rows(_t(b, dev), _t(order, dev))), b[order])


@pytest.mark.parametrize("d,M,nbits", [(64, 8, 8), (1536, 16, 8), (16, 4, 4)])
def test_ivfpq_terms_bit_exact(dev, oracle, d, M, nbits):
    from haag_vq import _native

    rng = np.random.default_rng(d)
    ksub = 1 << nbits
    n, K = 400, 11
    Cpq = rng.standard_normal((M, ksub, d // M)).astype(np.float32)
    coarse = rng.standard_normal((K, d)).astype(np.float32)
    codes = rng.integers(0, ksub, (n, M)).astype(np.uint8)
    a = rng.integers(0, K, n).astype(np.int32)
    prep = _native.pq_prepare(_t(Cpq, dev), nbits)
    tau = _native.ivfpq_terms(_t(codes, dev), _t(Cpq, dev), prep, _t(coarse, dev), _t(a, dev), nbits)
    np.testing.assert_array_equal(_h(tau), oracle.ivfpq_terms(codes, Cpq, coarse, a.view(np.uint32)))


@pytest.mark.parametrize("metric", [1, 0])
@pytest.mark.parametrize("n,d,K,M,nbits,nprobe,k", [
    (3000, 64, 32, 8, 8, 5, 10),
    (2000, 96, 50, 16, 8, 50, 100),   # nprobe = K: every list
    (256, 16, 8, 4, 4, 4, 4),         # the reference test's shape
    (1500, 1536, 64, 16, 8, 16, 10),  # headline dimensionality
    (1200, 48, 12, 6, 8, 5, 10),      # M % 4 != 0: the scan's byte path and the torch-indexing branch of add
    (900, 30, 9, 10, 3, 9, 10),       # nbits = 3: pq_unpack on the add path, M % 4 != 0
])
def test_ivfpq_pipeline_bit_exact(dev, oracle, metric, n, d, K, M, nbits, nprobe, k):
    """Same coarse centroids and codebooks -> identical lists and (dist, id) results."""
    from haag_vq import _native
    from haag_vq.methods._ivf import IvfPq

    rng = np.random.default_rng(n + d)
    X = _clustered(rng, n, d)
    Q = _clustered(rng, 40, d)
    ksub = 1 << nbits
    coarse = X[rng.choice(n, K, replace=False)].copy()
    Cpq = (0.3 * rng.standard_normal((M, ksub, d // M))).astype(np.float32)
    idx = IvfPq(d, K, M, nbits, metric)
    idx.coarse = _t(coarse, dev)
    idx.pq = _t(Cpq, dev)
    idx.prep = _native.pq_prepare(idx.pq, nbits)
    idx.add(_t(X, dev))
    built = oracle.ivfpq_build(X, coarse, Cpq, metric)
    _, codes, offsets, list_codes, list_ids, tau = built
    L = idx.lists
    np.testing.assert_array_equal(_h(L.offsets), offsets)
    np.testing.assert_array_equal(_h(L.ids).view(np.uint32), list_ids)
    np.testing.assert_array_equal(_h(L.codes), list_codes)
    if metric == 1:
        np.testing.assert_array_equal(_h(L.tau), tau)
    dd, ii = idx.search(_t(Q, dev), k, nprobe)
    rd, ri = oracle.ivfpq_query(Q, coarse, Cpq, built, nprobe, k, metric)
    np.testing.assert_array_equal(_h(ii).view(np.uint32), ri)
    np.testing.assert_array_equal(_h(dd), rd)


@pytest.mark.parametrize("metric", [1, 0])
def test_ivfpq_empty_list_and_k_above_ntotal(dev, oracle, metric):
    """A coarse centroid no row is assigned to (far from positive data under L2, the most negative
    product under IP): its list is empty, every list is probed, and k = 40 > ntotal = 30 pads."""
    from haag_vq import _native
    from haag_vq.methods._ivf import IvfPq

    n, d, K, M, nbits, k, dead = 30, 16, 5, 4, 4, 40, 2
    rng = np.random.default_rng(30)
    X = (np.abs(rng.standard_normal((n, d))) + 1.0).astype(np.float32)
    Q = (np.abs(rng.standard_normal((7, d))) + 1.0).astype(np.float32)
    coarse = X[rng.choice(n, K, replace=False)].copy()
    coarse[dead] = -10.0
    Cpq = (0.3 * rng.standard_normal((M, 1 << nbits, d // M))).astype(np.float32)
    idx = IvfPq(d, K, M, nbits, metric)
    idx.coarse = _t(coarse, dev)
    idx.pq = _t(Cpq, dev)
    idx.prep = _native.pq_prepare(idx.pq, nbits)
    idx.add(_t(X, dev))
    built = oracle.ivfpq_build(X, coarse, Cpq, metric)
    offsets = _h(idx.lists.offsets)
    np.testing.assert_array_equal(offsets, built[2])
    assert offsets[dead + 1] == offsets[dead] and offsets[-1] == n
    dd, ii = idx.search(_t(Q, dev), k, K)
    rd, ri = oracle.ivfpq_query(Q, coarse, Cpq, built, K, k, metric)
    ii = _h(ii).view(np.uint32)
    np.testing.assert_array_equal(ii, ri)
    np.testing.assert_array_equal(_h(dd).view(np.uint32), rd.view(np.uint32))
    assert (np.sort(ii[:, :n], axis=1) == np.arange(n)).all()  # every row once, then padding
    assert (ii[:, n:] == _native.NO_ID).all() and np.isposinf(_h(dd)[:, n:]).all()


def test_ivfpq_incremental_add_matches_single_add(dev):
    from haag_vq import _native
    from haag_vq.methods._ivf import IvfPq

    rng = np.random.default_rng(5)
    X = _clustered(rng, 2000, 32)
    a = IvfPq(32, 16, 8, 8)
    a.train(_t(X, dev), coarse_iters=3, pq_iters=3)
    b = IvfPq(32, 16, 8, 8)
    b.coarse, b.pq, b.prep = a.coarse, a.pq, a.prep
    a.add(_t(X, dev))
    b.add(_t(X[:700], dev))
    b.add(_t(X[700:], dev))
    for f in ("offsets", "codes", "ids", "tau"):
        np.testing.assert_array_equal(_h(getattr(a.lists, f)), _h(getattr(b.lists, f)))
    Q = _t(X[:20], dev)
    for x, y in zip(a.search(Q, 10, 4), b.search(Q, 10, 4)):
        np.testing.assert_array_equal(_h(x), _h(y))
    assert _native.NO_ID not in _h(a.search(Q, 10, 4)[1]).view(np.uint32)


def test_train_coarse_reproducible_and_matches_oracle_update(dev, oracle):
    """Two fits agree bit for bit; one Lloyd step equals the oracle's assignment + update."""
    from haag_vq import _native
    from haag_vq.methods import _ivf

    rng = np.random.default_rng(9)
    X = _clustered(rng, 4000, 24, centers=20)
    Xd = _t(X, dev)
    c1 = _ivf.train_coarse(Xd, 20, niter=4)
    c2 = _ivf.train_coarse(Xd, 20, niter=4)
    np.testing.assert_array_equal(_h(c1), _h(c2))
    C0 = _h(c1)
    _, a = _ivf.assign(Xd, c1)
    ra = oracle.topk_rows(oracle.pairwise(X, C0, 1), 1)[1][:, 0]
    np.testing.assert_array_equal(_h(a).view(np.uint32), ra)
    offsets, order = _native.bucket_sort(a, 20)
    C = c1.clone()
    counts = torch.empty(20, dtype=torch.int32, device=dev)
    _native.centroid_update(Xd, offsets, order, C, counts)
    rc, _ = oracle.centroid_update(X, ra, C0)
    np.testing.assert_array_equal(_h(C), rc)


# ------------------------------------------------------------ reference tests (test_faiss_ivfpq.py)
def make_data(N: int = 256, D: int = 16, seed: int = 0) -> np.ndarray:
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((N, D)).astype(np.float32)
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    return X


@pytest.fixture
def ivf_idx(dev):
    from haag_vq.methods.search.faiss_ivfpq_index import FaissIvfPqIndex

    return FaissIvfPqIndex(K=8, m=4, nbits=4, nprobe=4)


def test_fit_search_shape(ivf_idx):
    ivf_idx.fit(make_data())
    ids = ivf_idx.search(make_data(N=5, seed=42), k=4)
    assert ids.shape == (5, 4) and ids.dtype == np.uint32


def test_search_with_scores_shape(ivf_idx):
    ivf_idx.fit(make_data())
    ids, dists = ivf_idx.search_with_scores(make_data(N=3, seed=7), k=4)
    assert ids.shape == (3, 4) and dists.shape == (3, 4)
    assert np.all(np.diff(dists, axis=1) >= 0)


def test_memory_footprint(ivf_idx):
    ivf_idx.fit(make_data())
    assert ivf_idx.memory_footprint() == 8 * 16 * 4 + 256 * 4 + 16 * 16 * 4


def test_reconstruction_mse_none(ivf_idx):
    X = make_data()
    ivf_idx.fit(X)
    assert ivf_idx.reconstruction_mse(X) is None


def test_save_load(ivf_idx, tmp_path):
    from haag_vq.methods.search.faiss_ivfpq_index import FaissIvfPqIndex

    ivf_idx.fit(make_data())
    p = tmp_path / "ivfpq.npz"
    ivf_idx.save(str(p))
    with np.load(p, allow_pickle=False) as z:  # the file format (an L2 index: tau is there)
        assert sorted(z.files) == sorted(["meta", "coarse", "pq", "offsets", "codes", "ids", "tau"])
        assert z["meta"].dtype == np.int64 and z["meta"].shape == (7,)
        assert z["codes"].dtype == np.uint8 and z["ids"].dtype == np.int32
    loaded = FaissIvfPqIndex(K=8, m=4, nbits=4, nprobe=4)
    loaded.load(str(p))
    Q = make_data(N=5, seed=1)
    assert np.array_equal(ivf_idx.search(Q, k=3), loaded.search(Q, k=3))


def test_ip_metric(dev):
    from haag_vq.methods.search.faiss_ivfpq_index import FaissIvfPqIndex

    idx = FaissIvfPqIndex(K=8, m=4, nbits=4, nprobe=4)
    idx.fit(make_data(), metric="ip")
    ids, scores = idx.search_with_scores(make_data(N=3, seed=55), k=4)
    assert ids.shape == (3, 4) and ids.dtype == np.uint32
    assert np.all(np.diff(scores, axis=1) <= 0)  # inner products, best first


def test_unfitted_search_raises(ivf_idx):
    with pytest.raises(RuntimeError):
        ivf_idx.search(make_data(N=2), k=1)


def test_recall_full_probe_beats_partial(dev):
    """nprobe = K scans every list: recall@10 against exact neighbours must not drop below
    the nprobe = 1 result, and reach a sane level on clustered data."""
    from haag_vq.methods.search.faiss_ivfpq_index import FaissIvfPqIndex

    rng = np.random.default_rng(0)
    X = _clustered(rng, 6000, 64, centers=32, spread=0.5)
    Q = X[:50]
    d2 = ((Q[:, None, :].astype(np.float64) - X[None].astype(np.float64)) ** 2).sum(-1)
    gt = np.argsort(d2, axis=1, kind="stable")[:, :10]
    rec = {}
    for nprobe in (1, 32):
        idx = FaissIvfPqIndex(K=32, m=16, nbits=8, nprobe=nprobe)
        idx.fit(X)
        ids = idx.search(Q, 10).astype(np.int64)
        rec[nprobe] = np.mean([len(set(gt[i]) & set(ids[i])) / 10 for i in range(len(Q))])
    assert rec[32] >= rec[1] - 1e-9
    assert rec[32] > 0.3, rec
