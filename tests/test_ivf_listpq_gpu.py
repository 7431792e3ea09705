"""GPU: the per-list PQ entry points and IvfListPqIndex against the numpy rule
(tests/_ivf_listpq_rule.py).

The decode must equal the rule bit for bit; a search must return the rule's ids and its keys as
uint32 bit patterns.  The lists of the search tests are constructed on the host (seeded codebooks,
the oracle's codes), so a search is judged apart from the fit.  Every case takes a few seconds at
the most."""

import numpy as np
import pytest

import _ivf_listpq_rule as PR

pytestmark = pytest.mark.gpu

NO_ID = PR.NO_ID
CASE_IDS = [(n, m) for n in PR.CASES for m in PR.METRICS]


def _t(a, dev):
    import torch

    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).to(dev)


def _h(t):
    return t.detach().cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(got_d, got_i, want_d, want_i, what):
    np.testing.assert_array_equal(_h(got_i).view(np.uint32), want_i, err_msg=f"{what}: ids")
    np.testing.assert_array_equal(_bits(_h(got_d)), _bits(want_d), err_msg=f"{what}: keys")


@pytest.fixture(scope="module")
def cases(oracle):
    return {(n, m): PR.Case(oracle, n, m) for n, m in CASE_IDS}


def _search(dev, c, probe_l, k, list_ids=None, Q=None):
    from haag_vq import _native

    if not hasattr(c, "_dev"):
        c._dev = dict(Q=_t(c.Q, dev), cb=_t(c.cb, dev), coarse=_t(c.coarse, dev), offsets=_t(c.offsets, dev),
                      codes=_t(c.list_codes, dev), ids=_t(c.list_ids, dev))
    D = c._dev
    return _native.ivf_listpq_search(D["Q"] if Q is None else Q, D["cb"], D["coarse"],
                                     _t(np.asarray(probe_l).astype(np.uint32), dev), D["offsets"], D["codes"],
                                     D["ids"] if list_ids is None else _t(list_ids, dev), c.B, PR.METRIC_ID[c.metric], k)


# ------------------------------------------------------------------------------ search, bit-exact
@pytest.mark.parametrize("name,metric", CASE_IDS)
def test_search_is_bit_identical_to_the_rule_and_passes_the_judge(dev, oracle, cases, name, metric):
    c = cases[(name, metric)]
    want_d, want_i = c.expected(oracle)
    got_d, got_i = _search(dev, c, c.probe_l, PR.TOPK)
    _same(got_d, got_i, want_d, want_i, f"{name} {metric}")
    bad = PR.problems(c.judges, _h(got_i).view(np.uint32), _h(got_d), metric, tie_order=True)
    assert not bad, bad[:3]


@pytest.mark.parametrize("name,metric", CASE_IDS)
def test_search_slots_padding_and_id_order(dev, oracle, cases, name, metric):
    c = cases[(name, metric)]
    rng = np.random.default_rng([c.N, c.M, 5])
    # the probe slots of each query permuted
    perm = np.stack([rng.permutation(PR.NPROBE) for _ in range(PR.NQ)])
    want_d, want_i = c.expected(oracle)
    got_d, got_i = _search(dev, c, np.take_along_axis(c.probe_l, perm, axis=1), PR.TOPK)
    _same(got_d, got_i, want_d, want_i, f"{name} {metric} permuted slots")
    # skipped slots, the empty list, and list_ids with the top bit set (uint32 order)
    empty = int(np.flatnonzero(np.diff(c.offsets) == 0)[0])
    P = c.probe_l.copy()
    P[0, :] = NO_ID              # every slot skipped
    P[1, 0] = NO_ID
    P[1, 2] = PR.K + 3           # an id >= nlist
    P[2, :] = [empty, NO_ID, NO_ID]  # only the empty list
    P[3, 1] = empty              # the empty list next to a live one
    P[4, 1:] = NO_ID             # one list
    ids = c.list_ids.copy()
    ids[rng.random(ids.size) < 0.5] |= np.uint32(1 << 31)
    for k in (1, PR.TOPK, 256):
        want_d, want_i = c.expected(oracle, P, k=k, list_ids=ids)
        got_d, got_i = _search(dev, c, P, k, list_ids=ids)
        _same(got_d, got_i, want_d, want_i, f"{name} {metric} k={k}")
        for a in (0, 2):
            assert (want_i[a] == NO_ID).all() and np.isinf(want_d[a]).all()
    # k = 256 on a query probing fewer than 256 rows: padding after the real rows
    n1 = int(c.offsets[P[1, 1] + 1] - c.offsets[P[1, 1]])
    if n1 < 256:
        assert (want_i[1, :n1] != NO_ID).all() and (want_i[1, n1:] == NO_ID).all() and np.isinf(want_d[1, n1:]).all()
    else:
        assert c.B == 8  # a trained list holds at least 2^B rows; test_search_pads_after_a_short_list has shorter ones
    assert (want_i >> 31).any() and not (want_i[want_i != NO_ID] >> 31).all()


def _random_lists(seed, sizes, M, B, d, nq):
    """Lists of random codes with random codebooks: (offsets, cb, coarse, codes, ids, Q)."""
    rng = np.random.default_rng(seed)
    sizes = np.asarray(sizes)
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n = int(sizes.sum())
    cb = rng.standard_normal((len(sizes), M, 1 << B, d // M)).astype(np.float32)
    coarse = rng.standard_normal((len(sizes), d)).astype(np.float32)
    codes = rng.integers(0, 1 << B, (n, M)).astype(np.uint8)
    ids = rng.permutation(n).astype(np.uint32)
    Q = rng.standard_normal((nq, d)).astype(np.float32)
    return offsets, cb, coarse, codes, ids, Q


def _check_random_lists(dev, oracle, L, P, B, k, what):
    from haag_vq import _native

    offsets, cb, coarse, codes, ids, Q = L
    out = {}
    for metric in (PR.L2, PR.IP):
        want_d, want_i = PR.expected(oracle, codes, ids, offsets, coarse, cb, Q, P, metric, k)
        got_d, got_i = _native.ivf_listpq_search(_t(Q, dev), _t(cb, dev), _t(coarse, dev), _t(P.astype(np.uint32), dev),
                                                 _t(offsets, dev), _t(codes, dev), _t(ids, dev), B, metric, k)
        _same(got_d, got_i, want_d, want_i, f"{what} metric {metric} k={k}")
        out[metric] = want_i
    return out


def test_search_pads_after_a_short_list(dev, oracle):
    """k = 256 over one probed list of 40 rows (and an empty one), lists shorter than a row step.
    One sub-centroid of list 0 is NaN: the rows coded with it have NaN keys, which rank as +inf,
    by id, before the padding."""
    L = _random_lists(17, [40, 0, 25], M=4, B=4, d=12, nq=5)
    L[1][0, 1, 3, 2] = np.nan
    hit = int((L[3][:40, 1] == 3).sum())
    assert 0 < hit < 40
    P = np.array([[0, 1], [1, NO_ID], [2, 0], [NO_ID, 2], [0, 7]], np.int64)
    for metric, want_i in _check_random_lists(dev, oracle, L, P, 4, 256, "short lists").items():
        want_d = PR.expected(oracle, L[3], L[4], L[0], L[2], L[1], L[5], P, metric, 256)[0]
        assert np.isfinite(want_d[0, :40 - hit]).all() and np.isinf(want_d[0, 40 - hit:]).all()
        assert (np.diff(want_i[0, 40 - hit:40].astype(np.int64)) > 0).all()  # the NaN rows by id
        assert (want_i[0, :40] != NO_ID).all() and (want_i[0, 40:] == NO_ID).all() and (want_i[1] == NO_ID).all()
        assert (want_i[2, :65] != NO_ID).all() and (want_i[2, 65:] == NO_ID).all()


@pytest.mark.parametrize("M,B,d", [(4, 4, 12), (128, 8, 128)])
def test_search_long_lists_take_several_steps_and_row_ranges(dev, oracle, M, B, d):
    """A list of 20000 rows: under the row-range split every range is several 2048-row steps long
    and the last one is partial; at M = 128 every step restages the table chunks.  Codes with
    many exact key ties at M = 4 (16^4 codes for 20000 rows)."""
    L = _random_lists([M, B, 23], [20000, 300, 0, 2500], M=M, B=B, d=d, nq=5)
    P = np.array([[0, 3], [0, 1], [3, 1], [0, NO_ID], [1, 3]], np.int64)
    for k in (10, 256):
        _check_random_lists(dev, oracle, L, P, B, k, f"long lists M={M}")


@pytest.mark.parametrize("M,B,d", [(2, 4, 400), (2, 4, 402), (1, 8, 2500), (3, 2, 300)])
def test_search_sub_vectors_longer_than_the_staged_row(dev, oracle, M, B, d):
    """The table kernel stages 2048 floats a row for the subspaces of a unit of 256 entries (16 at
    B = 4, 64 at B = 2, one at B = 8): longer sub-vectors are tiled over t, the chains carried
    across the tiles (128 + 72, 128 + 73 odd, 2048 + 452, and 32 + 32 + 32 + 4 dims a tile)."""
    assert max(1, 256 >> B) * (d // M) > 2048
    L = _random_lists([M, B, d], [300, 40, 0], M=M, B=B, d=d, nq=7)
    P = np.array([[0, 1], [1, 0], [0, NO_ID], [1, 2], [2, 0], [0, 1], [1, NO_ID]], np.int64)
    _check_random_lists(dev, oracle, L, P, B, 10, f"tiled sub-vectors M={M} B={B} d={d}")


def test_search_of_no_queries(dev, cases):
    c = cases[("m8_b4_d40", "l2")]
    import torch

    d, i = _search(dev, c, np.zeros((0, PR.NPROBE), np.int64), PR.TOPK,
                   Q=torch.empty((0, c.D), dtype=torch.float32, device=dev))
    assert tuple(d.shape) == tuple(i.shape) == (0, PR.TOPK)


# ------------------------------------------------------------------------------ decode
@pytest.mark.parametrize("name", list(PR.CASES))
def test_decode_equals_the_rule_in_any_row_order(dev, oracle, cases, name):
    from haag_vq import _native

    c = cases[(name, "l2")]
    rows = np.random.default_rng(c.N).permutation(c.N)[: c.N - 7]  # row order, arbitrary
    got = _native.ivf_listpq_decode(_t(c.codes[rows], dev), _t(c.cb, dev), _t(c.coarse, dev),
                                    _t(c.assign[rows].astype(np.int32), dev), c.B)
    np.testing.assert_array_equal(_bits(_h(got)), _bits(c.rec[rows]))


# ------------------------------------------------------------------------------ composition, wide
def test_wide_search_is_the_composition_of_the_flat_adc_and_chunks_its_queries(dev):
    """d = 1024, M = 128, B = 8, 8 lists of 300 rows, 600 queries probing every list: 4800 pairs of
    128 KB tables, more than one chunk of the workspace.  Equal to adc_lut on cb[l] + c_l and
    adc_search per list merged on the host, and to the same search on the two halves of the queries."""
    import torch
    from haag_vq import _native

    d, M, B, nlist, per, nq, k = 1024, 128, 8, 8, 300, 600, 10
    ksub, dsub, n = 1 << B, d // M, nlist * per
    fn = _native.load_library().mivq_ivf_listpq_search_workspace_bytes
    assert 4800 * M * ksub * 4 > (1 << 29)
    assert 0 < fn(nq, n, nlist, nlist, d, M, B, k) < 4800 * M * ksub * 4  # several chunks of queries
    g = torch.Generator(device="cpu").manual_seed(1024)
    cb = (torch.randn((nlist, M, ksub, dsub), generator=g) * 0.8).to(dev)
    coarse = (torch.randn((nlist, d), generator=g) * 2.0).to(dev)
    codes = torch.randint(0, ksub, (n, M), generator=g, dtype=torch.uint8).to(dev)
    ids_h = (torch.arange(n) * 3 + 1).to(torch.int32)  # ascending with the position: a list's (key, row) order is (key, id)
    Q = (torch.randn((nq, d), generator=g) * 1.5).to(dev)
    offsets = (torch.arange(nlist + 1, dtype=torch.int64) * per).to(dev)
    probe = torch.stack([torch.randperm(nlist, generator=g) for _ in range(nq)]).to(torch.int32).to(dev)
    ids = ids_h.to(dev)
    for metric in (PR.L2, PR.IP):
        got_d, got_i = _native.ivf_listpq_search(Q, cb, coarse, probe, offsets, codes, ids, B, metric, k)
        cd, ci = [], []
        for l in range(nlist):
            e = (cb[l] + coarse[l].reshape(M, 1, dsub)).contiguous()
            lut = _native.adc_lut(Q, e, B, metric)
            d1, i1 = _native.adc_search(lut, codes[l * per:(l + 1) * per].contiguous(), k, B)  # the list's k best
            cd.append(_h(d1))
            ci.append(_h(ids_h)[l * per + _h(i1).astype(np.int64)].astype(np.int64))
        cd, ci = np.concatenate(cd, axis=1), np.concatenate(ci, axis=1)
        want_d, want_i = np.empty((nq, k), np.float32), np.empty((nq, k), np.uint32)
        for a in range(nq):
            o = np.lexsort((ci[a], cd[a]))[:k]
            want_d[a], want_i[a] = cd[a][o], ci[a][o]
        _same(got_d, got_i, want_d, want_i, f"wide metric {metric}")
        h = nq // 2
        for s, t in ((0, h), (h, nq)):
            p_d, p_i = _native.ivf_listpq_search(Q[s:t].contiguous(), cb, coarse, probe[s:t].contiguous(), offsets, codes,
                                                 ids, B, metric, k)
            _same(p_d, p_i, want_d[s:t], want_i[s:t], f"wide metric {metric} queries {s}:{t}")


# ------------------------------------------------------------------------------ the index
def _index_data():
    """N = 1500, D = 32 rows on 3 clusters and K = 4 centroids, one of which attracts nothing."""
    rng = np.random.default_rng([1500, 32, 4])
    centres = rng.standard_normal((3, 32)) * 2.0 + 3.0
    spread = rng.uniform(0.2, 1.5, 32)
    member = np.arange(1500) % 3
    X = (centres[member] + rng.standard_normal((1500, 32)) * spread).astype(np.float32)
    Q = (centres[rng.integers(0, 3, 9)] + rng.standard_normal((9, 32)) * spread).astype(np.float32)
    coarse = np.stack([X[0], np.full(32, -10.0, np.float32), X[1], X[2]]).astype(np.float32)
    return X, Q, coarse


def _factory(M=4, B=8, niter=2):
    from haag_vq.methods.product_quantization import ProductQuantizer

    def make():
        q = ProductQuantizer(M=M, B=B)
        q.niter = niter
        return q

    return make


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_index_against_train_pq_its_engine_and_numpy(dev, metric, tmp_path):
    import torch
    from haag_vq import _native
    from haag_vq.methods._kmeans import train_pq
    from haag_vq.methods.search import IvfListPqIndex

    X, Q, coarse = _index_data()
    idx = IvfListPqIndex(_factory(), K=4, nprobe=2)
    idx.fit(X, metric, centroids=coarse)
    assert idx.ntotal == 1500
    eng = idx._index
    off = _h(eng.lists.offsets)
    sizes = np.diff(off)
    assert sizes[1] == 0 and (sizes[[0, 2, 3]] >= 256).all() and sizes.sum() == 1500, sizes
    assert metric == "ip" or list(sizes) == [500, 0, 500, 500]  # inner products do not follow the clusters
    order = _h(eng.lists.ids).astype(np.int64)
    Xd, cd = _t(X, dev), _t(coarse, dev)
    assert tuple(eng.codebooks.shape) == (4, 4, 256, 8)
    for l in range(4):
        rows = order[off[l]:off[l + 1]]
        if rows.size == 0:
            assert not _h(eng.codebooks[l]).any()
            continue
        assert (np.diff(rows) > 0).all()  # ascending row order
        R = _native.ivf_residuals(Xd[torch.from_numpy(rows).to(dev)].contiguous(), cd,
                                  torch.full((rows.size,), l, dtype=torch.int32, device=dev))
        C = train_pq(R, 4, 8, niter=2, seed=1234)
        np.testing.assert_array_equal(_bits(_h(eng.codebooks[l])), _bits(_h(C)), err_msg=f"codebook of list {l}")
        want = _native.pq_encode(R, C, _native.pq_prepare(C, 8), 8)
        np.testing.assert_array_equal(_h(eng.lists.codes[off[l]:off[l + 1]]), _h(want), err_msg=f"codes of list {l}")
    # search_with_scores: the engine's raw result with the reference's sentinels; IP stays negated
    idx.nprobe = 1
    raw_d, raw_i = eng.search(_t(Q, dev), 256, 1)
    raw_d, raw_i = _h(raw_d), _h(raw_i).view(np.uint32)
    ids, dists = idx.search_with_scores(Q, 256)
    assert ids.shape == dists.shape == (9, 256) and ids.dtype == np.uint32 and dists.dtype == np.float32
    np.testing.assert_array_equal(ids, raw_i)
    assert (ids != NO_ID).all()  # every non-empty list holds at least 256 rows
    np.testing.assert_array_equal(_bits(dists), _bits(raw_d))
    idx.nprobe = 2
    dev_d, dev_i = idx.search_device(Q, 10)
    np.testing.assert_array_equal(idx.search(Q, 10), _h(dev_i).view(np.uint32))
    e_ids, e_dists = idx.search_with_scores(Q, 0)
    assert e_ids.shape == e_dists.shape == (9, 0) and e_ids.dtype == np.uint32 and e_dists.dtype == np.float32
    # reconstruction_mse: the numpy mean over reconstruct
    rec = _h(eng.reconstruct(torch.arange(1500)))
    sample = np.array([0, 5, 77, 1499, 300])
    for s in (None, sample):
        rows = np.arange(1500) if s is None else s
        want = float(np.mean(np.array([np.mean((X[r] - rec[r]) ** 2) for r in rows], np.float64)))
        assert idx.reconstruction_mse(X, s) == pytest.approx(want, rel=1e-6)
    # nprobe = K: the keys are ADC distances to the reconstruction (fp32 reordering apart)
    idx.nprobe = 4
    a_ids, a_d = idx.search_with_scores(Q, 10)
    for a in range(9):
        diff = rec[a_ids[a].astype(np.int64)].astype(np.float64) - Q[a].astype(np.float64)
        exact = (diff ** 2).sum(axis=1) if metric == "l2" else -(rec[a_ids[a].astype(np.int64)].astype(np.float64) @ Q[a])
        np.testing.assert_allclose(a_d[a], exact, rtol=1e-4, atol=1e-3)
    # memory_footprint: centroids + codes + codebooks
    assert idx.memory_footprint() == 4 * 32 * 4 + 1500 * 4 + 4 * 32 * 256 * 4
    # save / load into a fresh index
    path = tmp_path / "listpq.npz"
    idx.save(path)
    with np.load(path, allow_pickle=False) as z:  # the file format
        assert sorted(z.files) == sorted(["coarse", "codebooks", "offsets", "codes", "ids", "M", "B", "niter", "seed", "K",
                                          "nprobe", "metric", "N", "D"])
        assert z["codes"].dtype == np.uint8 and z["codes"].shape == (1500, 4) and z["ids"].dtype == np.int32
    other = IvfListPqIndex(_factory(M=2, B=4), K=3, nprobe=9)
    other.load(path)
    assert (other._M, other._B, other._K, other.nprobe, other.ntotal) == (4, 8, 4, 4, 1500)
    o_ids, o_dists = other.search_with_scores(Q, 10)
    np.testing.assert_array_equal(o_ids, a_ids)
    np.testing.assert_array_equal(_bits(o_dists), _bits(a_d))
    assert other.reconstruction_mse(X, sample) == idx.reconstruction_mse(X, sample)
    assert other.memory_footprint() == idx.memory_footprint()


def test_index_sentinels(dev):
    """Slots the probed lists cannot fill: id 0xFFFFFFFF with FLT_MAX (L2) / -FLT_MAX (IP)."""
    from haag_vq.methods.search import IvfListPqIndex

    X, Q, coarse = _index_data()
    fmax = np.finfo(np.float32).max
    for metric in ("l2", "ip"):
        idx = IvfListPqIndex(_factory(M=4, B=4), K=4, nprobe=1)
        idx.fit(X[:150], metric, centroids=coarse)  # about 50 rows per list
        eng = idx._index
        rows = np.diff(_h(eng.lists.offsets))[_h(eng.probes(_t(Q, dev), 1))[:, 0]]
        assert (rows >= 16).all() and (rows < 64).all(), rows
        ids, dists = idx.search_with_scores(Q, 64)
        raw_d, raw_i = idx.search_device(Q, 64)
        pad = ids == NO_ID
        np.testing.assert_array_equal(pad, np.arange(64)[None, :] >= rows[:, None])
        np.testing.assert_array_equal(ids, _h(raw_i).view(np.uint32))
        np.testing.assert_array_equal(_bits(dists[~pad]), _bits(_h(raw_d)[~pad]))
        assert np.isinf(_h(raw_d)[pad]).all()
        assert (dists[pad] == (-fmax if metric == "ip" else fmax)).all()
        assert (np.diff(np.where(pad, fmax, dists), axis=1) >= 0).all()


def test_index_errors(dev):
    from haag_vq.methods._ivf import IvfListPq
    from haag_vq.methods.search import IvfListPqIndex

    X, Q, coarse = _index_data()
    # one list gets 100 rows, fewer than 2^8: raised right after the assignment, before any training
    short = np.concatenate([X[np.arange(1500) % 3 != 1], X[1::3][:100]])
    idx = IvfListPqIndex(_factory(), K=4, nprobe=2)
    with pytest.raises(RuntimeError, match=r"Number of training points \(100\) should be at least as large as number of "
                                           r"clusters \(256\).*list 2.*1 non-empty list.*smaller K or B"):
        idx.fit(short, "l2", centroids=coarse)
    assert idx._index is None and idx.ntotal == 0 and idx.memory_footprint() == 0
    with pytest.raises(RuntimeError, match="fit"):
        idx.search(Q, 3)
    eng = IvfListPq(32, 4, 4, 8, niter=2)
    eng.coarse = _t(coarse, dev)
    with pytest.raises(RuntimeError, match="Number of training points"):
        eng.fit_lists(_t(short, dev))
    assert eng.codebooks is None and eng.lists is None
    with pytest.raises(AssertionError, match="divisible"):
        IvfListPqIndex(_factory(M=5), K=4).fit(X, "l2", centroids=coarse)
    with pytest.raises(ValueError, match="metric"):
        idx.fit(X, "cosine")
    with pytest.raises(ValueError, match="centroids"):
        idx.fit(X, "l2", centroids=coarse[:3])
    idx.fit(X, "l2", centroids=coarse)
    for call in (idx.search, idx.search_with_scores, idx.search_device):
        with pytest.raises(ValueError, match="k=257"):
            call(Q, 257)
