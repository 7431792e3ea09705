"""GPU: mivq_ivfpq_search and mivq_topk_merge on raw arrays against the numpy rule of
tests/_ivfpq_rule.py (pinned to the C oracle by tests/test_ivfpq_rule_cpu.py), GPU-against-GPU
invariants, the host-side rejections and query counts above the grid's y limit.

LUT, probe_d, probe_l, offsets, codes, ids and tau are all made by the helper: no encode, no
training.  Ids must equal the rule's and distances must equal it as uint32 bit patterns."""

import numpy as np
import pytest

import _ivfpq_rule as R

pytestmark = pytest.mark.gpu

NO_ID = R.NO_ID


def _t(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _h(t):
    return t.detach().cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _ids(case):
    return "-".join(str(x) for x in case)


def _search(dev, D, lut, probe_d, probe_l, tau, metric, k):
    from haag_vq import _native

    dd, ii = _native.ivfpq_search(_t(lut, dev), _t(probe_d, dev), _t(probe_l.view(np.int32), dev),
                                  _t(D["offsets"], dev), _t(D["codes"], dev), _t(D["ids"].view(np.int32), dev),
                                  None if tau is None else _t(tau, dev), metric, k, D["nbits"])
    return _h(dd), _h(ii).view(np.uint32)


def test_cases_cover_the_issue():
    R.assert_cases_cover_the_issue()


# ------------------------------------------------------------------------------ the scan, bit-exact
@pytest.mark.parametrize("case", R.CASES, ids=_ids)
def test_search_bit_exact(dev, case):
    name, M, nbits, metric, kind, k, nq, nprobe, probes = case
    I = R.case_inputs(case)
    D, P = I["D"], I["probe_l"]
    rd, ri = R.case_expected(case)
    dd, ii = _search(dev, D, I["lut"], I["probe_d"], P, I["tau"], metric, k)
    np.testing.assert_array_equal(ii, ri)
    np.testing.assert_array_equal(_bits(dd), _bits(rd))
    # what the constructed lists must show in the result
    rows = R.rows_probed(D, P)
    np.testing.assert_array_equal((ii != NO_ID).sum(1), np.minimum(k, rows))
    assert np.isposinf(dd[ii == NO_ID]).all() and not np.isnan(dd).any()
    if probes == "skips" and nq > 1:
        assert (ii[nq // 2] == NO_ID).all()              # every slot skipped: an all-padding row
    if probes == "empty_alone":
        assert (ii == NO_ID).all()
    if probes == "small_alone":
        assert (ii[:, :20] != NO_ID).all() and (ii[:, 20:] == NO_ID).all()
    if metric == R.L2 and D["nan_id"] is not None:
        seen = 0
        for a in range(nq):
            if R.SMALL in P[a] and rows[a] <= k:         # k large enough: the NaN-tau row must be there
                at = np.nonzero(ii[a] == D["nan_id"])[0]
                assert at.size == 1 and np.isposinf(dd[a, at[0]])
                assert at[0] < rows[a] and (ii[a, :at[0] + 1] != NO_ID).all()  # ahead of every pad
                seen += 1
        assert seen > 0 or probes != "small_alone"


def test_twin_rows_in_two_lists_rank_by_id(dev):
    """Equal code rows with equal tau in two lists of equal probe_d: equal distances found by
    different waves come out next to each other, the smaller id first (ids compared unsigned)."""
    D = R.data_set("A", 8, 8)
    nq, k = 5, 256
    P = np.tile(np.array([R.TWIN_A, R.TWIN_B, R.SMALL], np.uint32), (nq, 1))
    PD = R.list_distances(D, "generic", nq, 1)
    lut = R.make_lut(D, "generic", nq, 1)
    tau = D["tau"]["generic"]
    assert R.rows_probed(D, P).max() <= k
    dd, ii = _search(dev, D, lut, R.probe_distances(PD, P), P, tau, R.L2, k)
    x, y = D["dups"][1]
    lo, hi = sorted((int(D["ids"][x]), int(D["ids"][y])))
    for a in range(nq):
        ids = ii[a].tolist()
        assert ids.index(hi) == ids.index(lo) + 1 and dd[a][ids.index(lo)] == dd[a][ids.index(hi)]


# ------------------------------------------------------------------------------ invariants, GPU vs GPU
@pytest.mark.parametrize("name,M,nbits,metric,kind,k,nq,nprobe", [
    ("A", 8, 8, R.L2, "ties", 100, 37, 16),
    ("A", 6, 4, R.IP, "generic", 100, 37, 16),
    ("B", 8, 8, R.L2, "ties", 256, 1, 50),
    ("B", 10, 5, R.IP, "generic", 64, 1, 50),
])
def test_probe_order_does_not_matter(dev, name, M, nbits, metric, kind, k, nq, nprobe):
    """A permutation of a query's probe slots moves lists between waves and splits."""
    D = R.data_set(name, M, nbits)
    rng = np.random.default_rng([M, nprobe])
    P0 = R.make_probes(D, "rand", nq, nprobe, 3)
    P1 = np.stack([row[rng.permutation(nprobe)] for row in P0])
    assert (P0 != P1).any() and np.array_equal(np.sort(P0, 1), np.sort(P1, 1))
    PD = R.list_distances(D, kind, nq, 3)
    lut = R.make_lut(D, kind, nq, 3)
    tau = D["tau"][kind] if metric == R.L2 else None
    d0, i0 = _search(dev, D, lut, R.probe_distances(PD, P0), P0, tau, metric, k)
    d1, i1 = _search(dev, D, lut, R.probe_distances(PD, P1), P1, tau, metric, k)
    np.testing.assert_array_equal(i0, i1)
    np.testing.assert_array_equal(_bits(d0), _bits(d1))
    rd, ri = R.search_rule(lut, R.probe_distances(PD, P0), P0, D["offsets"], D["codes"], D["ids"], tau, metric, k)
    np.testing.assert_array_equal(i0, ri)
    np.testing.assert_array_equal(_bits(d0), _bits(rd))


@pytest.mark.parametrize("M,nbits,n,nq,k", [(8, 8, 3000, 37, 100), (16, 4, 1000, 5, 256), (6, 8, 700, 3, 10)])
def test_one_list_equals_adc_search(dev, M, nbits, n, nq, k):
    """One list holding every row, probe_d = 0, IP: "ranked like mivq_adc_search"."""
    import torch
    from haag_vq import _native

    rng = np.random.default_rng([M, nbits, n])
    lut = _t(rng.standard_normal((nq, M, 1 << nbits)).astype(np.float32), dev)
    codes = rng.integers(0, 1 << nbits, (n, M)).astype(np.uint8)
    codes[n // 2] = codes[n // 3]  # a tie, broken by the smaller id
    codes = _t(codes, dev)
    ad, ai = _native.adc_search(lut, codes, k, nbits)
    dd, ii = _native.ivfpq_search(lut, torch.zeros((nq, 1), dtype=torch.float32, device=dev),
                                  torch.zeros((nq, 1), dtype=torch.int32, device=dev),
                                  torch.tensor([0, n], dtype=torch.int64, device=dev), codes,
                                  torch.arange(n, dtype=torch.int32, device=dev), None, R.IP, k, nbits)
    np.testing.assert_array_equal(_h(ii), _h(ai))
    np.testing.assert_array_equal(_h(dd), _h(ad))


# ------------------------------------------------------------------------------ rejections
@pytest.mark.parametrize("M,nbits,k,msg", [(129, 8, 10, "LDS"), (65, 8, 257, "k=257"), (8, 8, 257, "k=257")])
def test_rejected_on_the_host(dev, M, nbits, k, msg):
    """M * ksub * 4 > 128 KiB and k > 256 raise from the host check, before any launch."""
    import torch
    from haag_vq import _native

    D = R.data_set("A", 8, 8)
    codes = np.zeros((D["n"], M), np.uint8)
    with pytest.raises(ValueError, match=msg):
        _native.ivfpq_search(_t(np.zeros((2, M, 1 << nbits), np.float32), dev), _t(np.zeros((2, 1), np.float32), dev),
                             _t(np.zeros((2, 1), np.int32), dev), _t(D["offsets"], dev), _t(codes, dev),
                             _t(D["ids"].view(np.int32), dev), _t(D["tau"]["generic"], dev), R.L2, k, nbits)
    torch.cuda.synchronize()  # nothing was launched, so nothing can have failed


# ------------------------------------------------------------------------------ mivq_topk_merge
@pytest.mark.parametrize("parts,k,nq,kind", R.MERGE_CASES)
def test_topk_merge_bit_exact(dev, parts, k, nq, kind):
    from haag_vq import _native

    dd, ii = R.merge_inputs(parts, k, nq, kind)
    rd, ri = R.merge_rule(dd, ii, k)
    od, oi = _native.topk_merge(_t(dd, dev), _t(ii.view(np.int32), dev), k)
    od, oi = _h(od), _h(oi).view(np.uint32)
    np.testing.assert_array_equal(oi, ri)
    np.testing.assert_array_equal(_bits(od), _bits(rd))
    if parts == 0:
        assert (oi == NO_ID).all() and np.isposinf(od).all()
    assert not np.isnan(od).any()


# ------------------------------------------------------------------------------ nq above grid.y
def test_more_queries_than_one_launch_takes(dev):
    """65,541 queries (seven distinct ones tiled): the C entry point takes at most 65,535 per
    call and the binding runs ranges of them; every row is the rule's row of its source query."""
    import torch
    from haag_vq import _native

    T = R.tiled_case()
    D, k = T["D"], T["k"]
    rd, ri = R.search_rule(T["lut"], T["probe_d"], T["probe_l"], D["offsets"], D["codes"], D["ids"], T["tau"], R.L2, k)
    nq = R.BIG_NQ
    assert nq > _native.MAX_QUERIES_PER_CALL == 65535
    src = torch.arange(nq, device=dev) % 7
    lut = _t(T["lut"], dev)[src].contiguous()
    assert lut.numel() * 4 < 20 << 20
    pd = _t(T["probe_d"], dev)[src].contiguous()
    pl = _t(T["probe_l"].view(np.int32), dev)[src].contiguous()
    args = (_t(D["offsets"], dev), _t(D["codes"], dev), _t(D["ids"].view(np.int32), dev), _t(T["tau"], dev))
    dd, ii = _native.ivfpq_search(lut, pd, pl, *args, R.L2, k, T["nbits"])
    src = _h(src)
    np.testing.assert_array_equal(_h(ii).view(np.uint32), ri[src])
    np.testing.assert_array_equal(_bits(_h(dd)), _bits(rd[src]))
    # the C entry point itself refuses the whole batch, on the host
    ws = _native.workspace(256, dev)  # the query count is checked before the workspace
    with pytest.raises(ValueError, match="65535"):
        _native._call("mivq_ivfpq_search", _native._ptr(lut), nq, 4, T["nbits"], _native._ptr(pd), _native._ptr(pl), 2,
                      4, *[_native._ptr(a) for a in args], R.L2, k, _native._ptr(ws), ws.numel(), _native._ptr(dd),
                      _native._ptr(ii), _native._stream())


def test_more_queries_than_one_launch_takes_rabitq_generic(dev, oracle):
    """The same for the generic estimator of mivq_rabitq_search (qb = 0), whose grid is
    (code blocks, nq): d = 8, n = 50, against oracle.rabitq_est + oracle.topk_rows."""
    import torch
    from haag_vq import _native

    d, n, k, qb = 8, 50, 5, 0
    rng = np.random.default_rng(8)
    X = rng.standard_normal((n, d)).astype(np.float32)
    X[31] = X[4]  # duplicate code: tie broken by the smaller id
    Q7 = rng.standard_normal((7, d)).astype(np.float32)
    c = X.mean(0).astype(np.float32)
    cd = _t(c, dev)
    codes = _native.rabitq_encode(_t(X, dev), cd, R.L2)
    rd, ri = oracle.topk_rows(oracle.rabitq_est(_h(codes), d, Q7, c, qb, R.L2), k)
    nq = R.BIG_NQ
    src = torch.arange(nq, device=dev) % 7
    Q = _t(Q7, dev)[src].contiguous()
    kd, ki = _native.rabitq_search(codes, d, cd, Q, qb, R.L2, k)
    src = _h(src)
    np.testing.assert_array_equal(_h(ki).view(np.uint32), ri[src])
    np.testing.assert_array_equal(_bits(_h(kd)), _bits(rd[src]))
    ws = _native.workspace(256, dev)  # the query count is checked before the workspace
    with pytest.raises(ValueError, match="65535"):
        _native._call("mivq_rabitq_search", _native._ptr(codes), n, d, _native._ptr(cd), _native._ptr(Q), nq, qb, R.L2,
                      k, 0, _native._ptr(ws), ws.numel(), _native._ptr(kd), _native._ptr(ki), _native._stream())
