"""GPU: the per-list SQ / LVQ entry points and IvfQuantizedIndex against the numpy rule
(tests/_ivf_quantized_rule.py) and the reference's fixture.

Fit, encode and decode must equal the rule bit for bit; a search must return the rule's ids and
its keys as uint32 bit patterns.  The lists of the search tests are constructed on the host (the
rule's parameters and codes), so a search is judged apart from the encode.  Every case takes a
few seconds at the most."""

from pathlib import Path

import numpy as np
import pytest

import _ivf_quantized_rule as IR

pytestmark = pytest.mark.gpu

NO_ID = IR.NO_ID
GOLDEN = Path(__file__).resolve().parent / "golden"
CASE_IDS = [(n, m) for n in IR.CASES for m in IR.METRICS]
FORMATS = [("sq", 4), ("sq", 8), ("sq", 16), ("lvq", 1), ("lvq", 3), ("lvq", 4), ("lvq", 8)]


def _t(a, dev):
    import torch

    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        a = a.view(np.int16)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).to(dev)


def _h(t):
    a = t.detach().cpu().numpy()
    return a.view(np.uint16) if a.dtype == np.int16 else a


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(got_d, got_i, want_d, want_i, what):
    np.testing.assert_array_equal(_h(got_i).view(np.uint32), want_i, err_msg=f"{what}: ids")
    np.testing.assert_array_equal(_bits(_h(got_d)), _bits(want_d), err_msg=f"{what}: keys")


@pytest.fixture(scope="module")
def cases(oracle):
    fx = IR.load_fixture(GOLDEN)
    return {(n, m): IR.Case(oracle, n, m, fx) for n, m in CASE_IDS}


def _params_t(params, dev):
    return tuple(_t(p, dev) for p in params)


def _gpu_fit(dev, X, coarse, assign, kind):
    """The engine's fit of the per-list parameters for a given assignment."""
    from haag_vq import _native
    from haag_vq.methods._ivf import IvfCodes

    eng = IvfCodes(X.shape[1], coarse.shape[0], kind, 8)
    eng.coarse = _t(coarse, dev)
    a = _t(assign.astype(np.int32), dev)
    offsets, order = _native.bucket_sort(a, coarse.shape[0])
    return tuple(eng._fit_params(_t(X, dev), a, offsets, order))


def _gpu_encode(dev, X, coarse, assign, params, kind, bits, out=None):
    from haag_vq import _native

    a = _t(assign.astype(np.int32), dev)
    if kind == "sq":
        return _native.ivf_sq_encode(_t(X, dev), _t(coarse, dev), a, params[0], params[1], bits, out=out)
    return _native.ivf_lvq_encode(_t(X, dev), _t(coarse, dev), a, params[0], bits, out=out)


def _gpu_decode(dev, codes, coarse, assign, params, kind, bits):
    from haag_vq import _native

    a = _t(assign.astype(np.int32), dev)
    if kind == "sq":
        return _native.ivf_sq_decode(codes, _t(coarse, dev), a, params[0], params[1], bits)
    return _native.ivf_lvq_decode(codes, _t(coarse, dev), a, params[0], bits)


# ------------------------------------------------------------------------------ fit / encode / decode
@pytest.mark.parametrize("name,metric", CASE_IDS)
def test_fit_encode_decode_equal_the_rule_on_the_fixture_cases(dev, oracle, cases, name, metric):
    c = cases[(name, metric)]
    params = _gpu_fit(dev, c.X, c.coarse, c.assign, c.kind)
    for got, want in zip(params, c.params):
        np.testing.assert_array_equal(_bits(_h(got)), _bits(want))
    codes = _gpu_encode(dev, c.X, c.coarse, c.assign, params, c.kind, c.bits)
    np.testing.assert_array_equal(_h(codes), c.codes)
    rec = _gpu_decode(dev, codes, c.coarse, c.assign, params, c.kind, c.bits)
    np.testing.assert_array_equal(_bits(_h(rec)), _bits(c.rec))


def test_lvq_means_in_groups_of_lists(dev, cases, monkeypatch):
    """A database past the residual buffer's budget is fitted whole lists at a time: the same means."""
    from haag_vq.methods import _ivf

    c = cases[("lvq4_d100", "l2")]
    monkeypatch.setattr(_ivf, "_MAT_BYTES", 4 * c.D * 450)  # two lists fit, three do not
    (mu,) = _gpu_fit(dev, c.X, c.coarse, c.assign, "lvq")
    np.testing.assert_array_equal(_bits(_h(mu)), _bits(c.params[0]))


@pytest.mark.parametrize("kind,bits", FORMATS)
@pytest.mark.parametrize("d", [37, 64, 3072])
def test_codec_edge_rows(dev, oracle, kind, bits, d):
    """A list of exactly one row (SQ: hi == lo, den = 1e-8, every level 0; LVQ: the residual is
    the mean, so span == 0, delta = FLT_MIN and every index 0), an empty list, odd d (SQ-4: the
    zero-padded nibble), and writes that stay inside the n rows."""
    import torch

    n, nlist = 203, 5
    rng = np.random.default_rng([d, bits, 11])
    coarse = (3.0 * rng.standard_normal((nlist, d))).astype(np.float32)
    assign = rng.integers(0, 3, n)   # lists 0..2; list 3 gets one row, list 4 none
    assign[57] = 3
    X = (coarse[assign] + rng.standard_normal((n, d)) * rng.uniform(0.2, 1.5, d)).astype(np.float32)
    want_p = IR.fit(X, coarse, assign, kind)
    params = _gpu_fit(dev, X, coarse, assign, kind)
    for got, want in zip(params, want_p):
        np.testing.assert_array_equal(_bits(_h(got)), _bits(want))
    if kind == "sq":
        assert (want_p[1][3] == np.float32(1e-8)).all() and (want_p[1][4] == np.float32(1e-8)).all()
        assert (want_p[0][4] == 0).all()
    want_c = IR.encode(X, coarse, assign, want_p, kind, bits)
    width, dt = IR.code_shape(kind, bits, d)
    fill = 0xAB if dt == np.uint8 else 0x2BAB
    buf = torch.full((n + 8, width), fill, dtype=torch.uint8 if dt == np.uint8 else torch.int16, device=dev)
    out = _gpu_encode(dev, X, coarse, assign, params, kind, bits, out=buf[:n])
    assert out.data_ptr() == buf.data_ptr()
    got = _h(buf)
    assert (got[n:] == fill).all()
    np.testing.assert_array_equal(got[:n], want_c)
    if kind == "sq":
        assert not got[57].any()
    else:
        ib = width - 8
        assert not got[57, :ib].any() and got[57, ib + 4:].copy().view("<f4")[0] == np.finfo(np.float32).tiny
    rec = _gpu_decode(dev, buf[:n], coarse, assign, params, kind, bits)
    np.testing.assert_array_equal(_bits(_h(rec)), _bits(IR.decode(oracle, want_c, coarse, assign, want_p, kind, bits)))


# ------------------------------------------------------------------------------ search, bit-exact
class Lists:
    """Constructed lists: the rule's parameters and codes for a planned assignment, in bucket
    order, ids with bit 31 set on half of the rows, duplicate rows planted in list 0."""

    def __init__(self, oracle, kind, bits, d, sizes, seed, nq=9):
        rng = np.random.default_rng([d, bits, seed])
        self.kind, self.bits, self.d, self.nlist = kind, bits, d, len(sizes)
        n = int(sum(sizes))
        assign = rng.permutation(np.repeat(np.arange(self.nlist), sizes))
        self.coarse = (2.0 * rng.standard_normal((self.nlist, d))).astype(np.float32)
        X = (self.coarse[assign] + rng.standard_normal((n, d)) * rng.uniform(0.2, 1.5, d)).astype(np.float32)
        rows0 = np.flatnonzero(assign == 0)
        ids = np.arange(n, dtype=np.int64)
        ids[rng.random(n) < 0.5] += 1 << 31
        a, b = int(rows0[3]), int(rows0[len(rows0) // 2])
        X[b] = X[a]                       # equal codes, equal keys: ranked by id as uint32
        ids[a], ids[b] = (1 << 31) + n + 5, n + 7  # (no other row has these) the larger id first in row order
        self.dups = (n + 7, (1 << 31) + n + 5)
        self.params = IR.fit(X, self.coarse, assign, kind)
        codes = IR.encode(X, self.coarse, assign, self.params, kind, bits)
        self.offsets, order = oracle.bucket_sort(assign, self.nlist)
        o = order.astype(np.int64)
        self.list_codes = np.ascontiguousarray(codes[o])
        self.list_ids = ids[o].astype(np.uint32)
        list_of = np.repeat(np.arange(self.nlist), sizes)
        self.rec = IR.decode(oracle, self.list_codes, self.coarse, list_of, self.params, kind, bits)
        qa = rng.integers(0, self.nlist, nq)
        qa[2] = 0
        self.Q = (self.coarse[qa] + rng.standard_normal((nq, d)) * 0.7).astype(np.float32)
        self.Q[2] = X[a] + np.float32(0.01)  # the duplicates lead this query's list
        self.rng = rng

    def probes(self, nprobe):
        """Distinct lists per query; query 0: every slot skipped; query 1: some slots skipped
        (0xFFFFFFFF and an id >= nlist); query 2 probes list 0."""
        nq = len(self.Q)
        P = np.stack([self.rng.permutation(self.nlist)[:nprobe] for _ in range(nq)]).astype(np.int64)
        if 0 not in P[2]:
            P[2, 0] = 0
        P[0, :] = NO_ID
        if nprobe >= 2:
            P[1, 0] = NO_ID
        if nprobe >= 3:
            P[1, 2] = self.nlist + 3
        return P

    def expected(self, oracle, P, metric, k):
        return IR.expected(oracle, self.list_codes, self.list_ids, self.offsets, self.coarse, self.params, self.kind,
                           self.bits, self.Q, P, metric, k, rec=self.rec)

    def device(self, dev):
        if not hasattr(self, "_dev"):
            self._dev = dict(Q=_t(self.Q, dev), coarse=_t(self.coarse, dev), offsets=_t(self.offsets, dev),
                             codes=_t(self.list_codes, dev), ids=_t(self.list_ids, dev),
                             params=_params_t(self.params, dev))
        return self._dev

    def search(self, dev, P, metric, k):
        from haag_vq import _native

        D = self.device(dev)
        return _native.ivf_code_search(self.kind, D["Q"], D["coarse"], _t(P.astype(np.uint32), dev), D["offsets"],
                                       D["codes"], D["ids"], D["params"], self.bits, metric, k)


@pytest.mark.parametrize("kind,bits", FORMATS)
@pytest.mark.parametrize("d", [37, 64, 100, 128])
@pytest.mark.parametrize("metric", [IR.L2, IR.IP])
def test_search_is_bit_identical_to_the_rule(dev, oracle, kind, bits, d, metric):
    L = Lists(oracle, kind, bits, d, sizes=[300, 0, 1, 130, 200, 69], seed=metric)
    for nprobe in (1, 3, L.nlist):
        P = L.probes(nprobe)
        for k in (1, 10, 256):  # 256 exceeds the rows of most probes: padding
            want_d, want_i = L.expected(oracle, P, metric, k)
            got_d, got_i = L.search(dev, P, metric, k)
            _same(got_d, got_i, want_d, want_i, f"{kind}{bits} d={d} nprobe={nprobe} k={k}")
            assert (want_i[0] == NO_ID).all() and np.isinf(want_d[0]).all()  # every slot skipped
        if nprobe == L.nlist:
            # ids >= 2^31 rank after the smaller id on equal keys (k = 256; under L2 the planted
            # pair leads query 2's list)
            row = list(want_i[2])
            assert metric == IR.IP or (L.dups[0] in row and L.dups[1] in row)
            if L.dups[0] in row and L.dups[1] in row:
                j = row.index(L.dups[0])
                assert row.index(L.dups[1]) == j + 1 and _bits(want_d[2])[j] == _bits(want_d[2])[j + 1]
        # the order of a query's probe slots does not matter
        perm = np.stack([L.rng.permutation(nprobe) for _ in range(len(P))])
        got2_d, got2_i = L.search(dev, np.take_along_axis(P, perm, axis=1), metric, 10)
        want_d, want_i = L.expected(oracle, P, metric, 10)
        _same(got2_d, got2_i, want_d, want_i, f"{kind}{bits} d={d} nprobe={nprobe} permuted slots")


@pytest.mark.parametrize("kind,bits", [("sq", 8), ("lvq", 4), ("sq", 4), ("lvq", 3)])
@pytest.mark.parametrize("metric", [IR.L2, IR.IP])
def test_search_skewed_lists(dev, oracle, kind, bits, metric):
    """N = 4099 over 4 lists, one of 3000 rows: it crosses every row-range and 512-row step boundary."""
    L = Lists(oracle, kind, bits, 64, sizes=[3000, 1, 0, 1098], seed=40 + metric)
    for nprobe in (1, 2, 4):
        P = L.probes(nprobe)
        P[3:6, 0] = 0  # several queries share the long list
        for a in range(3, 6):
            P[a, 1:] = [l for l in (1, 2, 3)][:nprobe - 1]
        for k in (10, 256):
            want_d, want_i = L.expected(oracle, P, metric, k)
            got_d, got_i = L.search(dev, P, metric, k)
            _same(got_d, got_i, want_d, want_i, f"{kind}{bits} skewed nprobe={nprobe} k={k}")


@pytest.mark.parametrize("kind,bits", FORMATS)
def test_search_wide_rows(dev, oracle, kind, bits):
    L = Lists(oracle, kind, bits, 3072, sizes=[100, 60, 0, 96], seed=5)
    for metric in (IR.L2, IR.IP):
        P = L.probes(4)
        want_d, want_i = L.expected(oracle, P, metric, 10)
        got_d, got_i = L.search(dev, P, metric, 10)
        _same(got_d, got_i, want_d, want_i, f"{kind}{bits} d=3072 metric={metric}")


# the first d past each step of the queries per workgroup (8 -> 4 -> 2 -> 1): the query rows and
# the list's rows (SQ 3, LVQ 2) of d rounded up to 4 floats within 128 KiB
@pytest.mark.parametrize("kind,bits,d", [("sq", 8, 2977), ("sq", 8, 4681), ("sq", 8, 6553),
                                         ("lvq", 4, 3277), ("lvq", 4, 5461), ("lvq", 4, 8193)])
def test_search_past_each_query_block_step(dev, oracle, kind, bits, d):
    rows = 3 if kind == "sq" else 2
    dp = (d + 3) // 4 * 4
    qb = next(q for q in (8, 4, 2, 1) if 4 * dp * (q + rows) <= (128 if q > 1 else 160) * 1024)
    qb_before = next(q for q in (8, 4, 2, 1) if 4 * (dp - 4) * (q + rows) <= (128 if q > 1 else 160) * 1024)
    assert qb_before == 2 * qb, (d, qb, qb_before)
    L = Lists(oracle, kind, bits, d, sizes=[40, 24], seed=9)
    P = L.probes(2)
    want_d, want_i = L.expected(oracle, P, IR.L2, 10)
    got_d, got_i = L.search(dev, P, IR.L2, 10)
    _same(got_d, got_i, want_d, want_i, f"{kind}{bits} d={d} (QB {qb})")


@pytest.mark.parametrize("kind,bits,metric", [("sq", 8, IR.L2), ("lvq", 4, IR.IP)])
def test_search_in_two_chunks_of_queries(dev, oracle, kind, bits, metric):
    """1040 queries x 256 probes x k = 256 do not fit one chunk of the workspace: the size stops
    growing with nq, so at least the last 16 queries go through in a second chunk.  About 500 rows
    over 256 lists (some empty), every query probing every list in its own order; skipped slots
    leave queries of each chunk with fewer than k rows."""
    from haag_vq import _native

    d, k, nq, nlist = 8, 256, 1040, 256
    sizes = [8] + [int(s) for s in np.random.default_rng(bits).integers(0, 5, nlist - 1)]
    assert 0 in sizes and sum(sizes) > k
    fn = getattr(_native.load_library(), f"mivq_ivf_{kind}_search_workspace_bytes")
    assert 0 < fn(nq - 16, sum(sizes), nlist, nlist, d, bits, k) == fn(nq, sum(sizes), nlist, nlist, d, bits, k)
    L = Lists(oracle, kind, bits, d, sizes=sizes, seed=21, nq=nq)
    P = L.probes(nlist)
    P[nq - 3, 9:] = NO_ID
    P[nq - 2, :] = NO_ID
    want_d, want_i = L.expected(oracle, P, metric, k)
    assert (want_i[0] == NO_ID).all() and (want_i[nq - 2] == NO_ID).all() and (want_i[nq - 1] != NO_ID).all()
    assert 0 < (want_i[nq - 3] != NO_ID).sum() < k
    got_d, got_i = L.search(dev, P, metric, k)
    _same(got_d, got_i, want_d, want_i, f"{kind}{bits} two chunks")


# ------------------------------------------------------------------------------ the index
def _factory(kind, bits):
    from haag_vq.methods.lvq_quantization import LVQQuantizer
    from haag_vq.methods.scalar_quantization import ScalarQuantizer

    return (lambda: ScalarQuantizer(num_bits=bits)) if kind == "sq" else (lambda: LVQQuantizer(num_bits=bits))


def _clustered(n, d, seed, nq=9):
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((12, d)) * 2.0
    spread = rng.uniform(0.2, 1.5, d)
    X = (centres[rng.integers(0, 12, n)] + rng.standard_normal((n, d)) * spread).astype(np.float32)
    Q = (centres[rng.integers(0, 12, nq)] + rng.standard_normal((nq, d)) * spread).astype(np.float32)
    return X, Q


@pytest.mark.parametrize("kind,bits", [("sq", 8), ("sq", 16), ("lvq", 4)])
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_index_against_its_engine_and_the_flat_search(dev, kind, bits, metric, tmp_path):
    import torch
    from haag_vq import _native
    from haag_vq.methods.search import IvfQuantizedIndex

    X, Q = _clustered(1500, 37, [bits, 3])
    idx = IvfQuantizedIndex(_factory(kind, bits), K=8, nprobe=1)
    idx.fit(X, metric)
    assert idx.ntotal == 1500
    eng = idx._index
    # search_with_scores: the engine's raw result with the reference's sentinels; IP stays negated
    raw_d, raw_i = eng.search(_t(Q, dev), 256, 1)
    raw_d, raw_i = _h(raw_d), _h(raw_i).view(np.uint32)
    pad = raw_i == NO_ID
    assert pad.any() and not pad.all() and np.isinf(raw_d[pad]).all()  # one list holds fewer than 256 rows
    ids, dists = idx.search_with_scores(Q, 256)
    assert ids.shape == dists.shape == (9, 256) and ids.dtype == np.uint32 and dists.dtype == np.float32
    np.testing.assert_array_equal(ids, raw_i)
    np.testing.assert_array_equal(_bits(dists[~pad]), _bits(raw_d[~pad]))
    fmax = np.finfo(np.float32).max
    assert (dists[pad] == (-fmax if metric == "ip" else fmax)).all()
    assert (np.diff(np.where(pad, fmax, dists), axis=1) >= 0).all()
    dev_d, dev_i = idx.search_device(Q, 256)
    np.testing.assert_array_equal(_bits(_h(dev_d)), _bits(raw_d))
    np.testing.assert_array_equal(idx.search(Q, 10), ids[:, :10])
    e_ids, e_dists = idx.search_with_scores(Q, 0)
    assert e_ids.shape == e_dists.shape == (9, 0) and e_ids.dtype == np.uint32 and e_dists.dtype == np.float32
    # nprobe = K: the flat search over the reconstruction of every row, bit for bit
    idx.nprobe = 8
    rec = eng.reconstruct(torch.arange(1500))
    f_d, f_i = _native.flat_search(_t(Q, dev), rec, 10, _native.METRIC_L2 if metric == "l2" else _native.METRIC_INNER_PRODUCT)
    a_d, a_i = idx.search_device(Q, 10)
    np.testing.assert_array_equal(_h(a_i), _h(f_i))
    np.testing.assert_array_equal(_bits(_h(a_d)), _bits(_h(f_d)))
    # reconstruction_mse: the numpy mean over the decode
    sample = np.array([0, 5, 77, 1499, 300])
    xh = _h(rec)
    for s in (None, sample):
        rows = np.arange(1500) if s is None else s
        want = float(np.mean(np.array([np.mean((X[r] - xh[r]) ** 2) for r in rows], np.float64)))
        assert idx.reconstruction_mse(X, s) == pytest.approx(want, rel=1e-6)
    # memory_footprint: centroids + codes + the per-list parameters
    width, dt = IR.code_shape(kind, bits, 37)
    assert idx.memory_footprint() == 8 * 37 * 4 + 1500 * width * np.dtype(dt).itemsize + (2 if kind == "sq" else 1) * 8 * 37 * 4
    # save / load
    path = tmp_path / "ivfq.npz"
    idx.save(path)
    with np.load(path, allow_pickle=False) as z:  # the file format
        assert sorted(z.files) == sorted(["coarse", "offsets", "codes", "ids", "kind", "bits", "K", "nprobe", "metric", "N",
                                          "D", "param0"] + (["param1"] if kind == "sq" else []))
        # (16-bit SQ rows are written as the int16 they are held in)
        assert z["codes"].dtype == (np.int16 if np.dtype(dt).itemsize == 2 else np.uint8)
        assert z["codes"].shape == (1500, width) and z["ids"].dtype == np.int32
    other = IvfQuantizedIndex(_factory("lvq", 1), K=3, nprobe=2)
    other.load(path)
    assert (other._kind, other._bits, other._K, other.nprobe, other.ntotal) == (kind, bits, 8, 8, 1500)
    o_ids, o_dists = other.search_with_scores(Q, 10)
    w_ids, w_dists = idx.search_with_scores(Q, 10)
    np.testing.assert_array_equal(o_ids, w_ids)
    np.testing.assert_array_equal(_bits(o_dists), _bits(w_dists))
    assert other.reconstruction_mse(X, sample) == idx.reconstruction_mse(X, sample)


def test_index_error_mapping(dev):
    from haag_vq.methods.search import IvfQuantizedIndex

    X, Q = _clustered(700, 8, 1)
    idx = IvfQuantizedIndex(_factory("sq", 8), K=300, nprobe=300)
    with pytest.raises(RuntimeError, match="fit"):
        idx.search_with_scores(Q, 3)
    with pytest.raises(RuntimeError, match="at least as large as number of clusters"):
        idx.fit(X[:299])
    idx.fit(X)
    with pytest.raises(ValueError, match="nprobe=300"):
        idx.search_with_scores(Q, 3)
    with pytest.raises(ValueError, match="nprobe=300"):
        idx.search_device(Q, 3)
    idx.nprobe = 256
    ids, dists = idx.search_with_scores(Q, 3)
    assert ids.shape == (9, 3) and (ids != NO_ID).all()
    for call in (idx.search, idx.search_with_scores, idx.search_device):
        with pytest.raises(ValueError, match="k=257"):
            call(Q, 257)
    with pytest.raises(ValueError, match="metric"):
        idx.fit(X, "cosine")


@pytest.mark.parametrize("name,metric", CASE_IDS)
def test_fixture_cases_end_to_end(dev, oracle, cases, name, metric):
    """The index, handed the fixture's centroids, passes the Judge of every query."""
    from haag_vq.methods.search import IvfQuantizedIndex

    c = cases[(name, metric)]
    idx = IvfQuantizedIndex(_factory(c.kind, c.bits), K=IR.K, nprobe=IR.NPROBE)
    idx.fit(c.X, metric, centroids=c.coarse)
    eng = idx._index
    np.testing.assert_array_equal(_h(eng.lists.offsets), c.offsets)  # the fp32 assignment is the fixture's
    np.testing.assert_array_equal(_h(eng.lists.ids).view(np.uint32), c.list_ids)
    np.testing.assert_array_equal(np.sort(_h(eng.probes(_t(c.Q, dev), IR.NPROBE)), axis=1), np.sort(c.probe_l, axis=1))
    ids, dists = idx.search_with_scores(c.Q, IR.TOPK)
    bad = IR.problems(c.judges, ids, dists, metric, tie_order=True)
    assert not bad, bad[:3]
    want_d, want_i = c.expected(oracle)
    np.testing.assert_array_equal(ids, want_i)
    np.testing.assert_array_equal(_bits(dists), _bits(want_d))
