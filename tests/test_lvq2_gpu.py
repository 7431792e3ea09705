"""GPU: two-level LVQ on the device against the numpy rule (tests/_lvq2_rule.py), bit for bit:
mivq_lvq2_encode / mivq_lvq2_decode, mivq_rerank_lvq2 (ranked by tests/_rerank_rule.py over the
rule's reconstruction, and against mivq_lvq2_decode + mivq_flat_search), TwoLevelLVQQuantizer,
LVQ2Index, and FlatQuantizedIndex over the quantizer's generic decode path."""

import ctypes
import functools

import numpy as np
import pytest
import torch

import _lvq2_rule as L2R
import _lvq_rule as LR
import _rerank_rule as RR

pytestmark = pytest.mark.gpu

F32 = np.float32


def _t(a, dev):
    return torch.from_numpy(np.array(a, order="C")).to(dev)  # a copy: the rule's arrays are read-only


def _off_by_one(t, dev):
    """The same values as a view one element into a larger buffer: the base is off every wider alignment."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=dev)
    buf[1:].copy_(t.reshape(-1))
    out = buf[1:].view(t.shape)
    assert out.data_ptr() % (4 * t.element_size()) != 0 and out.is_contiguous()
    return out


def _encode(dev, X, mu, B1, B2):
    from haag_vq import _native

    c1, c2 = _native.lvq2_encode(_t(X, dev), _t(mu, dev), B1, B2)
    return c1.cpu().numpy(), c2.cpu().numpy()


def _same_bits(got, want, what=""):
    np.testing.assert_array_equal(np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32),
                                  err_msg=what)


# ------------------------------------------------------------------------------ encode
@pytest.mark.parametrize("name", list(L2R.CASES))
def test_encode_equals_the_rule(dev, name):
    from haag_vq import _native

    c = L2R.case(name)
    c1, c2 = _encode(dev, c["X"], c["mu"], c["B1"], c["B2"])
    np.testing.assert_array_equal(c1, c["codes1"])
    np.testing.assert_array_equal(c2, c["codes2"])
    np.testing.assert_array_equal(c1, _native.lvq_encode(_t(c["X"], dev), _t(c["mu"], dev), c["B1"]).cpu().numpy())
    assert not L2R.padding_bits2(c2, c["D"], c["B2"]).any()
    p = c["planted"]  # span 0: delta = FLT_MIN, a subnormal delta2
    assert (L2R.unpack2(c2[p:p + 1], c["D"], c["B2"]) == (7 if c["B2"] == 4 else 127)).all()


@pytest.mark.parametrize("name", ["b3x4_d37", "b4x4_d100", "b4x8_d100", "b8x8_d128", "b7x4_d33", "beyond_b3x8_d5000"])
def test_encode_at_misaligned_bases(dev, name):
    """x, codes1 and codes2 each a view one element into a larger buffer (element-wise loads of x, byte
    stores of both arrays), written into the middle of over-allocated buffers whose other rows keep
    their fill."""
    from haag_vq import _native

    c = L2R.case(name)
    n = c["N"]
    s1, s2 = L2R.code_sizes(c["D"], c["B1"], c["B2"])
    x1 = _off_by_one(_t(c["X"], dev), dev)
    b1 = torch.full(((n + 4) * s1 + 1,), 0xA5, dtype=torch.uint8, device=dev)
    b2 = torch.full(((n + 4) * s2 + 1,), 0x5A, dtype=torch.uint8, device=dev)
    o1, o2 = b1[1:].view(n + 4, s1), b2[1:].view(n + 4, s2)
    assert o1.data_ptr() % 2 == 1 and o2.data_ptr() % 2 == 1
    _native.lvq2_encode(x1, _t(c["mu"], dev), c["B1"], c["B2"], out1=o1[2:2 + n], out2=o2[2:2 + n])
    g1, g2 = o1.cpu().numpy(), o2.cpu().numpy()
    np.testing.assert_array_equal(g1[2:2 + n], c["codes1"])
    np.testing.assert_array_equal(g2[2:2 + n], c["codes2"])
    assert (g1[:2] == 0xA5).all() and (g1[2 + n:] == 0xA5).all() and (g2[:2] == 0x5A).all() and (g2[2 + n:] == 0x5A).all()
    assert b1[0].item() == 0xA5 and b2[0].item() == 0x5A


@pytest.mark.parametrize("d", [1, 7, 8, 9, 63, 64, 65])
def test_encode_and_decode_at_small_widths(dev, d):
    from haag_vq import _native

    X, _ = RR.rows(5, d, [5, d])
    mu = LR.seq_mean(X)
    for B1, B2 in L2R.PAIRS:
        w1, w2 = L2R.encode2(X, mu, B1, B2)
        c1, c2 = _encode(dev, X, mu, B1, B2)
        np.testing.assert_array_equal(c1, w1, err_msg=f"{B1}x{B2}")
        np.testing.assert_array_equal(c2, w2, err_msg=f"{B1}x{B2}")
        rec = _native.lvq2_decode(_t(w1, dev), _t(w2, dev), _t(mu, dev), B1, B2).cpu().numpy()
        _same_bits(rec, L2R.decode2(w1, w2, mu, B1, B2), f"{B1}x{B2}")


@pytest.mark.parametrize("exp", [-70, -62, -58, 48, 52, 60])
def test_encode_where_the_fast_quotient_ends(dev, exp):
    """Rows scaled by 2^exp: the encoder divides by reciprocal and correction while delta <= 2^50 and
    delta2 >= 2^-60 and in IEEE otherwise; the fields are the rule's on either side (2^-70 and 2^60
    are outside, -62 / -58 and 48 / 52 straddle the two ends for some of the widths)."""
    from haag_vq import _native

    X, _ = RR.rows(4, 64, [4, 64])
    X = (X * F32(2.0 ** exp)).astype(F32)
    mu = LR.seq_mean(X)
    for B1, B2 in L2R.PAIRS:
        w1, w2 = L2R.encode2(X, mu, B1, B2)
        c1, c2 = _encode(dev, X, mu, B1, B2)
        np.testing.assert_array_equal(c1, w1, err_msg=f"{B1}x{B2}")
        np.testing.assert_array_equal(c2, w2, err_msg=f"{B1}x{B2}")
        np.testing.assert_array_equal(c1, _native.lvq_encode(_t(X, dev), _t(mu, dev), B1).cpu().numpy())
        rec = _native.lvq2_decode(_t(w1, dev), _t(w2, dev), _t(mu, dev), B1, B2).cpu().numpy()
        _same_bits(rec, L2R.decode2(w1, w2, mu, B1, B2), f"{B1}x{B2}")


@pytest.mark.parametrize("B2", [4, 8])
def test_planted_ties_round_half_to_even(dev, B2):
    lead, want_idx, want_j = L2R.TIES[B2]
    for D in (len(lead), 37):
        row, _, _ = L2R.tie_row(B2, D)
        mu = np.zeros(D, F32)
        c1, c2 = _encode(dev, row[None, :], mu, L2R.TIE_B1, B2)
        idx, _, _ = LR.unpack(c1, D, L2R.TIE_B1)
        assert idx[0, :len(lead)].tolist() == want_idx
        assert L2R.unpack2(c2, D, B2)[0, :len(lead)].tolist() == want_j
        w1, w2 = L2R.encode2(row[None, :], mu, L2R.TIE_B1, B2)
        np.testing.assert_array_equal(c1, w1)
        np.testing.assert_array_equal(c2, w2)


# ------------------------------------------------------------------------------ decode
@pytest.mark.parametrize("name", list(L2R.CASES))
def test_decode_equals_the_rule(dev, name):
    from haag_vq import _native

    c = L2R.case(name)
    mu = _t(c["mu"], dev)
    rec = _native.lvq2_decode(_t(c["codes1"], dev), _t(c["codes2"], dev), mu, c["B1"], c["B2"]).cpu().numpy()
    _same_bits(rec, c["rec"], name)
    # both arrays at misaligned bases: byte loads
    out = _native.lvq2_decode(_off_by_one(_t(c["codes1"], dev), dev), _off_by_one(_t(c["codes2"], dev), dev), mu,
                              c["B1"], c["B2"])
    _same_bits(out.cpu().numpy(), c["rec"], name + " misaligned")


@pytest.mark.parametrize("name", ["b4x8_d100", "b3x4_d37", "beyond_b3x8_d5000"])
def test_quantizer_round_trip(dev, name):
    from haag_vq.methods.lvq2_quantization import TwoLevelLVQQuantizer

    c = dict(L2R.case(name))
    c["X"] = c["X"].copy()  # writable: the class hands numpy inputs to torch as they are
    q = TwoLevelLVQQuantizer(c["B1"], c["B2"])
    q.fit(c["X"])
    _same_bits(q.mu, c["mu"])
    assert q.primary().num_bits == c["B1"] and q.primary().mu is q.mu
    want = np.concatenate([c["codes1"], c["codes2"]], axis=1)
    host = q.compress(c["X"])
    assert isinstance(host, np.ndarray) and host.shape == (c["N"], q.code_size(c["D"]))
    np.testing.assert_array_equal(host, want)
    devc = q.compress(_t(c["X"], dev))
    assert isinstance(devc, torch.Tensor) and devc.is_contiguous()
    np.testing.assert_array_equal(devc.cpu().numpy(), want)
    s1, s2 = q.split(devc)
    np.testing.assert_array_equal(s1.cpu().numpy(), c["codes1"])
    np.testing.assert_array_equal(s2.cpu().numpy(), c["codes2"])
    np.testing.assert_array_equal(q.primary().compress(c["X"]), c["codes1"])
    rec = q.decompress(host)
    assert isinstance(rec, np.ndarray) and rec.dtype == F32
    _same_bits(rec, c["rec"])
    _same_bits(q.decompress(devc).cpu().numpy(), c["rec"])
    ids = np.random.default_rng(5).permutation(c["N"])[:7]  # row-independent, as FaissQuantizerAdapter indexes
    _same_bits(q.decompress(host[ids]), c["rec"][ids])


# ------------------------------------------------------------------------------ re-rank: bit identity
@functools.lru_cache(maxsize=None)
def _rr_case(B1, B2, shape):
    d, mis = RR.SHAPES[shape]
    X, Q = RR.rows(RR.N, d, [RR.N, d, B1, B2])
    mu = LR.seq_mean(X)
    c1, c2 = L2R.encode2(X, mu, B1, B2)
    return dict(d=d, mis=mis, Q=Q, mu=mu, c1=c1, c2=c2, xh=L2R.decode2(c1, c2, mu, B1, B2),
                cand=RR.lists(RR.NQ, RR.R, RR.N, 0, [RR.R, d, B1, B2], dead=5))


def _cand(cand, dev):
    return _t(np.ascontiguousarray(cand, np.uint32).view(np.int32), dev)


def _rerank(dev, Q, cand, c1, c2, mu, B1, B2, k, metric, id_offset=0, mis=False):
    from haag_vq import _native

    t1, t2 = _t(c1, dev), _t(c2, dev)
    if mis:
        t1, t2 = _off_by_one(t1, dev), _off_by_one(t2, dev)
    d, i = _native.rerank_lvq2(_t(np.ascontiguousarray(Q, F32), dev), _cand(cand, dev), t1, t2, _t(mu, dev), B1, B2, k,
                               RR.METRIC_ID[metric] if isinstance(metric, str) else metric, id_offset)
    return d.cpu().numpy(), i.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("metric", RR.METRICS)
@pytest.mark.parametrize("shape", list(RR.SHAPES))
@pytest.mark.parametrize("B1,B2", L2R.PAIRS)
def test_rerank_bit_identical_to_the_rule(dev, B1, B2, shape, metric):
    c = _rr_case(B1, B2, shape)
    got = _rerank(dev, c["Q"], c["cand"], c["c1"], c["c2"], c["mu"], B1, B2, RR.K, metric, mis=c["mis"])
    RR.same(*got, *RR.rerank(c["Q"], c["cand"], c["xh"], 0, RR.METRIC_ID[metric], RR.K), f"{B1}x{B2} {shape} {metric}")


@pytest.mark.parametrize("metric", RR.METRICS)
@pytest.mark.parametrize("B1,B2", L2R.PAIRS)
def test_rerank_agrees_with_decode_and_flat_search(dev, B1, B2, metric):
    """One query's candidates, sorted ascending, decoded by mivq_lvq2_decode into a small f32 database:
    mivq_flat_search over it reports the same distances bit for bit, and the same rows."""
    from haag_vq import _native

    c = _rr_case(B1, B2, "d64")
    mt = RR.METRIC_ID[metric]
    ids = np.sort(c["cand"][0][c["cand"][0] < RR.N])
    mu = _t(c["mu"], dev)
    small = _native.lvq2_decode(_t(c["c1"][ids], dev), _t(c["c2"][ids], dev), mu, B1, B2)
    q = _t(c["Q"][:1], dev)
    fd, fi = _native.flat_search(q, small, RR.K, mt)
    gd, gi = _native.rerank_lvq2(q, _cand(c["cand"][:1], dev), _t(c["c1"], dev), _t(c["c2"], dev), mu, B1, B2, RR.K, mt)
    RR.same(gd.cpu().numpy(), gi.cpu().numpy(), fd.cpu().numpy(), ids[fi.cpu().numpy().astype(np.int64)],
            f"{B1}x{B2} {metric}")


# ------------------------------------------------------------------------------ re-rank: list and argument edges
D_LIST, N_LIST = 16, 700


@pytest.fixture(scope="module")
def listdb():
    X, Q = RR.rows(N_LIST, D_LIST, 78, nq=3)
    mu = LR.seq_mean(X)
    out = dict(Q=Q, mu=mu)
    for pair in ((4, 8), (3, 4)):
        c1, c2 = L2R.encode2(X, mu, *pair)
        out[pair] = (c1, c2, L2R.decode2(c1, c2, mu, *pair))
    return out


def _both(dev, db, cand, k, metric="l2", id_offset=0, n=N_LIST, Q=None, what=""):
    """LVQ-4x8 and LVQ-3x4 stores of the first n rows against the rule."""
    Q = db["Q"] if Q is None else Q
    mt = RR.METRIC_ID[metric]
    for pair in ((4, 8), (3, 4)):
        c1, c2, xh = db[pair]
        got = _rerank(dev, Q, cand, c1[:n], c2[:n], db["mu"], *pair, k, mt, id_offset)
        RR.same(*got, *RR.rerank(Q, cand, xh[:n], id_offset, mt, k), f"{what} {pair}")
    return got


@pytest.mark.parametrize("r", [1, 63, 64, 65, 600])
def test_list_lengths(dev, listdb, r):
    _both(dev, listdb, RR.lists(3, r, N_LIST, 0, [r, 2], dead=min(3, r - 1)), min(10, r), what=f"r={r}")


def test_k_edges(dev, listdb):
    _both(dev, listdb, RR.lists(3, 90, N_LIST, 0, 22), 1, what="k=1")
    for metric in RR.METRICS:
        _both(dev, listdb, RR.lists(3, 300, N_LIST, 0, 23, dead=7), 256, metric, what=f"k=256 r=300 {metric}")
    d, i = _both(dev, listdb, RR.lists(3, 5, N_LIST, 0, 24), 20, what="k > r")
    assert (i[:, 5:] == RR.NO_ID).all() and np.isinf(d[:, 5:]).all() and (i[:, :5] != RR.NO_ID).all()


def test_dead_slots_and_offsets(dev, listdb):
    cand = RR.lists(3, 40, N_LIST, 0, 26, dead=4)
    cand[1] = RR.NO_ID  # a query whose slots are all padding
    d, i = _both(dev, listdb, cand, 10, what="all padding")
    assert (i[1] == RR.NO_ID).all() and np.isinf(d[1]).all()
    off = 2 ** 31 + 5
    cand = RR.lists(3, 80, N_LIST, off, 27, dead=9)
    cand[0, :4] = [0, 5, off - 1, 2 ** 31]  # below id_offset
    cand[2, -2:] = [off + N_LIST, 2 ** 32 - 2]  # at and past id_offset + n
    for metric in RR.METRICS:
        d, i = _both(dev, listdb, cand, 10, metric, id_offset=off, what=f"offset {metric}")
        assert (i >= off).all() and (i < off + N_LIST).all()
    d, i = _both(dev, listdb, RR.lists(3, 120, N_LIST, 0, 28), 10, n=200, what="n=200")  # ids 200 .. 699 are past the store
    assert (i < 200).all()


def test_duplicate_id(dev, listdb):
    c1, c2, xh = listdb[(4, 8)]
    cand = RR.lists(3, 50, N_LIST, 0, 29)
    _, want = RR.rerank(listdb["Q"], cand, xh, 0, RR.L2, 10)
    best = want[0, 0]
    cand[0, 17 if cand[0, 17] != best else 18] = best  # query 0's nearest candidate, a second time
    d, i = _rerank(dev, listdb["Q"], cand, c1, c2, listdb["mu"], 4, 8, 10, "l2")
    RR.same(d, i, *RR.rerank(listdb["Q"], cand, xh, 0, RR.L2, 10), "duplicate")
    assert i[0, 0] == i[0, 1] == best and d[0, 0] == d[0, 1]


def test_nan_query(dev, listdb):
    Q = listdb["Q"].copy()
    Q[2, 7] = np.nan
    cand = np.random.default_rng(30).permutation(N_LIST)[:36].reshape(3, 12).astype(np.uint32)
    for metric in RR.METRICS:
        d, i = _both(dev, listdb, cand, 12, metric, Q=Q, what=f"nan {metric}")
        assert (d[2] == np.inf).all() and (i[2] == np.sort(cand[2])).all()  # every key +inf: id order
        assert np.isfinite(d[:2]).all()


def test_empty_batch_and_empty_store(dev, listdb):
    c1, c2, _ = listdb[(4, 8)]
    d, i = _rerank(dev, listdb["Q"][:0], np.zeros((0, 8), np.uint32), c1, c2, listdb["mu"], 4, 8, 5, "l2")
    assert d.shape == (0, 5) and i.shape == (0, 5)
    d, i = _rerank(dev, listdb["Q"], RR.lists(3, 8, N_LIST, 0, 31), c1[:0], c2[:0], listdb["mu"], 4, 8, 5, "l2")
    assert (i == RR.NO_ID).all() and (d == np.inf).all()


def test_many_queries(dev):
    """nq = 70 000 is past the 65 535 a grid's second and third dimensions hold."""
    nq, d = 70_000, 8
    X, Q = RR.rows(500, d, 32, nq=nq)
    mu = LR.seq_mean(X)
    c1, c2 = L2R.encode2(X, mu, 4, 4)
    cand = np.random.default_rng(33).integers(0, 500, (nq, 4)).astype(np.uint32)
    cand[::1000, 0] = RR.NO_ID
    got = _rerank(dev, Q, cand, c1, c2, mu, 4, 4, 1, "l2")
    RR.same(*got, *RR.rerank(Q, cand, L2R.decode2(c1, c2, mu, 4, 4), 0, RR.L2, 1), "nq=70000")


def test_workspace_size(dev, listdb):
    """The size query's bytes are enough; one byte less is refused."""
    from haag_vq import _native

    lib = _native.load_library()
    c1, c2, xh = listdb[(4, 8)]
    nq, r, k = 3, 600, 10
    need = lib.mivq_rerank_lvq2_workspace_bytes(nq, r, k)
    q, mu, t1, t2 = _t(listdb["Q"], dev), _t(listdb["mu"], dev), _t(c1, dev), _t(c2, dev)
    cand = RR.lists(nq, r, N_LIST, 0, 34)
    cd = _cand(cand, dev)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    dd = torch.empty((nq, k), dtype=torch.float32, device=dev)
    ii = torch.empty((nq, k), dtype=torch.int32, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    args = (p(q), nq, p(cd), r, p(t1), p(t2), N_LIST, D_LIST, p(mu), 4, 8, RR.L2, k, 0)
    assert lib.mivq_rerank_lvq2(*args, p(ws), need - 1, p(dd), p(ii), None) == _native.MIVQ_ERR_WORKSPACE
    assert lib.mivq_rerank_lvq2(*args, p(ws), need, p(dd), p(ii), None) == _native.MIVQ_OK
    torch.cuda.synchronize()
    RR.same(dd.cpu().numpy(), ii.cpu().numpy(), *RR.rerank(listdb["Q"], cand, xh, 0, RR.L2, k), "exact workspace")


# ------------------------------------------------------------------------------ LVQ2Index
@functools.lru_cache(maxsize=None)
def _index_rule(B1, B2):
    """b4_d100's inputs under the rule at (B1, B2): mu, both arrays, the reconstruction."""
    X, Q, _ = LR.inputs("b4_d100")
    mu = X.mean(axis=0)
    c1, c2 = L2R.encode2(X, mu, B1, B2)
    return dict(X=X, Q=Q, mu=mu, c1=c1, c2=c2, xh=L2R.decode2(c1, c2, mu, B1, B2))


@pytest.mark.parametrize("metric", RR.METRICS)
@pytest.mark.parametrize("B1,B2,f", [(4, 4, 4), (2, 8, 10)])
def test_index_is_the_rule_on_the_primary_lists(dev, B1, B2, f, metric):
    from haag_vq import _native
    from haag_vq.methods.search import LVQ2Index

    c = _index_rule(B1, B2)
    k, mt = 10, RR.METRIC_ID[metric]
    ix = LVQ2Index(B1, B2, refine_factor=f)
    ix.fit(c["X"], metric)
    assert ix.ntotal == 1500
    np.testing.assert_array_equal(ix._codes1.cpu().numpy(), c["c1"])
    np.testing.assert_array_equal(ix._codes2.cpu().numpy(), c["c2"])
    assert ix.memory_footprint() == c["c1"].nbytes + c["c2"].nbytes + c["mu"].nbytes
    ids, scores = ix.search_with_scores(c["Q"], k)
    assert ids.dtype == np.uint32 and scores.dtype == F32 and ids.shape == scores.shape == (16, k)
    # the primary search's own lists, then the rule
    _, cand = _native.lvq_flat_search(_t(c["Q"], dev), _t(c["c1"], dev), _t(c["mu"], dev), B1, k * f, mt)
    cand = cand.cpu().numpy().view(np.uint32)
    want_d, want_i = RR.rerank(c["Q"], cand, c["xh"], 0, mt, k)
    RR.same(scores if metric == "l2" else -scores, ids, want_d, want_i, f"{B1}x{B2} f={f} {metric}")
    np.testing.assert_array_equal(ix.search(c["Q"], k), ids)
    if metric == "ip":
        assert (np.diff(scores, axis=1) <= 0).all()  # inner products, descending
        return
    assert (np.diff(scores, axis=1) >= 0).all()
    _, truth = _native.flat_search(_t(c["Q"], dev), _t(c["X"], dev), k, mt)
    truth = truth.cpu().numpy().view(np.uint32)
    before, after = RR.hits(cand[:, :k], truth).sum(), RR.hits(ids, truth).sum()
    print(f"LVQ-{B1}x{B2} f={f}: hits of {16 * k}: primary {before}, two-level {after}")
    assert after > before


def test_index_caps_r_at_n_and_pads(dev):
    from haag_vq.methods.search import LVQ2Index

    X, Q, _ = LR.inputs("b8_tiny")  # 7 rows
    for metric, sentinel in (("l2", np.finfo(F32).max), ("ip", -np.finfo(F32).max)):
        ix = LVQ2Index(8, 8, refine_factor=10)
        ix.fit(X, metric)
        assert ix.candidate_count(10) == 7
        ids, scores = ix.search_with_scores(Q, 10)
        assert ids.shape == scores.shape == (3, 10)
        assert (ids[:, 7:] == RR.NO_ID).all() and (scores[:, 7:] == sentinel).all()
        assert (np.sort(ids[:, :7], axis=1) == np.arange(7)).all()
        mu = X.mean(axis=0)
        xh = L2R.decode2(*L2R.encode2(X, mu, 8, 8), mu, 8, 8)
        want_d, want_i = RR.rerank(Q, np.tile(np.arange(7, dtype=np.uint32), (3, 1)), xh, 0, RR.METRIC_ID[metric], 7)
        RR.same(scores[:, :7] if metric == "l2" else -scores[:, :7], ids[:, :7], want_d, want_i, metric)
    assert ix.search_with_scores(Q, 0)[0].shape == (3, 0) and ix.search_with_scores(Q[:0], 5)[0].shape == (0, 5)


def test_index_file_round_trip(dev, tmp_path):
    from haag_vq.methods.search import LVQ2Index

    c = _index_rule(4, 4)
    ix = LVQ2Index(4, 4, refine_factor=4)
    ix.fit(c["X"], "ip")
    path = tmp_path / "ix" / "lvq2.npz"
    ix.save(path)
    with np.load(path, allow_pickle=False) as z:  # the file format
        assert sorted(z.files) == sorted(["codes1", "codes2", "mu", "primary_bits", "residual_bits", "metric",
                                          "refine_factor", "N", "D"])
        assert z["codes1"].dtype == np.uint8 and z["codes2"].dtype == np.uint8
    back = LVQ2Index(4, 4, refine_factor=9)
    back.load(path)
    assert back.refine_factor == 4 and back.ntotal == 1500 and back.memory_footprint() == ix.memory_footprint()
    ids, scores = ix.search_with_scores(c["Q"], 10)
    RR.same(*back.search_with_scores(c["Q"], 10)[::-1], scores, ids, "round trip")
    with pytest.raises(ValueError, match="holds LVQ-4x4 codes"):
        LVQ2Index(4, 8).load(path)


def test_flat_quantized_index_takes_the_decode_path(dev):
    """No special case for the two-level quantizer in FlatQuantizedIndex: the generic path decodes and
    runs the exact f32 search, so its ids are mivq_flat_search's over the rule's reconstruction."""
    from haag_vq import _native
    from haag_vq.methods.lvq2_quantization import TwoLevelLVQQuantizer
    from haag_vq.methods.search import FlatQuantizedIndex

    c = _index_rule(4, 8)
    ix = FlatQuantizedIndex(TwoLevelLVQQuantizer(4, 8))
    ix.fit(c["X"], "l2")
    assert ix.memory_footprint() == c["c1"].nbytes + c["c2"].nbytes
    np.testing.assert_array_equal(ix._codes.cpu().numpy(), np.concatenate([c["c1"], c["c2"]], axis=1))
    ids, dists = ix.search_with_scores(c["Q"], 10)
    fd, fi = _native.flat_search(_t(c["Q"], dev), _t(c["xh"], dev), 10, RR.L2)
    RR.same(dists, ids, fd.cpu().numpy(), fi.cpu().numpy().view(np.uint32), "generic path")
