"""GPU: mivq_rerank_* against the numpy rule (tests/_rerank_rule.py) bit for bit, against the
existing flat searches, on the edge shapes of the candidate list, and RefinedIndex on top."""

import ctypes

import numpy as np
import pytest
import torch

import _rerank_rule as RR

pytestmark = pytest.mark.gpu


def _dev_store(kind, bits, store, dev, misaligned=False):
    """The store as the device tensor the binding takes (SQ-16: int16); `misaligned`: a view one
    element into a larger buffer, so the base is off every wider alignment."""
    a = np.ascontiguousarray(store)
    if kind == "sq" and bits == 16:
        a = a.view(np.int16)
    t = torch.from_numpy(a).to(dev)
    if not misaligned:
        return t
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=dev)
    buf[1:].copy_(t.reshape(-1))
    out = buf[1:].view(t.shape)
    assert out.data_ptr() % (4 * t.element_size()) != 0 and out.is_contiguous()
    return out


def _cand(cand, dev):
    return torch.from_numpy(np.ascontiguousarray(cand, np.uint32).view(np.int32)).to(dev)


def _run(dev, kind, bits, Q, cand, store, params, k, metric, id_offset=0, misaligned=False):
    from haag_vq import _native

    d, i = _native.rerank(kind, torch.from_numpy(np.ascontiguousarray(Q, np.float32)).to(dev), _cand(cand, dev),
                          _dev_store(kind, bits, store, dev, misaligned),
                          tuple(torch.from_numpy(np.ascontiguousarray(p)).to(dev) for p in params), bits, k,
                          RR.METRIC_ID[metric] if isinstance(metric, str) else metric, id_offset)
    return d.cpu().numpy(), i.cpu().numpy().view(np.uint32)


# ------------------------------------------------------------------------------ bit identity
@pytest.mark.parametrize("metric", RR.METRICS)
@pytest.mark.parametrize("fmt,shape", RR.cases())
def test_bit_identical_to_the_rule(dev, fmt, shape, metric):
    c = RR.case(fmt, shape)
    got = _run(dev, c["kind"], c["bits"], c["Q"], c["cand"], c["store"], c["params"], RR.K, metric,
               misaligned=c["misaligned"])
    RR.same(*got, *RR.rerank(c["Q"], c["cand"], c["xh"], 0, RR.METRIC_ID[metric], RR.K), f"{fmt} {shape} {metric}")


@pytest.mark.parametrize("metric", RR.METRICS)
@pytest.mark.parametrize("fmt", ["f32", "sq4", "sq8", "sq16", "lvq4", "lvq8"])
def test_agrees_with_the_flat_searches(dev, fmt, metric):
    """One query's candidates, sorted ascending, gathered into a small database: the existing flat
    search over it reports the same distances bit for bit, and the same rows."""
    from haag_vq import _native

    c = RR.case(fmt, "d64")  # rows of 256 / 32 / 64 / 128 / 40 / 72 bytes: multiples of 4, as gather_rows needs
    mt = RR.METRIC_ID[metric]
    ids = np.sort(c["cand"][0][c["cand"][0] < RR.N])
    store = _dev_store(c["kind"], c["bits"], c["store"], dev)
    small = _native.gather_rows(store, torch.from_numpy(ids.astype(np.int32)).to(dev))
    q = torch.from_numpy(c["Q"][:1]).to(dev)
    params = [torch.from_numpy(p).to(dev) for p in c["params"]]
    if c["kind"] == "f32":
        fd, fi = _native.flat_search(q, small, RR.K, mt)
    elif c["kind"] == "sq":
        fd, fi = _native.sq_flat_search(q, small, c["d"], params[0], params[1], c["bits"], RR.K, mt)
    else:
        fd, fi = _native.lvq_flat_search(q, small, params[0], c["bits"], RR.K, mt)
    got_d, got_i = _native.rerank(c["kind"], q, _cand(c["cand"][:1], dev), store, tuple(params), c["bits"], RR.K, mt)
    RR.same(got_d.cpu().numpy(), got_i.cpu().numpy(), fd.cpu().numpy(), ids[fi.cpu().numpy().astype(np.int64)],
            f"{fmt} {metric}")


# ------------------------------------------------------------------------------ list shapes
D_LIST, N_LIST = 16, 700


@pytest.fixture(scope="module")
def listdb():
    X, Q = RR.rows(N_LIST, D_LIST, 77, nq=3)
    sq = RR.encode("sq", 8, X)
    return dict(X=X, Q=Q, sq=sq, sq_xh=RR.dequant("sq", 8, sq[0], sq[1], D_LIST))


def _both(dev, db, cand, k, metric="l2", id_offset=0, n=N_LIST, Q=None, what=""):
    """f32 and SQ-8 stores of the first n rows against the rule."""
    Q = db["Q"] if Q is None else Q
    mt = RR.METRIC_ID[metric]
    for kind, bits, store, params, xh in (("f32", 0, db["X"], (), db["X"]), ("sq", 8, *db["sq"], db["sq_xh"])):
        got = _run(dev, kind, bits, Q, cand, store[:n], params, k, mt, id_offset)
        RR.same(*got, *RR.rerank(Q, cand, xh[:n], id_offset, mt, k), f"{what} {kind}")
    return got


@pytest.mark.parametrize("r", [1, 63, 64, 65, 600])
def test_list_lengths(dev, listdb, r):
    """One lane, one short of a wave, a wave, one past it, and several strides per lane (600 slots:
    three slices of 256 for this batch)."""
    _both(dev, listdb, RR.lists(3, r, N_LIST, 0, [r, 1], dead=min(3, r - 1)), min(10, r), what=f"r={r}")


def test_k_edges(dev, listdb):
    _both(dev, listdb, RR.lists(3, 90, N_LIST, 0, 2), 1, what="k=1")
    for metric in RR.METRICS:
        _both(dev, listdb, RR.lists(3, 300, N_LIST, 0, 3, dead=7), 256, metric, what=f"k=256 r=300 {metric}")
    d, i = _both(dev, listdb, RR.lists(3, 5, N_LIST, 0, 4), 20, what="k > r")
    assert (i[:, 5:] == RR.NO_ID).all() and np.isinf(d[:, 5:]).all() and (i[:, :5] != RR.NO_ID).all()
    d, i = _both(dev, listdb, RR.lists(3, 70, N_LIST, 0, 5, dead=64), 10, what="k > live")
    assert (i[:, 6:] == RR.NO_ID).all() and (i[:, :6] != RR.NO_ID).all()


def test_dead_slots_and_offsets(dev, listdb):
    cand = RR.lists(3, 40, N_LIST, 0, 6, dead=4)
    cand[1] = RR.NO_ID  # a query whose slots are all padding
    d, i = _both(dev, listdb, cand, 10, what="all padding")
    assert (i[1] == RR.NO_ID).all() and np.isinf(d[1]).all()
    # ids above 2^31 in uint32 order; slots at id_offset - 1, id_offset + n and 0xFFFFFFFF are dead,
    # and so is everything below id_offset (small ids that would be live without the offset)
    off = 2 ** 31 + 5
    cand = RR.lists(3, 80, N_LIST, off, 7, dead=9)
    cand[0, :4] = [0, 5, off - 1, 2 ** 31]
    cand[2, -2:] = [off + N_LIST, 2 ** 32 - 2]
    for metric in RR.METRICS:
        d, i = _both(dev, listdb, cand, 10, metric, id_offset=off, what=f"offset {metric}")
        assert (i >= off).all() and (i < off + N_LIST).all()
    # a store of 200 rows: ids 200 .. 699 are past it
    d, i = _both(dev, listdb, RR.lists(3, 120, N_LIST, 0, 8), 10, n=200, what="n=200")
    assert (i < 200).all()


def test_duplicate_id(dev, listdb):
    cand = RR.lists(3, 50, N_LIST, 0, 9)
    _, want = RR.rerank(listdb["Q"], cand, listdb["X"], 0, RR.L2, 10)
    best = want[0, 0]
    cand[0, 17 if cand[0, 17] != best else 18] = best  # query 0's nearest candidate, a second time
    d, i = _run(dev, "f32", 0, listdb["Q"], cand, listdb["X"], (), 10, "l2")
    RR.same(d, i, *RR.rerank(listdb["Q"], cand, listdb["X"], 0, RR.L2, 10), "duplicate")
    assert i[0, 0] == i[0, 1] == best and d[0, 0] == d[0, 1]
    np.testing.assert_array_equal(i[0, 2:], want[0, 1:9])  # nothing else disturbed
    np.testing.assert_array_equal(i[1:], want[1:])


def test_nan_row_and_nan_query(dev, listdb):
    X = listdb["X"].copy()
    cand = np.random.default_rng(10).permutation(N_LIST)[:36].reshape(3, 12).astype(np.uint32)  # disjoint lists
    X[cand[0, 3], 5] = np.nan
    X[cand[1, 0], 0] = np.nan
    Q = listdb["Q"].copy()
    Q[2, 7] = np.nan
    for metric in RR.METRICS:
        mt = RR.METRIC_ID[metric]
        d, i = _run(dev, "f32", 0, Q, cand, X, (), 12, mt)
        RR.same(d, i, *RR.rerank(Q, cand, X, 0, mt, 12), f"nan {metric}")
        assert i[0, -1] == cand[0, 3] and d[0, -1] == np.inf and np.isfinite(d[0, :-1]).all()
        assert i[1, -1] == cand[1, 0] and d[1, -1] == np.inf
        assert (d[2] == np.inf).all() and (i[2] == np.sort(cand[2])).all()  # every key +inf: id order


def test_empty_batch_and_empty_store(dev, listdb):
    d, i = _run(dev, "f32", 0, listdb["Q"][:0], np.zeros((0, 8), np.uint32), listdb["X"], (), 5, "l2")
    assert d.shape == (0, 5) and i.shape == (0, 5)
    for kind, bits, store, params in (("f32", 0, listdb["X"], ()), ("sq", 8, *listdb["sq"])):
        d, i = _run(dev, kind, bits, listdb["Q"], RR.lists(3, 8, N_LIST, 0, 11), store[:0], params, 5, "l2")
        assert (i == RR.NO_ID).all() and (d == np.inf).all()


def test_many_queries(dev):
    """nq = 70 000 is past the 65 535 a grid's second and third dimensions hold."""
    nq = 70_000
    X, Q = RR.rows(500, 4, 12, nq=nq)
    cand = np.random.default_rng(13).integers(0, 500, (nq, 2)).astype(np.uint32)
    cand[::1000, 0] = RR.NO_ID
    got = _run(dev, "f32", 0, Q, cand, X, (), 1, "l2")
    RR.same(*got, *RR.rerank(Q, cand, X, 0, RR.L2, 1), "nq=70000")


def test_workspace_size(dev, listdb):
    """A workspace of the size query's bytes is accepted and gives the rule's result; one byte less
    is refused.  This does not show that the call stays inside those bytes: the torch blocks here
    and in the wrapper's calls above are padded by the allocator.  tests/test_bounds_search_gpu.py
    runs the entry point in a guarded arena with exactly the reported bytes."""
    from haag_vq import _native

    lib = _native.load_library()
    nq, r, k = 3, 600, 10
    need = lib.mivq_rerank_f32_workspace_bytes(nq, r, k)
    q = torch.from_numpy(listdb["Q"]).to(dev)
    x = torch.from_numpy(listdb["X"]).to(dev)
    cand = _cand(RR.lists(nq, r, N_LIST, 0, 14), dev)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    dd = torch.empty((nq, k), dtype=torch.float32, device=dev)
    ii = torch.empty((nq, k), dtype=torch.int32, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    args = (p(q), nq, p(cand), r, p(x), N_LIST, D_LIST, RR.L2, k, 0)
    assert lib.mivq_rerank_f32(*args, p(ws), need - 1, p(dd), p(ii), None) == _native.MIVQ_ERR_WORKSPACE
    assert lib.mivq_rerank_f32(*args, p(ws), need, p(dd), p(ii), None) == _native.MIVQ_OK
    torch.cuda.synchronize()
    RR.same(dd.cpu().numpy(), ii.cpu().numpy(), *RR.rerank(listdb["Q"], cand.cpu().numpy().view(np.uint32),
                                                           listdb["X"], 0, RR.L2, k), "exact workspace")


# ------------------------------------------------------------------------------ RefinedIndex
@pytest.fixture(scope="module")
def refined(dev):
    """The fitted index of the issue's case, its inputs, the base's lists and the ground truth."""
    from haag_vq import _native
    from haag_vq.methods.product_quantization import ProductQuantizer
    from haag_vq.methods.search import FlatADCIndex, RefinedIndex

    X, Q = RR.index_inputs()
    c = RR.INDEX
    ix = RefinedIndex(FlatADCIndex(ProductQuantizer(M=c["M"], B=8)), None, refine_factor=c["factor"])
    ix.fit(X, "l2")
    _, truth = _native.flat_search(torch.from_numpy(Q).to(dev), torch.from_numpy(X).to(dev), c["k"])
    return dict(ix=ix, X=X, Q=Q, cand=ix.base.search(Q, c["k"] * c["factor"]),
                truth=truth.cpu().numpy().view(np.uint32))


def test_refined_index_is_the_rule_on_the_base_lists(refined):
    c = RR.INDEX
    ids, dists = refined["ix"].search_with_scores(refined["Q"], c["k"])
    assert ids.dtype == np.uint32 and dists.dtype == np.float32 and ids.shape == dists.shape == (c["nq"], c["k"])
    assert refined["cand"].shape == (c["nq"], c["k"] * c["factor"])
    want_d, want_i = RR.rerank(refined["Q"], refined["cand"], refined["X"], 0, RR.L2, c["k"])
    RR.same(dists, ids, want_d, want_i, "f32 store")
    np.testing.assert_array_equal(refined["ix"].search(refined["Q"], c["k"]), ids)


def test_refined_index_recall(refined):
    """Against flat_search's ground truth (the same chain and tie rule) no query loses a hit, by
    construction: the base's top-k is a prefix of its top-r, and a true neighbour among the
    candidates cannot be ranked out by exact distances.  No tolerance.  And the total rises."""
    k = RR.INDEX["k"]
    np.testing.assert_array_equal(refined["ix"].base.search(refined["Q"], k), refined["cand"][:, :k])
    before = RR.hits(refined["cand"][:, :k], refined["truth"])
    after = RR.hits(refined["ix"].search(refined["Q"], k), refined["truth"])
    print(f"hits of {before.size * k}: base {before.sum()}, refined {after.sum()}")
    assert (after >= before).all()
    assert after.sum() > before.sum()


@pytest.mark.parametrize("fmt", ["lvq8", "sq8"])
def test_refined_index_code_stores(dev, refined, fmt):
    from haag_vq.methods.lvq_quantization import LVQQuantizer
    from haag_vq.methods.scalar_quantization import ScalarQuantizer
    from haag_vq.methods.search import RefinedIndex

    c = RR.INDEX
    kind, bits = RR.FORMATS[fmt]
    # the base is fitted already: keep its codebooks
    ix = RefinedIndex(_Fitted(refined["ix"].base), LVQQuantizer(8) if kind == "lvq" else ScalarQuantizer(8), c["factor"])
    ix.fit(refined["X"], "l2")
    store, params = RR.encode(kind, bits, refined["X"])  # the quantizers are bit-identical to numpy
    np.testing.assert_array_equal(ix._store.cpu().numpy().view(np.uint8), np.ascontiguousarray(store).view(np.uint8))
    for got, want in zip(ix._params, params):
        np.testing.assert_array_equal(got.cpu().numpy(), want)
    ids, dists = ix.search_with_scores(refined["Q"], c["k"])
    xh = RR.dequant(kind, bits, store, params, c["D"])
    RR.same(dists, ids, *RR.rerank(refined["Q"], refined["cand"], xh, 0, RR.L2, c["k"]), fmt)
    assert ix.memory_footprint() == refined["ix"].base.memory_footprint() + store.nbytes + sum(p.nbytes for p in params)


class _Fitted:
    """A fitted base index whose fit() is a no-op, so that a second RefinedIndex shares it."""

    def __init__(self, base):
        self._b = base

    def fit(self, X, metric="l2"):
        pass

    def __getattr__(self, name):
        return getattr(self._b, name)


def test_refined_index_inner_product(dev):
    from haag_vq.methods.product_quantization import ProductQuantizer
    from haag_vq.methods.search import FlatADCIndex, RefinedIndex

    X, Q = RR.index_inputs()
    X, Q = X[:1024], Q[:8]
    ix = RefinedIndex(FlatADCIndex(ProductQuantizer(M=4, B=8)), None, refine_factor=5)
    ix.fit(X, "ip")
    ids, scores = ix.search_with_scores(Q, 10)
    assert (np.diff(scores, axis=1) <= 0).all()  # inner products, descending
    want_d, want_i = RR.rerank(Q, ix.base.search(Q, 50), X, 0, RR.IP, 10)
    RR.same(scores, ids, -want_d, want_i, "ip")


def test_refined_index_file_round_trip(refined, tmp_path):
    from haag_vq.methods.product_quantization import ProductQuantizer
    from haag_vq.methods.scalar_quantization import ScalarQuantizer
    from haag_vq.methods.search import FlatADCIndex, RefinedIndex

    c = RR.INDEX
    path = tmp_path / "ix" / "refined.npz"
    refined["ix"].save(path)
    assert path.exists() and (tmp_path / "ix" / "refined.npz.base").exists()
    with np.load(path, allow_pickle=False) as z:  # the file format: an f32 store has no param* entries
        assert sorted(z.files) == sorted(["store", "kind", "bits", "metric", "refine_factor", "N", "D"])
        assert z["store"].dtype == np.float32 and z["store"].shape == (c["N"], c["D"])
    back = RefinedIndex(FlatADCIndex(ProductQuantizer(M=c["M"], B=8)), None, refine_factor=3)
    back.load(path)
    assert back.refine_factor == c["factor"] and back.ntotal == c["N"]
    assert back.memory_footprint() == refined["ix"].memory_footprint() == \
        refined["ix"].base.memory_footprint() + c["N"] * c["D"] * 4
    ids, dists = refined["ix"].search_with_scores(refined["Q"], c["k"])
    RR.same(*back.search_with_scores(refined["Q"], c["k"])[::-1], dists, ids, "round trip")
    with pytest.raises(ValueError, match="holds a f32 store"):
        RefinedIndex(FlatADCIndex(ProductQuantizer(M=c["M"], B=8)), ScalarQuantizer(8)).load(path)


def test_refined_index_over_an_ivf_base_with_padding(dev):
    """IvfQuantizedIndex (LVQ-4, K = 8, one probe) over 400 rows: a probed list holds about 50
    rows, so the 100-slot candidate lists arrive padded with 0xFFFFFFFF."""
    from haag_vq.methods.lvq_quantization import LVQQuantizer
    from haag_vq.methods.search import IvfQuantizedIndex, RefinedIndex

    X, Q = RR.index_inputs()
    X, Q = X[:400], Q[:16]
    ix = RefinedIndex(IvfQuantizedIndex(lambda: LVQQuantizer(4), K=8, nprobe=1), None, refine_factor=10)
    ix.fit(X, "l2")
    cand = ix.base.search(Q, 100)
    assert cand.shape == (16, 100) and (cand == RR.NO_ID).any(axis=1).all()
    ids, dists = ix.search_with_scores(Q, 10)
    want_d, want_i = RR.rerank(Q, cand, X, 0, RR.L2, 10)
    live = want_i != RR.NO_ID
    assert live[:, 0].all()
    want_d[~live] = np.finfo(np.float32).max  # the package's sentinel for slots that could not be filled
    RR.same(dists, ids, want_d, want_i, "ivf base")
