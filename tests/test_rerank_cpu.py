"""CPU: the re-ranking rule against brute force, the host logic of RefinedIndex, and the argument
checks of mivq_rerank_* (made before any HIP call)."""

import ctypes

import numpy as np
import pytest

import _rerank_rule as RR
import _search_rule as SR


# ------------------------------------------------------------------------------ the rule
def test_fma32_is_the_fused_operation():
    """One rounding: the product is not rounded, a tie goes to even, and a sum that becomes a
    float32 tie only through the float64 rounding goes the way of the exact sum."""
    one = np.ones(1, np.float32)
    a = np.float32(1.0 + 2.0 ** -12) * one  # a a = 1 + 2^-11 + 2^-24, rounded: 1 + 2^-11
    assert RR.fma32(a, a, -(a * a))[0] == np.float32(2.0 ** -24)
    h = np.float32(2.0 ** -12) * one
    assert RR.fma32(h, h, np.float32(1.0 + 2.0 ** -23) * one)[0] == np.float32(1.0 + 2.0 ** -22)  # a tie: to even
    # 4097 x 16773121 = 2^36 + 1: the product is 2^-24 + 2^-60, and 1 + 2^-24 + 2^-60 lies above the
    # tie 1 + 2^-24 that the float64 sum rounds it to
    x, y = np.float32(4097 * 2.0 ** -30) * one, np.float32(16773121 * 2.0 ** -30) * one
    assert float(x[0]) * float(y[0]) == 2.0 ** -24 + 2.0 ** -60
    assert RR.fma32(x, y, one)[0] == np.float32(1.0 + 2.0 ** -23)
    assert RR.fma32(-x, y, -one)[0] == np.float32(-1.0 - 2.0 ** -23)


@pytest.mark.parametrize("metric", RR.METRICS)
@pytest.mark.parametrize("fmt,shape", RR.cases())
def test_rule_is_flat_search_restricted_to_the_candidates(oracle, fmt, shape, metric):
    """On every case: rank all rows with the oracle's flat search (C fmaf chains; SQ rows decoded by
    the oracle), keep the rows that are candidates, and the first k of those are the rule's output."""
    c = RR.case(fmt, shape)
    mt = RR.METRIC_ID[metric]
    if c["kind"] == "sq":
        xh = oracle.sq_decode(c["store"], c["d"], c["params"][0], c["params"][1], c["bits"])
        np.testing.assert_array_equal(xh.view(np.uint32), c["xh"].view(np.uint32))
    else:
        xh = c["xh"]
    all_d, all_i = oracle.flat_search(c["Q"], xh, RR.N, mt)
    got_d, got_i = RR.rerank(c["Q"], c["cand"], c["xh"], 0, mt, RR.K)
    for a in range(RR.NQ):
        keep = np.isin(all_i[a], c["cand"][a])
        assert keep.sum() == RR.R - 5  # the case's 5 dead slots
        RR.same(got_d[a], got_i[a], all_d[a][keep][:RR.K], all_i[a][keep][:RR.K], f"{fmt} {shape} {metric} q{a}")


def test_rule_filters_pads_and_keeps_duplicates():
    X, Q = RR.rows(20, 8, 1, nq=2)
    off = 2 ** 31 + 5
    cand = np.array([[off + 3, off + 3, RR.NO_ID, off - 1, off + 20, off + 19],
                     [RR.NO_ID] * 6], np.uint32)
    d, i = RR.rerank(Q, cand, X, off, RR.L2, 5)
    assert sorted(i[0][:3].tolist()) == [off + 3, off + 3, off + 19] and (i[0][3:] == RR.NO_ID).all()
    assert np.isinf(d[0][3:]).all() and (i[1] == RR.NO_ID).all() and np.isinf(d[1]).all()
    assert d[0][0] <= d[0][1] <= d[0][2]
    X[4] = np.nan
    d, i = RR.rerank(Q, np.array([[4, 7, RR.NO_ID], [7, 4, 2]], np.uint32), X, 0, RR.IP, 3)
    assert i[0].tolist() == [7, 4, RR.NO_ID] and np.isinf(d[0][1]) and i[1][2] == 4
    d, i = RR.rerank(Q, np.array([[1, 2]] * 2, np.uint32), X[:0], 0, RR.L2, 3)
    assert (i == RR.NO_ID).all() and np.isinf(d).all()


# ------------------------------------------------------------------------------ the recall property
def _standin_base(X, Q, r):
    """A first stage that needs no device: PQ M = 4 codes against seeded codebooks of 256 data rows
    per subspace, ranked by the exact distance to the reconstruction."""
    M, D = RR.INDEX["M"], X.shape[1]
    pick = np.random.default_rng(RR.INDEX["seed"] + 1).permutation(len(X))[:256]
    C = np.ascontiguousarray(X[pick].reshape(256, M, D // M).transpose(1, 0, 2))
    xh = SR.table_decompress(SR.table_compress(X, C), C)
    _, ids = RR.rerank(Q, np.tile(np.arange(len(X), dtype=np.uint32), (len(Q), 1)), xh, 0, RR.L2, r)
    return ids


def test_reranking_never_loses_a_neighbour_and_gains_some():
    """The property tests/test_rerank_gpu.py asserts for RefinedIndex, on the rule alone: with the
    ground truth ranked by the same chains and tie rule, every query's hit count after re-ranking
    the base's top-r is at least that of the base's top-k, and the total is strictly larger."""
    X, Q = RR.index_inputs()
    k, r = RR.INDEX["k"], RR.INDEX["k"] * RR.INDEX["factor"]
    everyone = np.tile(np.arange(len(X), dtype=np.uint32), (len(Q), 1))
    _, truth = RR.rerank(Q, everyone, X, 0, RR.L2, k)
    cand = _standin_base(X, Q, r)
    _, refined = RR.rerank(Q, cand, X, 0, RR.L2, k)
    before, after = RR.hits(cand[:, :k], truth), RR.hits(refined, truth)
    print(f"hits of {len(Q) * k}: base {before.sum()}, refined {after.sum()}")
    assert (after >= before).all()
    assert after.sum() > before.sum()


# ------------------------------------------------------------------------------ RefinedIndex, host logic
class _StubBase:
    """A base index that needs no device: it records what it is asked."""

    def __init__(self):
        self.asked, self.loaded, self.fitted = [], None, None

    def fit(self, X, metric="l2"):
        self.fitted = metric

    def search(self, Q, k):
        self.asked.append(k)
        return np.zeros((len(Q), k), np.uint32)

    def memory_footprint(self):
        return 1000

    def reconstruction_mse(self, X, sample_ids=None):
        return 0.25

    def save(self, path):
        pass

    def load(self, path):
        self.loaded = str(path)


def test_refined_index_constructor_refusals():
    from haag_vq.methods.lvq_quantization import LVQQuantizer
    from haag_vq.methods.product_quantization import ProductQuantizer
    from haag_vq.methods.scalar_quantization import ScalarQuantizer
    from haag_vq.methods.search import RefinedIndex

    for ok in (None, ScalarQuantizer(4), ScalarQuantizer(16), LVQQuantizer(1), LVQQuantizer(8)):
        RefinedIndex(_StubBase(), ok, refine_factor=1)
    with pytest.raises(ValueError, match="ProductQuantizer"):
        RefinedIndex(_StubBase(), ProductQuantizer(M=4, B=8))
    for bad in (0, -3):
        with pytest.raises(ValueError, match="refine_factor"):
            RefinedIndex(_StubBase(), None, refine_factor=bad)
    ix = RefinedIndex(_StubBase(), None, 4)
    assert ix.memory_footprint() == 1000 and ix.reconstruction_mse(None) == 0.25


def test_refined_index_candidate_count():
    from haag_vq.methods.search import RefinedIndex

    ix = RefinedIndex(_StubBase(), None, refine_factor=10)
    ix._N = 4096
    assert ix.candidate_count(10) == 100 and ix.candidate_count(25) == 250
    with pytest.raises(ValueError, match=r"26 \* 10 = 260.*at most 256"):
        ix.candidate_count(26)
    with pytest.raises(ValueError, match="at most 256"):
        ix.search_with_scores(np.zeros((2, 8), np.float32), 26)  # refused before the base is asked
    assert ix.base.asked == []
    ix._N = 37
    assert ix.candidate_count(10) == 37  # r is capped at N
    assert RefinedIndex(_StubBase(), None, refine_factor=1).candidate_count(256) == 0  # nothing fitted


def test_refined_index_load_refuses_another_store_kind(tmp_path):
    from haag_vq.methods.lvq_quantization import LVQQuantizer
    from haag_vq.methods.scalar_quantization import ScalarQuantizer
    from haag_vq.methods.search import RefinedIndex

    path = tmp_path / "refined.npz"
    with open(path, "wb") as f:
        np.savez(f, store=np.zeros((3, 12), np.uint8), kind=np.array("lvq"), bits=np.array(4), metric=np.array("l2"),
                 refine_factor=np.array(10), N=np.array(3), D=np.array(8), param0=np.zeros(8, np.float32))
    for refine in (None, ScalarQuantizer(4), LVQQuantizer(8)):
        base = _StubBase()
        with pytest.raises(ValueError, match="holds a lvq store of 4 bits"):
            RefinedIndex(base, refine).load(path)
        assert base.loaded is None  # refused before the base is touched


# ------------------------------------------------------------------------------ the C ABI
def _fake(n=16):
    return ctypes.c_void_p(n)  # non-null, never dereferenced: every check below precedes the launch


def test_rerank_argument_errors_need_no_gpu():
    from haag_vq import _native

    lib = _native.load_library()
    p = _fake()
    INV, UNS, WS = _native.MIVQ_ERR_INVALID, _native.MIVQ_ERR_UNSUPPORTED, _native.MIVQ_ERR_WORKSPACE

    def f32(nq=2, r=4, n=10, d=8, metric=1, k=3, off=0, q=p, cand=p, x=p, ws=p, nb=1 << 20, out=p):
        return lib.mivq_rerank_f32(q, nq, cand, r, x, n, d, metric, k, off, ws, nb, out, out, None)

    def sq(nbits, nq=2, r=4, n=10, d=8, k=3, codes=p, lo=p):
        return lib.mivq_rerank_sq(p, nq, p, r, codes, n, d, lo, p, nbits, 1, k, 0, p, 1 << 20, p, p, None)

    def lvq(nbits, nq=2, r=4, n=10, d=8, k=3, mu=p):
        return lib.mivq_rerank_lvq(p, nq, p, r, p, n, d, mu, nbits, 1, k, 0, p, 1 << 20, p, p, None)

    for bad in (dict(nq=-1), dict(n=-1), dict(r=0), dict(d=0), dict(q=None), dict(cand=None), dict(x=None),
                dict(out=None), dict(off=-1), dict(off=2 ** 32 - 5)):
        assert f32(**bad) == INV, bad
    assert b"rerank_f32" in lib.mivq_last_error()
    for bad in (dict(k=0), dict(k=257), dict(metric=7), dict(d=40964)):
        assert f32(**bad) == UNS, bad
    with pytest.raises(ValueError):
        _native._raise(UNS)
    need = lib.mivq_rerank_f32_workspace_bytes(2, 4, 3)
    assert need > 0 and f32(nb=need - 1) == WS and f32(ws=None) == WS
    with pytest.raises(RuntimeError, match="workspace"):
        _native._raise(WS)
    assert f32(nq=0, q=None, cand=None, x=None, ws=None, nb=0, out=None) == _native.MIVQ_OK  # nothing to do

    for nbits in (0, 5, 32):
        assert sq(nbits) == UNS
    for nbits in (0, 9):
        assert lvq(nbits) == UNS
    assert sq(8, r=0) == INV and sq(8, lo=None) == INV and sq(16, codes=_fake(17)) == INV and sq(8, d=13656) == UNS
    assert lvq(4, nq=-2) == INV and lvq(4, mu=None) == INV and lvq(4, k=300) == UNS and lvq(4, d=20484) == UNS
    assert sq(8, nq=0) == _native.MIVQ_OK and lvq(4, nq=0) == _native.MIVQ_OK


def test_rerank_workspace_follows_the_shape():
    """Partial top-k lists only: 4 waves x S slices of (nq, k) pairs, S growing with r while the
    batch is small and 1 for a large batch; 0 for sizes the entry points refuse."""
    from haag_vq import _native

    lib = _native.load_library()
    for fn in (lib.mivq_rerank_f32_workspace_bytes, lib.mivq_rerank_sq_workspace_bytes, lib.mivq_rerank_lvq_workspace_bytes):
        assert fn(1000, 250, 10) == 2 * 4 * 1000 * 10 * 4           # S = 1
        assert fn(3, 600, 10) == 2 * 256 * -(-(3 * 4 * 3 * 10 * 4) // 256)  # S = 3, rounded up to 256 B
        assert fn(70_000, 2, 1) == 2 * 4 * 70_000 * 4
        assert fn(0, 10, 10) == 0 and fn(5, 0, 10) == 0 and fn(5, 10, 0) == 0 and fn(5, 10, 257) == 0
