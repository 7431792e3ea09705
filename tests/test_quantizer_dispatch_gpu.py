"""GPU: which kernel chain ranks which quantizer's codes, and what RefinedIndex hands to the re-rank.

``search_codes`` asks the quantizer (``BaseQuantizer.flat_keys``).  ``chain`` below is the type
ladder it had before, written with direct ``_native`` calls on parameters made by hand; the two
must agree bit for bit in distances and ids, for both metrics and with an id offset past 2^31.
The quantizers are put together from random state, not fitted: only the dispatch is under test.
"""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N, D, NQ, K = 257, 64, 3, 5
OFFSETS = (0, 2 ** 31 + 5)
CASES = ("pq8", "pq4", "opq8", "sq8_f32", "sq8_f64", "rabitq", "lvq4", "rankaware", "extrabitq")
RA_BITS = np.tile(np.array([8, 6, 5, 4, 4, 3, 2, 0], dtype=np.int64), 8)  # 4 bits a dimension on average
# quantizer_state's members (name, dtype, shape) before the state rules moved onto the classes
PQ_FORMAT = {
    "pq8": [("qtype", "<U2", ()), ("M", "int64", ()), ("B", "int64", ()), ("centroids", "float32", (4, 256, 16))],
    "pq4": [("qtype", "<U2", ()), ("M", "int64", ()), ("B", "int64", ()), ("centroids", "float32", (4, 16, 16))],
    "opq8": [("qtype", "<U3", ()), ("M", "int64", ()), ("B", "int64", ()), ("A", "float32", (64, 64)),
             ("centroids", "float32", (4, 256, 16))],
}


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(got, want):
    return torch.equal(_bits(got[0]), _bits(want[0])) and torch.equal(got[1], want[1])


class Case:
    """A quantizer of one kind over the rows X, its codes, and the hand-made parameters of ``chain``."""

    def __init__(self, dev, name):
        from haag_vq import _native
        from haag_vq.methods.extended_rabitq import ExtendedRaBitQuantizer
        from haag_vq.methods.lvq_quantization import LVQQuantizer
        from haag_vq.methods.optimized_product_quantization import OptimizedProductQuantizer
        from haag_vq.methods.product_quantization import ProductQuantizer
        from haag_vq.methods.rabit_quantization import RaBitQuantizer
        from haag_vq.methods.rank_aware_quantization import RankAwareQuantizer
        from haag_vq.methods.scalar_quantization import ScalarQuantizer

        g = np.random.default_rng([7, CASES.index(name)])
        self.name = name
        X = g.standard_normal((N, D)).astype(np.float32)
        self.Q = torch.from_numpy(g.standard_normal((NQ, D)).astype(np.float32)).to(dev)
        Xd = torch.from_numpy(X).to(dev)
        if name in ("pq8", "pq4", "opq8"):
            self.B = int(name[-1])
            C = g.standard_normal((4, 1 << self.B, D // 4)).astype(np.float32)
            self.C = torch.from_numpy(C).to(dev)
            if name == "opq8":
                A = np.linalg.qr(g.standard_normal((D, D)))[0].astype(np.float32)
                self.A = torch.from_numpy(A).to(dev)
                q = OptimizedProductQuantizer.from_state(dict(M=4, B=8, A=A, centroids=C))
            else:
                q = ProductQuantizer(M=4, B=self.B)
                q.set_codebooks(C)
        elif name in ("sq8_f32", "sq8_f64"):
            q = ScalarQuantizer(8)
            dt = np.float32 if name == "sq8_f32" else np.float64
            q.min, q.max = X.min(axis=0).astype(dt), X.max(axis=0).astype(dt)
            self.lo = torch.from_numpy(q.min).to(dev)
            self.den = torch.from_numpy(((q.max - q.min) + 1e-8).astype(dt)).to(dev)
        elif name == "rabitq":
            q = RaBitQuantizer()
            q.fit(X[:0])
        elif name == "lvq4":
            q = LVQQuantizer(4)
            q.mu = X.mean(axis=0)
            self.mu = torch.from_numpy(q.mu).to(dev)
        elif name == "rankaware":
            q = RankAwareQuantizer(4.0)
            q.mu = X.mean(axis=0).astype(np.float64)
            q.V = np.linalg.qr(g.standard_normal((D, D)))[0]
            q.var = np.sort(g.random(D) + 0.1)[::-1].copy()
            q.bits, q.D = RA_BITS.copy(), D
            q.cb = [np.sort(g.standard_normal(2 ** b)) * np.sqrt(v) for b, v in zip(q.bits, q.var)]
            q._levels = [np.sort(g.standard_normal(2 ** b)) for b in range(9)]
            q._Dg = g.random(9)
            q._layout()
        else:
            q = ExtendedRaBitQuantizer(num_bits=4)
            q.D, q.c = D, X.mean(axis=0).astype(np.float64)
            q.P = np.linalg.qr(g.standard_normal((D, D)))[0]
            q.levels = np.sort(g.standard_normal(16))
            self.state = tuple(torch.from_numpy(a).to(dev) for a in (q.c, q.P, q.levels))
        self.q = q
        self.codes = q.compress(Xd)
        assert self.codes.is_cuda and self.codes.shape[0] == N
        self._native = _native

    def decoded(self):
        """The f32 rows the decode path searches, by the decode kernel of the format."""
        nt = self._native
        if self.name == "sq8_f64":
            return nt.sq_decode(self.codes, D, self.lo, self.den, 8).to(torch.float32)
        if self.name == "lvq4":
            return nt.lvq_decode(self.codes, self.mu, 4)
        if self.name == "rankaware":
            return nt.rankaware_decode(self.codes, self.q._state())
        assert self.name == "extrabitq"
        return nt.extrabitq_decode(self.codes, *self.state, 4)

    def chain(self, k, mt, off):
        """(keys, ids) of the kernel chain this kind of quantizer is ranked by."""
        nt, Q = self._native, self.Q
        if self.name in ("pq8", "pq4", "opq8"):
            if self.name == "opq8":
                Q = nt.opq_rotate_prepared(Q, nt.opq_prepare(self.A, False))  # Q . A^T; D % 8 == 0
            u8 = self.codes if self.B == 8 else nt.pq_unpack(self.codes, 4, self.B)
            return nt.adc_search(nt.adc_lut(Q, self.C, self.B, mt), u8, k, self.B, id_offset=off)
        if self.name == "sq8_f32":
            return nt.sq_flat_search(Q, self.codes, D, self.lo, self.den, 8, k, mt, id_offset=off)
        if self.name == "rabitq":
            return nt.rabitq_flat_search(Q, self.codes, D, None, k, mt, id_offset=off)
        if self.name == "lvq4":
            return nt.lvq_flat_search(Q, self.codes, self.mu, 4, k, mt, id_offset=off)
        return nt.flat_search(Q, self.decoded(), k, mt, id_offset=off)  # f64-fitted SQ, rank-aware, Extended RaBitQ

    def expected(self, k, metric, off):
        d, i = self.chain(k, {"ip": 0, "l2": 1}[metric], off)  # mivq metric codes (include/mivq.h)
        return (-d if metric == "ip" else d), i


@pytest.fixture(scope="module")
def cases(dev):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Case(dev, name)
        return made[name]
    return get


@pytest.mark.parametrize("off", OFFSETS)
@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("name", CASES)
def test_search_codes_runs_the_chain_of_the_quantizer(cases, name, metric, off):
    from haag_vq.methods.search.flat_quantized_index import search_codes

    c = cases(name)
    got = search_codes(c.q, c.codes, c.Q, K, metric, off)
    assert got[0].shape == (NQ, K) and got[1].dtype == torch.int32
    assert _same(got, c.expected(K, metric, off))
    first = (got[1][:, 0].to(torch.int64) & 0xFFFFFFFF) - off
    assert bool(((first >= 0) & (first < N)).all())


@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("name", ["rankaware", "extrabitq"])
def test_rotated_indices_rank_by_the_quantizer_and_the_plain_index_does_not(cases, name, metric):
    """RankAwareFlatIndex / ExtendedRaBitQFlatIndex return ``q.search_codes`` bit for bit; a
    FlatQuantizedIndex over the same quantizer stays on decode + mivq_flat_search."""
    from haag_vq.methods.search import ExtendedRaBitQFlatIndex, FlatQuantizedIndex, RankAwareFlatIndex

    c = cases(name)
    Q = c.Q.cpu().numpy()
    out = {}
    for cls in (RankAwareFlatIndex if name == "rankaware" else ExtendedRaBitQFlatIndex, FlatQuantizedIndex):
        idx = cls(c.q)
        idx._codes, idx._metric, idx._N, idx._D = c.codes, metric, N, D
        out[cls] = idx.search_with_scores(Q, K)
    rot_d, rot_i = c.q.search_codes(c.codes, c.Q, K, metric)
    flat_d, flat_i = c.expected(K, metric, 0)
    (ids, dists), (fids, fdists) = out.values()
    assert np.array_equal(ids.view(np.int32), rot_i.cpu().numpy())
    assert np.array_equal(dists.view(np.int32), _bits(rot_d).cpu().numpy())
    assert np.array_equal(fids.view(np.int32), flat_i.cpu().numpy())
    assert np.array_equal(fdists.view(np.int32), _bits(flat_d).cpu().numpy())


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_large_k_decodes_sorts_and_offsets_the_ids(cases, metric):
    """k = 300 > 256 over 257 rows: every row, by a stable sort of the pairwise distances to the
    decoded rows, and ids + (2^31 + 5) as uint32 bit patterns."""
    from haag_vq import _native
    from haag_vq.methods.search.flat_quantized_index import search_codes

    c, off = cases("lvq4"), 2 ** 31 + 5
    d, i = search_codes(c.q, c.codes, c.Q, 300, metric, off)
    P = _native.pairwise_distances(c.Q, c.decoded(), {"ip": 0, "l2": 1}[metric])
    v, order = torch.sort(P, dim=1, stable=True)
    assert d.shape == (NQ, N) and i.dtype == torch.int32
    assert torch.equal(_bits(d), _bits(-v if metric == "ip" else v))
    assert torch.equal(i.to(torch.int64) & 0xFFFFFFFF, order + off)


@pytest.mark.parametrize("name", list(PQ_FORMAT))
def test_pq_state_keeps_its_format_and_searches_the_same(cases, name):
    from haag_vq.methods.search.flat_quantized_index import quantizer_from_state, quantizer_state, search_codes

    c = cases(name)
    st = quantizer_state(c.q)
    assert [(nm, str(np.asarray(v).dtype), np.asarray(v).shape) for nm, v in st.items()] == PQ_FORMAT[name]
    back = quantizer_from_state(st)
    assert type(back) is type(c.q)
    for metric in ("l2", "ip"):
        assert _same(search_codes(back, c.codes, c.Q, K, metric, 5), c.expected(K, metric, 5))
    assert torch.equal(back.decompress(c.codes), c.q.decompress(c.codes))


@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("kind", ["f32", "sq", "lvq"])
def test_refined_index_hands_the_code_parameters_to_the_rerank(dev, kind, metric):
    from haag_vq import _native
    from haag_vq.methods.lvq_quantization import LVQQuantizer
    from haag_vq.methods.scalar_quantization import ScalarQuantizer
    from haag_vq.methods.search import FlatQuantizedIndex, RefinedIndex

    g = np.random.default_rng(19)
    X = g.standard_normal((N, D)).astype(np.float32)
    Q = g.standard_normal((NQ, D)).astype(np.float32)
    Xd, Qd = torch.from_numpy(X).to(dev), torch.from_numpy(Q).to(dev)
    refine = {"f32": None, "sq": ScalarQuantizer(8), "lvq": LVQQuantizer(8)}[kind]
    idx = RefinedIndex(FlatQuantizedIndex(LVQQuantizer(4)), refine)
    idx.fit(X, metric)
    ids, dists = idx.search_with_scores(Q, K)
    if kind == "f32":
        store, params, bits = Xd, (), 0
    elif kind == "sq":
        lo, hi = X.min(axis=0), X.max(axis=0)
        params = (torch.from_numpy(lo).to(dev), torch.from_numpy(((hi - lo) + 1e-8).astype(np.float32)).to(dev))
        store, bits = _native.sq_encode(Xd, *params, 8), 8
    else:
        params = (_native.column_mean(Xd),)
        store, bits = _native.lvq_encode(Xd, params[0], 8), 8
    cand = idx.base.search(Q, idx.candidate_count(K))
    assert cand.shape == (NQ, 10 * K)
    d, i = _native.rerank(kind, Qd, torch.from_numpy(cand.view(np.int32)).to(dev), store, params, bits, K,
                          {"ip": 0, "l2": 1}[metric])
    assert np.array_equal(ids, i.cpu().numpy().view(np.uint32))
    assert np.array_equal(dists.view(np.int32), _bits(-d if metric == "ip" else d).cpu().numpy())


def test_indices_refuse_a_quantizer_without_a_code_kind():
    from haag_vq.methods.lvq_quantization import LVQQuantizer
    from haag_vq.methods.product_quantization import ProductQuantizer
    from haag_vq.methods.search import FlatQuantizedIndex, IvfQuantizedIndex, RefinedIndex

    with pytest.raises(ValueError) as e:
        RefinedIndex(FlatQuantizedIndex(LVQQuantizer(4)), ProductQuantizer(M=4))
    assert str(e.value) == ("RefinedIndex re-ranks on f32 rows (refine=None), ScalarQuantizer (4 / 8 / 16 bits) or "
                            "LVQQuantizer (1..8 bits) codes, got ProductQuantizer")
    with pytest.raises(NotImplementedError) as e:
        IvfQuantizedIndex(lambda: ProductQuantizer(M=4), K=4, nprobe=2)
    assert str(e.value) == ("IvfQuantizedIndex is native for ScalarQuantizer (4 / 8 / 16 bits) and LVQQuantizer "
                            "(1..8 bits); the factory returned ProductQuantizer")
