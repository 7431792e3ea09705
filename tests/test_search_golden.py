"""Search results of FlatQuantizedIndex / search_codes against the reference's own search.

tests/golden/search_golden.npz (make_golden.py `search`) holds what the reference's
FlatQuantizedIndex (search/flat_quantized_index.py:34-76: decode, scipy cdist or Q @ X_hat^T,
argpartition, argsort) returned for SQ-4/8/16, Extended RaBitQ and fixed PQ / OPQ tables, L2 and
IP.  A result is judged by the rule of tests/_search_rule.py: in fp64, from the oracle's decode
of the reference's codes, it separates the positions every correct fp32 search must fill with
the same row ("settled") from the near-ties ("open", at most 10 % per case, stored with the
fixture) and accepts only results that agree with the fp64 order exactly at the former and
within the fp32 error bound at the latter.

CPU tests: the inputs and codes regenerate to the stored digests, the reference's result passes
the rule, the oracle's search (flat_search over its decode, adc_lut + adc_search) passes it, and
the rule rejects six deliberately wrong results.  `-m gpu` tests: the classes on the device pass
the rule, equal the oracle's pipeline bit for bit, keep id order in planted ties, clamp k, and
add id_offset modulo 2^32 on both the kernel (k <= 256) and the large-k path.
"""

import numpy as np
import pytest
import torch

import _search_rule as R

MT = {"l2": 1, "ip": 0}  # mivq metric codes (include/mivq.h), as oracle.py takes them
PQ_KINDS = ("pq", "opq")
ALL = [(n, m) for n in R.CASES for m in R.METRICS]


@pytest.fixture(scope="module")
def sg(golden_dir):
    with np.load(golden_dir / "search_golden.npz") as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def erq(golden_dir):
    with np.load(golden_dir / "extrabitq_golden.npz") as z:
        return {k: z[k] for k in z.files}


class Case:
    """One fixture case: inputs, the reference's codes (reproduced and checked against their
    digest), the oracle's decode of them, and the judges per metric (built once, shared)."""

    def __init__(self, name, O, sg, erq):
        self.name, self.c, self.O, self.sg = name, R.CASES[name], O, sg
        c = self.c
        self.kind, self.N, self.D, self.k = c["kind"], c["N"], c["D"], c["k"]
        self.X, self.Q = R.inputs(name, erq["X"])
        assert int(sg[f"{name}_seed"]) == c["seed"]
        assert R.sha(self.X) == str(sg[f"{name}_X_sha"]), f"{name}: regenerated X differs from the fixture's"
        assert R.sha(self.Q) == str(sg[f"{name}_Q_sha"]), f"{name}: regenerated Q differs from the fixture's"
        self.M, self.A, self.C, self.yh = 0, None, None, None
        if self.kind == "sq":
            self.lo, self.hi = sg[f"{name}_lo"], sg[f"{name}_hi"]
            np.testing.assert_array_equal(self.lo, self.X.min(axis=0))
            np.testing.assert_array_equal(self.hi, self.X.max(axis=0))
            self.den = (self.hi - self.lo) + 1e-8
            self.codes = O.sq_encode(self.X, self.lo, self.den, c["bits"])
            self.xh = O.sq_decode(self.codes, self.D, self.lo, self.den, c["bits"])
        elif self.kind == "erq":
            t = f"b{c['bits']}"
            self.state = (erq[f"{t}_c"], erq[f"{t}_P"], erq[f"{t}_levels"])
            self.codes = erq[f"{t}_codes"]
            np.testing.assert_array_equal(O.extrabitq_encode(self.X, *self.state, c["bits"]), self.codes)
            self.xh = O.extrabitq_decode(self.codes, *self.state, c["bits"])
        else:
            self.M = c["M"]
            self.C = R.table_centroids(name)
            assert R.sha(self.C) == str(sg[f"{name}_centroids_sha"])
            self.A = sg[f"{name}_A"] if self.kind == "opq" else None
            self.codes = R.table_compress(self.X, self.C, self.A)  # (N, M) one byte per sub-code
            self.yh = O.pq_decode(self.codes, self.C)
            self.xh = self.yh if self.A is None else R.matmul_seq(self.yh, self.A).astype(np.float32)
        assert R.sha(self.codes) == str(sg[f"{name}_codes_sha"]), f"{name}: codes differ from the reference's"
        assert self.xh.dtype == np.float32
        self._judges = {}

    def judge(self, metric) -> R.Judge:
        if metric not in self._judges:
            opq = (self.yh, self.A) if self.kind == "opq" else None
            self._judges[metric] = R.Judge(self.Q, self.xh, metric, self.k, M=self.M, opq=opq)
        return self._judges[metric]

    def ref(self, metric):
        return self.sg[f"{self.name}_{metric}_ids"], self.sg[f"{self.name}_{metric}_dists"]

    # the oracle's pipelines, returned as the classes return them (IP as +inner product)
    def oracle_flat(self, metric, xh=None, k=None, id_offset=0):
        k = min(self.k if k is None else k, self.N)
        d, i = self.O.flat_search(self.Q, self.xh if xh is None else xh, k, MT[metric], id_offset)
        return i, (-d if metric == "ip" else d)

    def rotated_queries(self):
        """fp32 Q . A^T on the host: within the rotation bound of the rule (64 terms of fp32)."""
        return self.Q if self.A is None else (self.Q @ self.A.T).astype(np.float32)

    def oracle_adc(self, metric, Q=None, codes=None, k=None, id_offset=0):
        k = min(self.k if k is None else k, self.N)
        lut = self.O.adc_lut(self.rotated_queries() if Q is None else Q, self.C, MT[metric])
        d, i = self.O.adc_search(lut, self.codes if codes is None else codes, k, id_offset)
        return i, (-d if metric == "ip" else d)

    def oracle_pipeline(self, metric, **kw):
        """What search_codes computes for this kind of quantizer (k <= 256)."""
        return self.oracle_adc(metric, **kw) if self.kind in PQ_KINDS else self.oracle_flat(metric, **kw)


@pytest.fixture(scope="module")
def cases(oracle, sg, erq):
    made = {}

    def get(name) -> Case:
        if name not in made:
            made[name] = Case(name, oracle, sg, erq)
        return made[name]

    return get


def _report(tag, judge, ids, dists):
    print(f"\n[search-golden] {tag}: open share {judge.open_share:.4f}, "
          f"max |dist - key| / e {judge.ratio(ids, dists):.4f}")


# ------------------------------------------------------------------------------ CPU
def test_fixture_lists_every_case(sg):
    assert list(map(str, sg["cases"])) == list(R.CASES)
    for v in sg.values():
        assert v.dtype.kind in "iufbU", v.dtype  # plain arrays: numbers, masks, digests


@pytest.mark.parametrize("name", list(R.CASES))
def test_inputs_and_codes_regenerate(cases, name):
    """X, Q (and the PQ tables) regenerate to the stored digests; the oracle's SQ / Extended
    RaBitQ encode and the table quantizer reproduce the reference's codes."""
    cases(name)  # the constructor asserts all of it


@pytest.mark.parametrize("name,metric", ALL)
def test_reference_result_passes_the_rule(cases, name, metric):
    cs = cases(name)
    j = cs.judge(metric)
    ids, dists = cs.ref(metric)
    _report(f"reference {name} {metric}", j, ids, dists)
    np.testing.assert_array_equal(j.open, cs.sg[f"{name}_{metric}_open"])  # derived here = stored
    assert j.open_share <= R.OPEN_CAP
    j.check(ids, dists, f"reference {name} {metric}")
    want = np.stack(j.order).astype(np.uint32)
    np.testing.assert_array_equal(ids[~j.open], want[~j.open])
    assert ids.shape == (cs.c["nq"], min(cs.k, cs.N))


@pytest.mark.parametrize("name,metric", ALL)
def test_oracle_flat_search_passes_the_rule(cases, name, metric):
    """oracle.flat_search over the oracle's decode (for PQ / OPQ: pq_decode, rotated back)."""
    cs = cases(name)
    ids, dists = cs.oracle_flat(metric)
    _report(f"oracle flat {name} {metric}", cs.judge(metric), ids, dists)
    cs.judge(metric).check(ids, dists, f"oracle flat_search {name} {metric}")


@pytest.mark.parametrize("name,metric", [(n, m) for n, m in ALL if R.CASES[n]["kind"] in PQ_KINDS])
def test_oracle_adc_passes_the_rule(cases, name, metric):
    """oracle.adc_lut + oracle.adc_search on the byte codes (OPQ: on the rotated queries)."""
    cs = cases(name)
    ids, dists = cs.oracle_adc(metric)
    _report(f"oracle adc {name} {metric}", cs.judge(metric), ids, dists)
    cs.judge(metric).check(ids, dists, f"oracle adc {name} {metric}")


def _ties_db():
    """SQ-8 database 512 x 32 with rows 5, 17 and 509 identical; query 0 is that row."""
    rng = np.random.default_rng(77)
    X = rng.standard_normal((512, 32)).astype(np.float32)
    X[17] = X[5]
    X[509] = X[5]
    Q = np.concatenate([X[5:6], rng.standard_normal((3, 32)).astype(np.float32)])
    return X, Q


def _ties_oracle(O, metric, k):
    X, Q = _ties_db()
    lo, hi = X.min(axis=0), X.max(axis=0)
    den = (hi - lo) + 1e-8
    xh = O.sq_decode(O.sq_encode(X, lo, den, 8), 32, lo, den, 8)
    d, i = O.flat_search(Q, xh, k, MT[metric])
    return X, Q, xh, i, (-d if metric == "ip" else d)


def test_the_rule_rejects_wrong_results(cases, oracle):
    """Each of these is a result a plausible bug would produce; the unspoilt version of each is
    accepted by the tests above (and, for the ties, just below)."""
    sq = cases("sq8_d128")
    for metric in R.METRICS:
        ids, dists = sq.oracle_flat(metric)
        assert not sq.judge(metric).problems(ids, dists)
        # ids shifted by one
        assert sq.judge(metric).problems(((ids + 1) % sq.N).astype(np.uint32), dists), metric
        # SQ decode without "+ lo"
        bad = sq.oracle_flat(metric, xh=(sq.xh - sq.lo).astype(np.float32))
        assert sq.judge(metric).problems(*bad), metric
    # IP scores returned negated (the search kernels rank -q.x ascending; the class flips the sign)
    ids, dists = sq.oracle_flat("ip")
    assert sq.judge("ip").problems(ids, (-dists).astype(np.float32))
    for metric in R.METRICS:
        # OPQ query left unrotated
        opq = cases("opq_M8_b8")
        assert not opq.judge(metric).problems(*opq.oracle_adc(metric))
        assert opq.judge(metric).problems(*opq.oracle_adc(metric, Q=opq.Q)), metric
        # B = 4 codes searched without unpacking: the packed bytes taken for sub-codes
        p4 = cases("pq_M16_b4")
        packed = oracle.pq_pack(p4.codes, 4)
        assert packed.shape == (p4.N, 8)
        np.testing.assert_array_equal(oracle.pq_unpack(packed, 16, 4), p4.codes)
        as_codes = np.concatenate([packed, packed], axis=1) & 15  # kept inside the 16-entry tables
        assert p4.judge(metric).problems(*p4.oracle_adc(metric, codes=as_codes)), metric
        # two equal-distance rows swapped out of id order
        X, Q, xh, ids, dists = _ties_oracle(oracle, metric, 10)
        j = R.Judge(Q, xh, metric, 10)
        assert not j.problems(ids, dists)
        if metric == "l2":
            assert list(ids[0, :3]) == [5, 17, 509] and dists[0, 0] == dists[0, 2]
            swapped = ids.copy()
            swapped[0, [0, 1]] = ids[0, [1, 0]]
            assert any(p.startswith("7") for p in j.problems(swapped, dists))
    # wrong dtype / unclamped shape
    tiny = cases("sq8_tiny")
    ids, dists = tiny.oracle_flat("l2")
    assert ids.shape == (3, 7) and not tiny.judge("l2").problems(ids, dists)
    assert tiny.judge("l2").problems(ids.astype(np.int64), dists)
    assert tiny.judge("l2").problems(np.pad(ids, ((0, 0), (0, 3))), np.pad(dists, ((0, 0), (0, 3))))


# ------------------------------------------------------------------------------ GPU
def _t(a, dev):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(dev)


def _model(cs: Case, dev):
    """The repo's quantizer of a case with the fixture's state, and the codes search_codes takes."""
    from haag_vq.methods.extended_rabitq import ExtendedRaBitQuantizer
    from haag_vq.methods.optimized_product_quantization import OPQHandle, OptimizedProductQuantizer
    from haag_vq.methods.product_quantization import ProductQuantizer
    from haag_vq.methods.scalar_quantization import ScalarQuantizer

    if cs.kind == "sq":
        q = ScalarQuantizer(num_bits=cs.c["bits"])
        q.min, q.max = cs.lo.copy(), cs.hi.copy()
        return q, _t(cs.codes, dev)
    if cs.kind == "erq":
        q = ExtendedRaBitQuantizer(num_bits=cs.c["bits"], seed=0)
        q.c, q.P, q.levels = cs.state
        q.D = cs.D
        return q, _t(cs.codes, dev)
    B = cs.c["B"]
    inner = ProductQuantizer(M=cs.M, B=B)
    inner.set_codebooks(cs.C)
    codes = _t(cs.codes if B == 8 else cs.O.pq_pack(cs.codes, B), dev)  # faiss' bit stream
    if cs.kind == "pq":
        return inner, codes
    q = OptimizedProductQuantizer(M=cs.M, B=B)  # as quantizer_from_state builds it
    q.opq = OPQHandle(_t(cs.A, dev))
    q._inner = inner
    q.pq = inner.pq
    return q, codes


def _search_codes(model, codes, Q, k, metric, id_offset=0):
    from haag_vq.methods.search.flat_quantized_index import ids_to_numpy, search_codes

    d, i = search_codes(model, codes, Q, k, metric, id_offset=id_offset)
    return ids_to_numpy(i), d.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("name,metric", [(n, m) for n, m in ALL if R.CASES[n]["kind"] == "sq"])
def test_sq_index_end_to_end(dev, cases, name, metric):
    """FlatQuantizedIndex(ScalarQuantizer).fit + search_with_scores on the device: the codes are
    the reference's, the result passes the rule and equals the oracle's pipeline bit for bit
    (k = 300 through _search_large_k, N = 7 through the clamp)."""
    from haag_vq.methods.scalar_quantization import ScalarQuantizer
    from haag_vq.methods.search import flat_quantized_index as fqi

    cs = cases(name)
    idx = fqi.FlatQuantizedIndex(ScalarQuantizer(num_bits=cs.c["bits"]))
    idx.fit(cs.X, metric)
    np.testing.assert_array_equal(idx.quantizer.min, cs.lo)
    np.testing.assert_array_equal(idx.quantizer.max, cs.hi)
    assert R.sha(idx._codes.cpu().numpy()) == str(cs.sg[f"{name}_codes_sha"])
    if name == "sq4_d37_k300":
        assert cs.k > fqi.MAX_KERNEL_K
    ids, dists = idx.search_with_scores(cs.Q, cs.k)
    j = cs.judge(metric)
    _report(f"device {name} {metric}", j, ids, dists)
    assert ids.shape == (cs.c["nq"], min(cs.k, cs.N))
    j.check(ids, dists, f"device {name} {metric}")
    oi, od = cs.oracle_flat(metric)
    np.testing.assert_array_equal(ids, oi)
    np.testing.assert_array_equal(dists, od)
    e_ids, e_d = idx.search_with_scores(cs.Q, 0)
    assert e_ids.shape == e_d.shape == (cs.c["nq"], 0) and e_ids.dtype == np.uint32 and e_d.dtype == np.float32
    assert np.array_equal(idx.search(cs.Q, cs.k), ids)


@pytest.mark.gpu
@pytest.mark.parametrize("name,metric", [(n, m) for n, m in ALL if R.CASES[n]["kind"] != "sq"])
def test_search_codes_on_fixture_codes(dev, cases, name, metric):
    """search_codes over the reference's codes with the fixture's model state: Extended RaBitQ
    (decode -> mivq_flat_search), PQ (ADC; B = 4 through pq_unpack), OPQ (rotated queries).
    Passes the rule; equals the oracle's pipeline bit for bit (OPQ exempt: its rotated query
    differs from the host's within the rotation bound)."""
    cs = cases(name)
    model, codes = _model(cs, dev)
    ids, dists = _search_codes(model, codes, cs.Q, cs.k, metric)
    j = cs.judge(metric)
    _report(f"device {name} {metric}", j, ids, dists)
    j.check(ids, dists, f"device {name} {metric}")
    if cs.kind != "opq":
        oi, od = cs.oracle_pipeline(metric)
        np.testing.assert_array_equal(ids, oi)
        np.testing.assert_array_equal(dists, od)


@pytest.mark.gpu
@pytest.mark.parametrize("metric", R.METRICS)
def test_rabitq1_search_codes_equals_oracle(dev, oracle, metric):
    """1-bit RaBitQ has no reference without faiss: search_codes(RaBitQuantizer) at n = 1031,
    d = 520 equals oracle.rabitq_decode + oracle.flat_search bit for bit."""
    from haag_vq.methods.rabit_quantization import RaBitQuantizer
    from haag_vq.utils.faiss_utils import MetricType

    n, d, nq, k = 1031, 520, 9, 10
    rng = np.random.default_rng(13)
    X = rng.standard_normal((n, d)).astype(np.float32)
    Q = rng.standard_normal((nq, d)).astype(np.float32)
    mtype = MetricType.L2 if metric == "l2" else MetricType.INNER_PRODUCT
    codes = oracle.rabitq_encode(X, None, int(mtype))
    model = RaBitQuantizer(metric_type=mtype)
    model.fit(X)
    ids, dists = _search_codes(model, _t(codes, dev), Q, k, metric)
    od, oi = oracle.flat_search(Q, oracle.rabitq_decode(codes, d), k, MT[metric])
    np.testing.assert_array_equal(ids, oi)
    np.testing.assert_array_equal(dists, -od if metric == "ip" else od)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [10, 300])
@pytest.mark.parametrize("metric", R.METRICS)
def test_planted_ties_keep_id_order(dev, oracle, metric, k):
    """Rows 5, 17 and 509 are identical and the query is that row: the three come first (L2) in
    ascending id order, and the whole result equals the oracle's, on the kernel path and on
    the large-k path."""
    from haag_vq.methods.scalar_quantization import ScalarQuantizer
    from haag_vq.methods.search.flat_quantized_index import FlatQuantizedIndex

    X, Q, xh, oi, od = _ties_oracle(oracle, metric, k)
    idx = FlatQuantizedIndex(ScalarQuantizer(num_bits=8))
    idx.fit(X, metric)
    ids, dists = idx.search_with_scores(Q, k)
    if metric == "l2":
        assert list(ids[0, :3]) == [5, 17, 509]
    pos = [int(np.flatnonzero(ids[0] == r)[0]) for r in (5, 17, 509)]
    assert pos[1] == pos[0] + 1 and pos[2] == pos[0] + 2  # adjacent, ascending ids
    assert dists[0, pos[0]] == dists[0, pos[2]]
    R.Judge(Q, xh, metric, k).check(ids, dists, f"ties {metric} k={k}")
    np.testing.assert_array_equal(ids, oi)
    np.testing.assert_array_equal(dists, od)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [10, 300])
@pytest.mark.parametrize("name", ["sq8_d128", "pq_M8_b8"])
def test_id_offset_is_added_modulo_2_32(dev, cases, name, k):
    """search_codes(..., id_offset=o) returns (ids_0 + o) mod 2^32 with the distances unchanged,
    up to the last offset that keeps every id below the 0xFFFFFFFF sentinel."""
    cs = cases(name)
    model, codes = _model(cs, dev)
    ids0, d0 = _search_codes(model, codes, cs.Q, k, "l2")
    assert ids0.shape == (cs.c["nq"], k) and int(ids0.max()) < cs.N
    for o in (1, 2 ** 31 - 5, 2 ** 32 - cs.N - 1):
        ids, d = _search_codes(model, codes, cs.Q, k, "l2", id_offset=o)
        want = ((ids0.astype(np.int64) + o) % 2 ** 32).astype(np.uint32)
        np.testing.assert_array_equal(ids, want, err_msg=f"offset {o}")
        np.testing.assert_array_equal(d, d0, err_msg=f"offset {o}")
