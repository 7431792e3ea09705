"""IvfListPqIndex: the cases, their inputs, and a numpy restatement of the arithmetic.

Shared by tests/test_ivf_listpq_cpu.py and tests/test_ivf_listpq_gpu.py.  Everything here is numpy
on the host, composed with the oracle (handed in, as in _ivf_quantized_rule.py).  The reference's
own index needs faiss, which is absent, so there is no reference-generated fixture: the semantics
are pinned to fp64 distances to the reconstruction through _search_rule.Judge (with M, the ADC
bound), the bits to the composition of the oracle's ADC.

For a row i of list l = assign[i] with centroid c = coarse[l] and the list's codebook cb[l]
(M, ksub, dsub), one float32 operation per step, in the order include/mivq.h documents:

    residual : r = x - c
    code row : oracle.pq_encode(r, cb[l]), one byte per sub-code
    e        : cb[l][m][j][t] + c[m*dsub + t]
    x^       : oracle.pq_decode(row, cb[l]) + c            (= the gather of e)
    table    : oracle.adc_lut(q, e, metric)
    key      : oracle.adc_search's sum over the row's codes
    ranking  : ascending (key, id), id compared as uint32; padding (+inf, 0xFFFFFFFF)

The per-list codebooks of the cases are seeded, not trained: 2^B rows of the list's residuals,
drawn with a per-list seed and split by subspace.
"""

from __future__ import annotations

import numpy as np

from _ivf_quantized_rule import IP, L2, METRIC_ID, METRICS, NO_ID, assign64, open_share, probes64, problems  # noqa: F401

F32 = np.float32

# name -> M, B, N, D; every case: K = 4 lists (one of them empty), nprobe 3, nq 9, k 10
CASES = {
    "m4_b8_d32": dict(M=4, B=8, N=4000, D=32),       # ~1333 rows per list: several row steps, row ranges under S
    "m64_b8_d64": dict(M=64, B=8, N=1300, D=64),     # dsub = 1
    "m8_b4_d40": dict(M=8, B=4, N=700, D=40),        # odd dsub = 5, 16-entry tables
    "m128_b8_d256": dict(M=128, B=8, N=1100, D=256),  # 128 KB of table per pair: chunks of subspaces
    "m2_b8_d200": dict(M=2, B=8, N=1000, D=200),     # dsub = 100; 333 rows on 256 centroids: exact key ties
}
K, NPROBE, NQ, TOPK = 4, 3, 9, 10
# a draw other than 0 replaces a case's seed [N, D, M, B] by [N, D, M, B, draw] (used when a
# case's open share exceeds _search_rule.OPEN_CAP)
DRAWS = {}


def seed_of(name: str):
    c = CASES[name]
    s = [c["N"], c["D"], c["M"], c["B"]]
    return s + [DRAWS[name]] if DRAWS.get(name) else s


def inputs(name: str):
    """(X, Q, coarse) float32 of a case from its seed: the construction of
    _ivf_quantized_rule.inputs with K = 4.  Gaussian clusters: K - 1 centres N(0, 4) + 3 per
    dimension, per-dimension spread U(0.2, 1.5), rows dealt evenly to the clusters (row i to
    cluster i mod (K - 1)); the queries are further draws from the same clusters.  coarse: K - 1
    data rows, one per cluster, and a spare centroid at -10 in every dimension, which attracts
    nothing under either metric (the tests assert it)."""
    c = CASES[name]
    N, D = c["N"], c["D"]
    rng = np.random.default_rng(seed_of(name))
    centres = rng.standard_normal((K - 1, D)) * 2.0 + 3.0
    spread = rng.uniform(0.2, 1.5, D)
    member = np.arange(N) % (K - 1)
    X = (centres[member] + rng.standard_normal((N, D)) * spread).astype(F32)
    qm = rng.integers(0, K - 1, NQ)
    Q = (centres[qm] + rng.standard_normal((NQ, D)) * spread).astype(F32)
    coarse = np.empty((K, D), F32)
    order = rng.permutation(K)  # where the spare sits differs from case to case
    for j in range(K - 1):
        coarse[order[j]] = X[j]
    coarse[order[K - 1]] = F32(-10.0)
    return X, Q, coarse


# ------------------------------------------------------------------------------ the restatement
def seeded_codebooks(X, coarse, assign, M: int, B: int, seed) -> np.ndarray:
    """(nlist, M, 2^B, dsub) float32: per non-empty list, 2^B of its residuals (drawn without
    replacement with the seed [*seed, l]) split by subspace; an empty list keeps zeros."""
    X, coarse = np.ascontiguousarray(X, F32), np.ascontiguousarray(coarse, F32)
    nlist, D = coarse.shape
    ksub, dsub = 1 << B, D // M
    cb = np.zeros((nlist, M, ksub, dsub), F32)
    for l in range(nlist):
        rows = np.flatnonzero(assign == l)
        if rows.size == 0:
            continue
        assert rows.size >= ksub, (l, rows.size)
        pick = np.sort(np.random.default_rng(list(seed) + [l]).permutation(rows.size)[:ksub])
        R = X[rows[pick]] - coarse[l]
        assert R.dtype == F32
        cb[l] = R.reshape(ksub, M, dsub).transpose(1, 0, 2)
    return cb


def encode(oracle, X, coarse, assign, cb) -> np.ndarray:
    """(N, M) uint8 code rows in row order."""
    X, coarse = np.ascontiguousarray(X, F32), np.ascontiguousarray(coarse, F32)
    codes = np.zeros((X.shape[0], cb.shape[1]), np.uint8)
    for l in range(coarse.shape[0]):
        rows = np.flatnonzero(assign == l)
        if rows.size:
            R = X[rows] - coarse[l]
            assert R.dtype == F32
            codes[rows] = oracle.pq_encode(R, cb[l])
    return codes


def shifted(cb_l, c) -> np.ndarray:
    """e (M, ksub, dsub) float32 = cb[l] + c, one add."""
    M, ksub, dsub = cb_l.shape
    e = cb_l + np.ascontiguousarray(c, F32).reshape(M, 1, dsub)
    assert e.dtype == F32
    return np.ascontiguousarray(e)


def decode(oracle, codes, coarse, assign, cb) -> np.ndarray:
    """x^ (n, D) float32: oracle.pq_decode with the list's codebook, plus the centroid."""
    coarse = np.ascontiguousarray(coarse, F32)
    assign = np.asarray(assign)
    out = np.zeros((codes.shape[0], coarse.shape[1]), F32)
    for l in range(coarse.shape[0]):
        rows = np.flatnonzero(assign == l)
        if rows.size:
            dec = oracle.pq_decode(np.ascontiguousarray(codes[rows]), cb[l])
            assert dec.dtype == F32
            out[rows] = dec + coarse[l]
    return out


def expected(oracle, list_codes, list_ids, offsets, coarse, cb, Q, probe_l, metric: int, k: int):
    """(dists f32 (nq, k), ids uint32 (nq, k)) for probe lists probe_l (nq, nprobe): per query and
    probed list, oracle.adc_lut on e = cb[l] + c and oracle.adc_search over the list's codes;
    the lists' results merged by (dist, id), id as uint32.  Slots holding NO_ID or any id >= nlist
    are skipped."""
    Q = np.ascontiguousarray(Q, F32)
    nq, nlist = Q.shape[0], coarse.shape[0]
    ids = np.asarray(list_ids).astype(np.int64) & 0xFFFFFFFF
    e = {}
    dd = np.full((nq, k), np.inf, F32)
    ii = np.full((nq, k), NO_ID, np.uint32)
    for a in range(nq):
        cd, ci = [], []
        for s in np.asarray(probe_l[a]).ravel():
            l = int(s) & 0xFFFFFFFF
            if l >= nlist:
                continue
            b, t = int(offsets[l]), int(offsets[l + 1])
            if t == b:
                continue
            if l not in e:
                # the list's rows in ascending uint32 id order: adc_search breaks ties by position
                o = np.argsort(ids[b:t], kind="stable")
                e[l] = (shifted(cb[l], coarse[l]), np.ascontiguousarray(list_codes[b:t][o]), ids[b:t][o])
            el, codes_l, ids_l = e[l]
            lut = oracle.adc_lut(Q[a:a + 1], el, metric)
            d1, i1 = oracle.adc_search(lut, codes_l, min(k, t - b))  # the list's k best by (key, id)
            cd.append(d1[0])
            ci.append(ids_l[i1[0].astype(np.int64)])
        if not cd:
            continue
        cd, ci = np.concatenate(cd), np.concatenate(ci)
        o = np.lexsort((ci, cd))[:k]  # NaN keys came back as +inf
        dd[a, :o.size] = cd[o]
        ii[a, :o.size] = ci[o].astype(np.uint32)
    return dd, ii


def judges(Q, rec, offsets, list_ids, nlist, probe_l, metric: str, k: int, M: int):
    """One _search_rule.Judge (ADC bound: M) per query over the rows it probes (rec in bucket
    order), with the probed rows' ids in ascending order: [(judge, ids of its rows)]."""
    from _ivf_quantized_rule import probed_rows
    from _search_rule import Judge

    ids = np.asarray(list_ids).astype(np.int64) & 0xFFFFFFFF
    out = []
    for a in range(len(Q)):
        pos = probed_rows(offsets, list_ids, nlist, probe_l[a])
        out.append((Judge(Q[a:a + 1], rec[pos], metric, k, M=M), ids[pos]))
    return out


class Case:
    """One (case, metric): inputs, the fp64 assignment and probes, seeded codebooks, and the
    restatement's codes, lists and reconstruction (computed once)."""

    def __init__(self, oracle, name, metric):
        self.name, self.metric, self.c = name, metric, CASES[name]
        self.M, self.B, self.N, self.D = self.c["M"], self.c["B"], self.c["N"], self.c["D"]
        self.X, self.Q, self.coarse = inputs(name)
        self.assign = assign64(self.X, self.coarse, metric)
        self.probe_l = probes64(self.Q, self.coarse, metric, NPROBE)
        self.cb = seeded_codebooks(self.X, self.coarse, self.assign, self.M, self.B, seed_of(name))
        self.codes = encode(oracle, self.X, self.coarse, self.assign, self.cb)
        self.offsets, self.order = oracle.bucket_sort(self.assign, K)
        o = self.order.astype(np.int64)
        self.list_codes = np.ascontiguousarray(self.codes[o])
        self.list_ids = self.order.astype(np.uint32)
        self.list_of = self.assign[o]
        self.rec = decode(oracle, self.codes, self.coarse, self.assign, self.cb)
        self.judges = judges(self.Q, self.rec[o], self.offsets, self.list_ids, K, self.probe_l, metric, TOPK, self.M)

    def expected(self, oracle, probe_l=None, k=TOPK, list_ids=None):
        return expected(oracle, self.list_codes, self.list_ids if list_ids is None else list_ids, self.offsets,
                        self.coarse, self.cb, self.Q, self.probe_l if probe_l is None else probe_l,
                        METRIC_ID[self.metric], k)
