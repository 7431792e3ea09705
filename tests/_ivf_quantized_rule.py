"""IvfQuantizedIndex fixtures: the cases, their inputs, and a numpy restatement of the arithmetic.

Shared by the fixture generator (tests/golden/make_ivf_quantized_golden.py, which runs the
reference's IvfQuantizedIndex around the reference's ScalarQuantizer / LVQQuantizer) and by
tests/test_ivf_quantized_cpu.py / tests/test_ivf_quantized_gpu.py.  Everything here is numpy on
the host, composed with the oracle (handed in, as in _ivf_rabitq_rule.py); nothing of the
reference is imported.

For a row i of list l = assign[i] with centroid c = coarse[l], one float32 operation per step
(every intermediate is a float32 array), in the order include/mivq.h documents:

    residual : r = x - c
    SQ fit   : lo = min r, hi = max r over the list's rows, den = (hi - lo) + 1e-8;
               an empty list: lo = 0, den = 1e-8
    LVQ fit  : mu = (sum of r over the list's rows in ascending row order) / float32(count);
               an empty list: 0
    SQ row   : rint(((r - lo) / den) * L) as uint8 / uint16, 4 bits packed high nibble first,
               odd d zero-padded
    LVQ row  : _lvq_rule.encode(r, mu): the quantised value is (x - c) - mu
    x^       : oracle.sq_decode / _lvq_rule.decode of the row with the list's parameters, + c
    key      : the chains of oracle.flat_search on x^
    ranking  : ascending (key, id), id compared as uint32; padding (+inf, 0xFFFFFFFF)
"""

from __future__ import annotations

import hashlib

import numpy as np

import _lvq_rule as LR

F32 = np.float32
NO_ID = 0xFFFFFFFF
L2, IP = 1, 0  # MIVQ_METRIC_L2, MIVQ_METRIC_INNER_PRODUCT
METRIC_ID = {"l2": L2, "ip": IP}
METRICS = ("l2", "ip")

# name -> kind, bits, N, D; every case: K = 8 lists (one of them empty), nprobe 3, nq 9, k 10
CASES = {
    "sq8_d37": dict(kind="sq", bits=8, N=1500, D=37),
    "sq4_d128": dict(kind="sq", bits=4, N=2000, D=128),
    "sq16_d64": dict(kind="sq", bits=16, N=1200, D=64),
    "lvq4_d100": dict(kind="lvq", bits=4, N=1500, D=100),
    "lvq8_d128": dict(kind="lvq", bits=8, N=2000, D=128),
    "lvq3_d37": dict(kind="lvq", bits=3, N=1031, D=37),
}
K, NPROBE, NQ, TOPK = 8, 3, 9, 10
# a draw other than 0 replaces a case's seed [N, D, bits] by [N, D, bits, draw] (used when the
# reference's own result leaves more than OPEN_CAP of a case's positions open)
DRAWS = {}


def sha(a) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def seed_of(name: str):
    c = CASES[name]
    s = [c["N"], c["D"], c["bits"]]
    return s + [DRAWS[name]] if DRAWS.get(name) else s


def inputs(name: str):
    """(X, Q, coarse) float32 of a case from its seed.  Gaussian clusters: K - 1 centres
    N(0, 4) + 3 per dimension, per-dimension spread U(0.2, 1.5), rows dealt to the clusters at
    random; the queries are further draws from the same clusters.  coarse: K - 1 data rows, one
    per cluster, and a spare centroid at -10 in every dimension.  Every row's coordinates sum to
    about 3 D, so the spare is the farthest centroid under L2 and has the most negative inner
    product: it attracts nothing under either metric (the generator and the tests assert it)."""
    c = CASES[name]
    N, D = c["N"], c["D"]
    rng = np.random.default_rng(seed_of(name))
    centres = rng.standard_normal((K - 1, D)) * 2.0 + 3.0
    spread = rng.uniform(0.2, 1.5, D)
    member = rng.integers(0, K - 1, N)
    member[:K - 1] = np.arange(K - 1)  # every cluster has a row
    X = (centres[member] + rng.standard_normal((N, D)) * spread).astype(F32)
    qm = rng.integers(0, K - 1, NQ)
    Q = (centres[qm] + rng.standard_normal((NQ, D)) * spread).astype(F32)
    coarse = np.empty((K, D), F32)
    order = rng.permutation(K)  # where the spare sits differs from case to case
    for j in range(K - 1):
        coarse[order[j]] = X[j]
    coarse[order[K - 1]] = F32(-10.0)
    return X, Q, coarse


def scores64(X, C, metric: str) -> np.ndarray:
    """fp64 (n, K) coarse scores, smaller is nearer: squared L2, or the negated inner product.
    Summed dimension by dimension in a fixed order (no BLAS: the same bits on every CPU)."""
    X, C = np.asarray(X, np.float64), np.asarray(C, np.float64)
    out = np.zeros((X.shape[0], C.shape[0]))
    for t in range(X.shape[1]):
        if metric == "l2":
            out += (X[:, t, None] - C[None, :, t]) ** 2
        else:
            out -= X[:, t, None] * C[None, :, t]
    return out


def assign64(X, C, metric: str) -> np.ndarray:
    return np.argmin(scores64(X, C, metric), axis=1).astype(np.int64)


def probes64(Q, C, metric: str, nprobe: int) -> np.ndarray:
    """(nq, nprobe) nearest lists, nearest first (stable on ties)."""
    return np.argsort(scores64(Q, C, metric), axis=1, kind="stable")[:, :nprobe].astype(np.int64)


# ------------------------------------------------------------------------------ the restatement
def code_shape(kind: str, bits: int, D: int):
    """(elements per row, dtype) of a code row."""
    if kind == "lvq":
        return LR.code_size(D, bits), np.uint8
    return ((D + 1) // 2 if bits == 4 else D), (np.uint16 if bits == 16 else np.uint8)


def fit(X, coarse, assign, kind: str):
    """The per-list parameters as (K, D) float32 arrays: (lo, den) for SQ, (mu,) for LVQ."""
    X, coarse = np.ascontiguousarray(X, F32), np.ascontiguousarray(coarse, F32)
    nlist, D = coarse.shape
    if kind == "sq":
        lo, den = np.zeros((nlist, D), F32), np.full((nlist, D), F32(1e-8), F32)
    else:
        mu = np.zeros((nlist, D), F32)
    for l in range(nlist):
        rows = np.flatnonzero(assign == l)  # ascending row order
        if rows.size == 0:
            continue
        R = X[rows] - coarse[l]
        assert R.dtype == F32
        if kind == "sq":
            lo[l] = R.min(axis=0)
            hi = R.max(axis=0)
            den[l] = (hi - lo[l]) + F32(1e-8)
        else:
            mu[l] = LR.seq_mean(R)
    return (lo, den) if kind == "sq" else (mu,)


def sq_rows(R, lo, den, bits: int) -> np.ndarray:
    """The SQ code rows of residuals R with one list's (lo, den)."""
    L = F32((1 << bits) - 1)
    a = R - lo
    b = a / den
    c = b * L
    assert a.dtype == b.dtype == c.dtype == F32
    q = np.rint(c).astype(np.int64)  # in [0, L]: 0 <= r - lo <= hi - lo < den
    assert q.min() >= 0 and q.max() <= int(L)
    if bits == 16:
        return q.astype(np.uint16)
    q = q.astype(np.uint8)
    if bits == 8:
        return q
    if q.shape[1] % 2:
        q = np.pad(q, ((0, 0), (0, 1)))
    return ((q[:, 0::2] << 4) | q[:, 1::2]).astype(np.uint8)


def encode(X, coarse, assign, params, kind: str, bits: int) -> np.ndarray:
    """(N, row) code rows in row order."""
    X, coarse = np.ascontiguousarray(X, F32), np.ascontiguousarray(coarse, F32)
    width, dt = code_shape(kind, bits, X.shape[1])
    codes = np.zeros((X.shape[0], width), dt)
    for l in range(coarse.shape[0]):
        rows = np.flatnonzero(assign == l)
        if rows.size == 0:
            continue
        R = X[rows] - coarse[l]
        codes[rows] = sq_rows(R, params[0][l], params[1][l], bits) if kind == "sq" else LR.encode(R, params[0][l], bits)
    return codes


def decode(oracle, codes, coarse, assign, params, kind: str, bits: int) -> np.ndarray:
    """x^ (N, D) float32: the row's decode with its list's parameters, plus the centroid."""
    coarse = np.ascontiguousarray(coarse, F32)
    D = coarse.shape[1]
    assign = np.asarray(assign)
    out = np.zeros((codes.shape[0], D), F32)
    for l in range(coarse.shape[0]):
        rows = np.flatnonzero(assign == l)
        if rows.size == 0:
            continue
        if kind == "sq":
            dec = oracle.sq_decode(np.ascontiguousarray(codes[rows]), D, params[0][l], params[1][l], bits)
        else:
            dec = LR.decode(codes[rows], params[0][l], bits)
        assert dec.dtype == F32
        out[rows] = dec + coarse[l]
    return out


def probed_rows(offsets, list_ids, nlist: int, slots):
    """Bucket positions of the rows a query probes, in ascending uint32 id order.  Slots holding
    NO_ID or any id >= nlist are skipped."""
    ids = np.asarray(list_ids).astype(np.int64) & 0xFFFFFFFF
    pos = [np.arange(int(offsets[l]), int(offsets[l + 1]))
           for l in (int(s) & 0xFFFFFFFF for s in np.asarray(slots).ravel()) if l < nlist]
    pos = np.concatenate(pos) if pos else np.zeros(0, np.int64)
    return pos[np.argsort(ids[pos], kind="stable")]


def expected(oracle, list_codes, list_ids, offsets, coarse, params, kind, bits, Q, probe_l, metric: int, k: int,
             rec=None):
    """(dists f32 (nq, k), ids uint32 (nq, k)) for probe lists probe_l (nq, nprobe): per query,
    decode the probed lists, add their centroids, oracle.flat_search over those rows.  rec: the
    decode of list_codes (bucket order), when the caller has it already."""
    Q = np.ascontiguousarray(Q, F32)
    nq = Q.shape[0]
    nlist = coarse.shape[0]
    ids = np.asarray(list_ids).astype(np.int64) & 0xFFFFFFFF
    list_of = np.repeat(np.arange(nlist), np.diff(np.asarray(offsets)))
    if rec is None:
        rec = decode(oracle, list_codes, coarse, list_of, params, kind, bits)
    dd = np.full((nq, k), np.inf, F32)
    ii = np.full((nq, k), NO_ID, np.uint32)
    for a in range(nq):
        pos = probed_rows(offsets, list_ids, nlist, probe_l[a])
        if pos.size == 0:
            continue
        kk = min(k, pos.size)
        d1, i1 = oracle.flat_search(Q[a:a + 1], rec[pos], kk, metric)  # ties to the smaller position = id
        dd[a, :kk] = d1[0]
        ii[a, :kk] = ids[pos[i1[0].astype(np.int64)]].astype(np.uint32)
    return dd, ii


# ------------------------------------------------------------------------------ acceptance
def judges(Q, rec, offsets, list_ids, nlist, probe_l, metric: str, k: int):
    """One _search_rule.Judge per query over the rows it probes (rec in bucket order), with the
    probed rows' ids in ascending order: [(judge, ids of its rows)]."""
    from _search_rule import Judge

    ids = np.asarray(list_ids).astype(np.int64) & 0xFFFFFFFF
    out = []
    for a in range(len(Q)):
        pos = probed_rows(offsets, list_ids, nlist, probe_l[a])
        out.append((Judge(Q[a:a + 1], rec[pos], metric, k), ids[pos]))
    return out


def open_share(js) -> float:
    return float(np.mean([j.open.mean() for j, _ in js]))


def problems(js, ids, dists, metric: str, tie_order: bool):
    """The clauses of _search_rule a result (ids uint32 (nq, k), dists f32 (nq, k): ascending keys,
    IP as negated inner products) breaks, query by query.  Every query must probe >= k rows."""
    out = []
    for a, (j, rid) in enumerate(js):
        if j.k != ids.shape[1]:
            out.append(f"q{a}: probes {len(rid)} rows, fewer than k")
            continue
        loc = np.searchsorted(rid, ids[a].astype(np.int64))
        if (loc >= len(rid)).any() or (rid[np.minimum(loc, len(rid) - 1)] != ids[a]).any():
            out.append(f"q{a}: an id outside the probed lists")
            continue
        score = -dists[a] if metric == "ip" else dists[a]  # the Judge takes IP scores as +inner product
        # clause 5 (order) is checked on what the index returns: ascending keys
        if (np.diff(dists[a]) < 0).any():
            out.append(f"5: q{a} keys out of order")
        p = j.problems(loc.astype(np.uint32)[None, :], score.astype(F32)[None, :], tie_order)
        out += [f"q{a}: {s}" for s in p if not s.startswith("5:")]
    return out


# ------------------------------------------------------------------------------ fixture cases
def load_fixture(golden_dir) -> dict:
    with np.load(golden_dir / "ivf_quantized_golden.npz") as z:
        return {k: z[k] for k in z.files}


class Case:
    """One (case, metric) of the fixture: regenerated inputs, the fixture's assignment and probes,
    and the restatement's parameters, codes, lists and reconstruction (computed once)."""

    def __init__(self, oracle, name, metric, fx):
        self.name, self.metric, self.fx, self.c = name, metric, fx, CASES[name]
        self.kind, self.bits, self.N, self.D = self.c["kind"], self.c["bits"], self.c["N"], self.c["D"]
        self.X, self.Q, self.coarse = inputs(name)
        assert list(fx[f"{name}_seed"]) == seed_of(name)
        assert sha(self.X) == str(fx[f"{name}_X_sha"]), f"{name}: regenerated X differs from the fixture's"
        assert sha(self.Q) == str(fx[f"{name}_Q_sha"]), f"{name}: regenerated Q differs from the fixture's"
        assert sha(self.coarse) == str(fx[f"{name}_coarse_sha"]), f"{name}: regenerated centroids differ"
        key = f"{name}_{metric}"
        self.assign = fx[f"{key}_assign"].astype(np.int64)
        self.probe_l = fx[f"{key}_probes"].astype(np.int64)
        self.params = fit(self.X, self.coarse, self.assign, self.kind)
        self.codes = encode(self.X, self.coarse, self.assign, self.params, self.kind, self.bits)
        self.offsets, self.order = oracle.bucket_sort(self.assign, K)
        self.list_codes = np.ascontiguousarray(self.codes[self.order.astype(np.int64)])
        self.list_ids = self.order.astype(np.uint32)
        self.rec = decode(oracle, self.codes, self.coarse, self.assign, self.params, self.kind, self.bits)
        self.judges = judges(self.Q, self.rec[self.order.astype(np.int64)], self.offsets, self.list_ids, K,
                             self.probe_l, metric, TOPK)

    def ref(self):
        key = f"{self.name}_{self.metric}"
        return self.fx[f"{key}_ids"], self.fx[f"{key}_dists"]

    def expected(self, oracle):
        return expected(oracle, self.list_codes, self.list_ids, self.offsets, self.coarse, self.params, self.kind,
                        self.bits, self.Q, self.probe_l, METRIC_ID[self.metric], TOPK)
