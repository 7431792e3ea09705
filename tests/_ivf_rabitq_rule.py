"""What mivq_ivf_rabitq_search must return, composed from existing oracle calls (numpy + oracle).

The key of (query a, row i of list l) is ``oracle.rabitq_est`` on that one code row with
``centroid = coarse[l]``; a query's result is the k smallest (key, id) pairs over the lists it
probes, ascending, ties to the smaller id, NaN keys ranked as +inf, padded with
(+inf, 0xFFFFFFFF).  The list codes are handed in (the tests pass the GPU-encoded rows, as
test_rabitq_search_bit_exact does, so the 1e-5 latitude of the encode's factors does not leak
into the search comparison).
"""

import numpy as np

NO_ID = 0xFFFFFFFF


def assign_rows(oracle, X, coarse, metric):
    """Nearest coarse centroid per row: oracle.topk_rows(oracle.pairwise(...), 1)."""
    return oracle.topk_rows(oracle.pairwise(X, coarse, metric), 1)[1][:, 0].astype(np.int64)


def bucket_order(oracle, assign, nlist):
    """(offsets (nlist + 1) int64, order): the rows of each list in ascending row order."""
    return oracle.bucket_sort(assign, nlist)


def expected(oracle, list_codes, list_ids, offsets, coarse, Q, probe_l, qb, metric, k):
    """(dists f32 (nq, k), ids uint32 (nq, k)) for probe lists probe_l (nq, nprobe), NO_ID = skip."""
    Q = np.ascontiguousarray(Q, np.float32)
    nq, d = Q.shape
    nlist = coarse.shape[0]
    probe_l = np.asarray(probe_l).astype(np.int64) & 0xFFFFFFFF
    keys = [[] for _ in range(nq)]
    ids = [[] for _ in range(nq)]
    for l in range(nlist):
        beg, end = int(offsets[l]), int(offsets[l + 1])
        who = np.nonzero((probe_l == l).any(axis=1))[0]
        if end == beg or who.size == 0:
            continue
        est = oracle.rabitq_est(list_codes[beg:end], d, Q[who], coarse[l], qb, metric)
        for row, a in zip(est, who):
            keys[a].append(row)
            ids[a].append(np.asarray(list_ids[beg:end]).astype(np.int64) & 0xFFFFFFFF)
    dd = np.full((nq, k), np.inf, np.float32)
    ii = np.full((nq, k), NO_ID, np.uint32)
    for a in range(nq):
        if not keys[a]:
            continue
        ka = np.concatenate(keys[a]).astype(np.float32)
        ia = np.concatenate(ids[a])
        ka = np.where(np.isnan(ka), np.float32(np.inf), ka)
        order = np.lexsort((ia, ka))[:k]
        dd[a, :order.size] = ka[order]
        ii[a, :order.size] = ia[order].astype(np.uint32)
    return dd, ii
