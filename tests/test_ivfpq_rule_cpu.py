"""CPU: the numpy rule of tests/_ivfpq_rule.py against the C oracle, on every constructed input the
GPU tests of tests/test_ivfpq_search_gpu.py use.  The two share no code, so a GPU result that
equals the rule bit for bit has been checked by two independent restatements of include/mivq.h."""

import numpy as np
import pytest

import _ivfpq_rule as R

NO_ID = R.NO_ID


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _ids(case):
    return "-".join(str(x) for x in case)


def test_cases_cover_the_issue():
    R.assert_cases_cover_the_issue()


def test_constructed_lists_are_what_the_cases_need():
    D = R.data_set("A", 8, 8)
    s = D["sizes"]
    assert D["n"] == 3000 and len(s) == 16
    assert (s[R.BIG], s[R.EMPTY], s[R.SMALL], s[R.L64], s[R.L65]) == (2500, 0, 20, 64, 65)
    assert 2500 == 39 * 64 + 4
    ids = D["ids"].astype(np.int64)
    assert len(np.unique(ids)) == 3000 and 250 <= (ids >= 1 << 31).sum() <= 350 and ids.max() < NO_ID
    assert (ids != np.arange(3000)).mean() > 0.99
    (a, b), (ta, tb) = D["dups"]
    off = D["offsets"]
    assert off[R.BIG] <= a < b < off[R.BIG + 1]
    assert off[R.TWIN_A] <= ta < off[R.TWIN_A + 1] and off[R.TWIN_B] <= tb < off[R.TWIN_B + 1]
    for x, y in D["dups"]:
        assert np.array_equal(D["codes"][x], D["codes"][y])
        for t in D["tau"].values():
            assert t[x] == t[y]
    for t in D["tau"].values():
        nan = np.nonzero(np.isnan(t))[0]
        assert nan.size == 1 and off[R.SMALL] <= nan[0] < off[R.SMALL + 1] and D["ids"][nan[0]] == D["nan_id"]
    PD = R.list_distances(D, "generic", 5, 0)
    assert np.array_equal(PD[:, R.TWIN_A], PD[:, R.TWIN_B])
    B = R.data_set("B", 8, 8)
    assert len(B["sizes"]) == 300 and B["sizes"].max() == 5 and B["sizes"].min() == 0 and 500 <= B["n"] <= 700
    # the "ties" kind: exact quarters, +inf and -inf on codes of one row, which sees both
    lut = R.make_lut(D, "ties", 4, 0)
    fin = lut[np.isfinite(lut)]
    assert np.array_equal(fin * 4, np.round(fin * 4)) and np.abs(fin).max() <= 2
    row = D["codes"][D["inf_row"]]
    assert lut[0, 0, row[0]] == np.inf and lut[0, 7, row[7]] == -np.inf and np.isfinite(lut[1]).all()


def test_probe_tables_hold_what_their_names_say():
    for case in R.CASES:
        name, M, nbits, metric, kind, k, nq, nprobe, probes = case
        I = R.case_inputs(case)
        P, D = I["probe_l"], I["D"]
        assert P.shape == (nq, nprobe) and I["probe_d"].shape == (nq, nprobe) and I["lut"].shape == (nq, M, 1 << nbits)
        real = P[P != NO_ID]
        assert (real < D["nlist"]).all()
        if probes == "skips":
            assert (P == NO_ID).any() and (P != NO_ID).any()
            if nq > 1:
                assert (P[nq // 2] == NO_ID).all()
            if nprobe > 16:
                assert (P[0, 3:] == NO_ID).all()
        if probes == "rand" and nprobe == 17 and name == "A":
            assert ((P == NO_ID).sum(1) == 1).all()
        if probes == "empty_alone":
            assert (R.rows_probed(D, P) == 0).all()
        if name == "A" and probes == "rand" and nprobe == 16:
            tw = np.take_along_axis(I["probe_d"], np.argsort(P, axis=1), 1)  # columns in list order
            assert np.array_equal(tw[:, R.TWIN_A], tw[:, R.TWIN_B])


@pytest.mark.parametrize("case", R.CASES, ids=_ids)
def test_rule_equals_the_oracle(oracle, case):
    I = R.case_inputs(case)
    D = I["D"]
    metric, k = case[3], case[5]
    rd, ri = R.case_expected(case)
    od, oi = oracle.ivfpq_search(I["lut"], I["probe_d"], I["probe_l"], D["offsets"], D["codes"], D["ids"], I["tau"],
                                 metric, k)
    np.testing.assert_array_equal(ri, oi)
    np.testing.assert_array_equal(_bits(rd), _bits(od))
    # what the constructed inputs must show in the reference itself
    rows = R.rows_probed(D, I["probe_l"])
    np.testing.assert_array_equal((ri != NO_ID).sum(1), np.minimum(k, rows))
    assert not np.isnan(rd).any() and np.isposinf(rd[ri == NO_ID]).all()
    if case[8] == "small_alone":
        assert ((ri[:, :20] != NO_ID).all() and (ri[:, 20:] == NO_ID).all())
        if metric == R.L2:
            assert (ri == D["nan_id"]).sum() == case[6] and np.isposinf(rd[ri == D["nan_id"]]).all()
    if case[4] == "ties" and case[0] == "A" and case[7] >= 5:
        # neighbours collide (the fewer sub-quantizers, the more): there the id decides, and ids
        # >= 2^31 are among the results
        same = (rd[:, 1:] == rd[:, :-1]) & (ri[:, 1:] != NO_ID)
        if k > 1:
            assert same.sum() >= 10
            assert (ri[:, 1:].astype(np.int64) > ri[:, :-1].astype(np.int64))[same].all()
        if k >= 64:
            assert ((ri >= 1 << 31) & (ri != NO_ID)).any()


def test_rule_equals_the_oracle_on_the_tiled_input(oracle):
    T = R.tiled_case()
    D = T["D"]
    rd, ri = R.search_rule(T["lut"], T["probe_d"], T["probe_l"], D["offsets"], D["codes"], D["ids"], T["tau"], R.L2,
                           T["k"])
    od, oi = oracle.ivfpq_search(T["lut"], T["probe_d"], T["probe_l"], D["offsets"], D["codes"], D["ids"], T["tau"],
                                 R.L2, T["k"])
    np.testing.assert_array_equal(ri, oi)
    np.testing.assert_array_equal(_bits(rd), _bits(od))
    assert (ri[4] == NO_ID).all() and (ri[5] == NO_ID).all() and (ri[0] != NO_ID).all()


def test_merge_cases_cover_the_issue():
    C = R.MERGE_CASES
    assert {c[0] for c in C} == {0, 1, 2, 3, 17, 256}
    assert {c[1] for c in C} == {1, 10, 64, 65, 256}
    assert {c[2] for c in C} == {1, 3, 4, 5, 130}
    assert {c[3] for c in C} == {"generic", "ties"}


@pytest.mark.parametrize("parts,k,nq,kind", R.MERGE_CASES)
def test_merge_inputs_hold_what_the_issue_lists(parts, k, nq, kind):
    dd, ii = R.merge_inputs(parts, k, nq, kind)
    assert dd.shape == ii.shape == (parts, nq, k) and dd.dtype == np.float32 and ii.dtype == np.uint32
    key = np.where(np.isnan(dd), np.inf, dd)
    i64 = ii.astype(np.int64)
    if k > 1:  # every list sorted by (dist, id)
        assert ((key[..., 1:] > key[..., :-1]) | ((key[..., 1:] == key[..., :-1]) & (i64[..., 1:] >= i64[..., :-1]))).all()
    assert np.isposinf(dd[ii == NO_ID]).all()
    if parts >= 17 and k >= 10:
        assert ((ii >= 1 << 31) & (ii != NO_ID)).any()
        assert (ii == NO_ID).all(axis=2).any()                                  # whole parts of padding
        assert ((ii[..., 0] != NO_ID) & (ii[..., -1] == NO_ID)).any()           # lists that end in padding
        assert np.isnan(dd).any()
        for a in range(nq):  # equal distances across parts under distinct ids
            real = ii[:, a, :] != NO_ID
            vals = [set(key[p, a][real[p]].tolist()) for p in range(parts)]
            seen = set()
            hit = False
            for v in vals:
                hit = hit or bool(seen & v)
                seen |= v
            assert hit
            ids_a = i64[:, a, :][real]
            assert len(np.unique(ids_a)) == ids_a.size
    if kind == "ties":
        fin = dd[np.isfinite(dd)]
        assert np.array_equal(fin * 4, np.round(fin * 4))


@pytest.mark.parametrize("parts,k,nq,kind", [c for c in R.MERGE_CASES if c[0] > 0])
def test_merge_rule_equals_topk_rows_of_the_concatenation(oracle, parts, k, nq, kind):
    """With the ids the column numbers of the (nq, parts * k) candidate matrix, the merge is
    oracle.topk_rows of that matrix."""
    dd, _ = R.merge_inputs(parts, k, nq, kind)
    cols = np.arange(parts * k, dtype=np.uint32).reshape(parts, 1, k).repeat(nq, axis=1)
    md, mi = R.merge_rule(dd, cols, k)
    flat = dd.transpose(1, 0, 2).reshape(nq, parts * k)
    od, oi = oracle.topk_rows(flat, k)
    np.testing.assert_array_equal(mi, oi)
    np.testing.assert_array_equal(_bits(md), _bits(od))


def test_merge_rule_of_no_parts_is_all_padding():
    md, mi = R.merge_rule(np.zeros((0, 3, 10), np.float32), np.zeros((0, 3, 10), np.uint32), 10)
    assert np.isposinf(md).all() and (mi == NO_ID).all() and md.shape == mi.shape == (3, 10)
