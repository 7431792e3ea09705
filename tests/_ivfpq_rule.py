"""What mivq_ivfpq_search and mivq_topk_merge must return, restated from include/mivq.h in plain
numpy, and the constructed inputs the CPU and GPU tests share.

The rule (float32 throughout, every operation one IEEE single operation):

    S    = ((0 + lut[q, 0, c_0]) + lut[q, 1, c_1]) + ... + lut[q, M-1, c_{M-1}]
    L2:    dist = (probe_d + tau) + 2 * S          IP:  dist = probe_d + S
    NaN -> +inf; a query's result is the k smallest (dist, id) over the rows of the lists it probes,
    ids compared as unsigned 32-bit; 0xFFFFFFFF probe slots are skipped; missing slots hold
    (+inf, 0xFFFFFFFF).

It is vectorised over the rows a query probes and shares no code with oracle/mivq_oracle.c, whose
oracle_ivfpq_search is a scalar loop with an insertion list: tests/test_ivfpq_rule_cpu.py pins
the two to each other on every input below, so the GPU comparison has two independent referees.

Inputs (no training, no encode; every array is made here):
  set A  16 lists, 3,000 rows: BIG 2,500 (39 steps of 64 rows + 4), EMPTY, SMALL 20, one list of
         64 rows, one of 65, eleven lists sharing 351; ids a permutation unrelated to position
         with a tenth of them in [2^31, 0xFFFFFFFE]; duplicate code rows with equal tau inside
         BIG; duplicate code rows with equal tau in lists TWIN_A and TWIN_B, which always get
         equal probe_d (equal distances in different waves); one row of SMALL with tau = NaN.
  set B  300 lists of 0..5 rows (about 600 rows), for nprobe up to 256 with distinct lists.
  LUT kinds  "generic": Gaussian LUT, probe_d, tau.  "ties": all three are multiples of 0.25 in
         [-2, 2], so every sum is exact, most distances collide and the id decides; every
         even query also has one +inf and one -inf LUT entry on codes of one row of BIG (with
         M >= 2 that row and others see both: NaN -> +inf with the row's own id).
"""

import numpy as np

NO_ID = 0xFFFFFFFF
L2, IP = 1, 0
NLIST_A = 16
BIG, EMPTY, SMALL, L64, L65, TWIN_A, TWIN_B = 0, 1, 2, 3, 4, 5, 6
NLIST_B = 300


# ------------------------------------------------------------------------------ the rule
def search_rule(lut, probe_d, probe_l, offsets, list_codes, list_ids, tau, metric, k):
    """(dists f32 (nq, k), ids uint32 (nq, k)); tau may be None for IP."""
    lut = np.asarray(lut, np.float32)
    probe_d = np.asarray(probe_d, np.float32)
    nq, M, _ = lut.shape
    pl = np.asarray(probe_l).astype(np.int64) & 0xFFFFFFFF
    ids64 = np.asarray(list_ids).astype(np.int64) & 0xFFFFFFFF
    codes = np.asarray(list_codes, np.uint8)
    two = np.float32(2.0)
    dd = np.full((nq, k), np.inf, np.float32)
    ii = np.full((nq, k), NO_ID, np.uint32)
    with np.errstate(invalid="ignore", over="ignore"):
        for a in range(nq):
            slots = np.nonzero(pl[a] != NO_ID)[0]
            if slots.size == 0:
                continue
            rows = np.concatenate([np.arange(offsets[l], offsets[l + 1]) for l in pl[a, slots]])
            if rows.size == 0:
                continue
            base = np.concatenate([np.full(int(offsets[l + 1] - offsets[l]), probe_d[a, s], np.float32)
                                   for s, l in zip(slots, pl[a, slots])])
            S = np.zeros(rows.size, np.float32)
            for m in range(M):
                S = S + lut[a, m][codes[rows, m]]
            dist = (base + np.asarray(tau, np.float32)[rows]) + two * S if metric == L2 else base + S
            assert dist.dtype == np.float32
            dist = np.where(np.isnan(dist), np.float32(np.inf), dist)
            order = np.lexsort((ids64[rows], dist))[:k]
            dd[a, :order.size] = dist[order]
            ii[a, :order.size] = ids64[rows][order].astype(np.uint32)
    return dd, ii


def merge_rule(dists, ids, k):
    """mivq_topk_merge: (parts, nq, k) candidate lists -> the k smallest (dist, id) per query."""
    dists = np.asarray(dists, np.float32)
    parts, nq, kk = dists.shape
    assert kk == k
    ids64 = np.asarray(ids).astype(np.int64) & 0xFFFFFFFF
    dd = np.full((nq, k), np.inf, np.float32)
    ii = np.full((nq, k), NO_ID, np.uint32)
    for a in range(nq):
        d = dists[:, a, :].reshape(-1)
        i = ids64[:, a, :].reshape(-1)
        d = np.where(np.isnan(d), np.float32(np.inf), d)
        order = np.lexsort((i, d))[:k]
        dd[a, :order.size] = d[order]
        ii[a, :order.size] = i[order].astype(np.uint32)
    return dd, ii


# ------------------------------------------------------------------------------ constructed lists
def _quarters(rng, shape):
    return (rng.integers(-8, 9, shape) / 4.0).astype(np.float32)


def _make_lists(sizes, M, nbits, rng):
    sizes = np.asarray(sizes, np.int64)
    n = int(sizes.sum())
    offsets = np.zeros(len(sizes) + 1, np.int64)
    offsets[1:] = np.cumsum(sizes)
    codes = rng.integers(0, 1 << nbits, (n, M)).astype(np.uint8)
    ids = rng.permutation(n).astype(np.int64)
    high = rng.choice(n, n // 10, replace=False)
    ids[high] = (1 << 31) + rng.choice((1 << 31) - 1, high.size, replace=False)  # distinct, <= 0xFFFFFFFE
    assert len(set(ids.tolist())) == n and ids.max() < NO_ID
    tau = {"generic": rng.standard_normal(n).astype(np.float32), "ties": _quarters(rng, n)}
    return dict(offsets=offsets, codes=codes, ids=ids.astype(np.uint32), tau=tau, M=M, nbits=nbits,
                nlist=len(sizes), n=n, nan_id=None, inf_row=0)


_sets = {}


def data_set(name, M, nbits):
    """Set "A" or "B" for (M, nbits), made once."""
    key = (name, M, nbits)
    if key in _sets:
        return _sets[key]
    rng = np.random.default_rng([ord(name), M, nbits, 11])
    if name == "B":
        sizes = rng.choice(6, NLIST_B, p=[0.2, 0.2, 0.25, 0.15, 0.1, 0.1])
        D = _make_lists(sizes, M, nbits, rng)
        assert 500 <= D["n"] <= 700 and (sizes == 0).any()
    else:
        sizes = np.zeros(NLIST_A, np.int64)
        sizes[[BIG, EMPTY, SMALL, L64, L65]] = (2500, 0, 20, 64, 65)
        rest = [l for l in range(NLIST_A) if l > L65]
        cut = np.sort(rng.choice(np.arange(1, 351), len(rest) - 1, replace=False))
        sizes[rest] = np.diff(np.concatenate([[0], cut, [351]]))
        assert sizes.sum() == 3000 and (sizes[rest] > 0).all()
        D = _make_lists(sizes, M, nbits, rng)
        off, codes, tau = D["offsets"], D["codes"], D["tau"]
        a, b = off[BIG] + 7, off[BIG] + 1900           # duplicates inside BIG
        ta, tb = off[TWIN_A], off[TWIN_B + 1] - 1      # duplicates across two lists
        for x, y in ((a, b), (ta, tb)):
            codes[y] = codes[x]
            for t in tau.values():
                t[y] = t[x]
        nan_row = off[SMALL] + 13
        for t in tau.values():
            t[nan_row] = np.nan
        D.update(dups=[(int(a), int(b)), (int(ta), int(tb))], nan_id=int(D["ids"][nan_row]),
                 inf_row=int(off[BIG] + 100))
    D["sizes"] = np.diff(D["offsets"])
    _sets[key] = D
    return D


def list_distances(D, kind, nq, seed):
    """PD (nq, nlist): the coarse distance of (query, list); probe_d follows the probe table.
    TWIN_A and TWIN_B of set A get equal values."""
    rng = np.random.default_rng([seed, nq, 3])
    PD = (rng.standard_normal((nq, D["nlist"])).astype(np.float32) if kind == "generic"
          else _quarters(rng, (nq, D["nlist"])))
    if D["nlist"] == NLIST_A:
        PD[:, TWIN_B] = PD[:, TWIN_A]
    return PD


def make_lut(D, kind, nq, seed):
    rng = np.random.default_rng([seed, nq, 5])
    M, ksub = D["M"], 1 << D["nbits"]
    if kind == "generic":
        return rng.standard_normal((nq, M, ksub)).astype(np.float32)
    lut = _quarters(rng, (nq, M, ksub))
    row = D["codes"][D["inf_row"]]
    if M >= 2:  # the row (and every row sharing both codes) sees +inf then -inf: NaN
        lut[0::2, 0, row[0]] = np.inf
        lut[0::2, M - 1, row[M - 1]] = -np.inf
    else:       # M = 1: two codes that occur in the data
        other = D["codes"][D["codes"][:, 0] != row[0]][0, 0]
        lut[0::2, 0, row[0]] = np.inf
        lut[0::2, 0, other] = -np.inf
    return lut


def make_probes(D, probes, nq, nprobe, seed):
    """(nq, nprobe) uint32, distinct lists per query.
    "rand":  random distinct lists; on set A BIG, EMPTY and SMALL are forced in by turns when
             nprobe >= 5, nprobe = 1 walks SMALL, BIG, EMPTY, 3, 4, ..., and nprobe = 17 is
             all 16 lists and one skipped slot.
    "skips": the same with about a quarter of the slots 0xFFFFFFFF, every slot of query nq // 2
             skipped (nq > 1) and, for nprobe > 16, query 0 keeping its first 3 slots only (the
             other waves and every later split of that query own nothing).
    "empty_alone", "small_alone": nprobe = 1, that list for every query."""
    rng = np.random.default_rng([seed, nq, nprobe, 7])
    nlist = D["nlist"]
    set_a = nlist == NLIST_A
    if probes in ("empty_alone", "small_alone"):
        assert set_a and nprobe == 1
        return np.full((nq, 1), EMPTY if probes == "empty_alone" else SMALL, np.uint32)
    real = min(nprobe, nlist)
    P = np.full((nq, nprobe), NO_ID, np.int64)
    for a in range(nq):
        P[a, rng.permutation(nprobe)[:real]] = rng.permutation(nlist)[:real]
    if set_a and nprobe == 1:
        walk = [SMALL, BIG, EMPTY] + list(range(3, NLIST_A))
        P[:, 0] = [walk[a % len(walk)] for a in range(nq)]
    elif set_a and nprobe < nlist:
        for a in range(nq):
            force = (BIG, EMPTY, SMALL)[a % 3]
            if force not in P[a]:
                P[a, a % nprobe] = force
    if probes == "skips":
        P[rng.random(P.shape) < 0.25] = NO_ID
        if nprobe > 16:
            P[0, 3:] = NO_ID
        if nq > 1:
            P[nq // 2] = NO_ID
    else:
        assert probes == "rand"
    for a in range(nq):
        r = P[a][P[a] != NO_ID]
        assert len(set(r.tolist())) == r.size
    return P.astype(np.uint32)


def probe_distances(PD, P):
    """probe_d (nq, nprobe) for probe table P (skipped slots get 0, never read)."""
    safe = np.where(P == NO_ID, 0, P).astype(np.int64)
    out = np.take_along_axis(PD, safe, 1)
    return np.where(P == NO_ID, np.float32(0), out).astype(np.float32)


# (set, M, nbits, metric, kind, k, nq, nprobe, probes).  Byte path of the scan: M % 4 != 0.
# Probe splits = min(ceil(512 / nq), ceil(nprobe / 16)): nq = 1 x nprobe = 256 gives 16 (256 part
# lists into the merge), nq = 600 one whatever nprobe is, nprobe = 17 two.  M = 64 / 128 at nbits = 8
# are exactly 64 KiB / 128 KiB of LDS.
CASES = [
    ("A", 8, 8, L2, "generic", 10, 37, 16, "rand"),
    ("A", 8, 8, IP, "ties", 256, 37, 16, "rand"),
    ("A", 4, 8, L2, "ties", 64, 5, 5, "rand"),
    ("A", 16, 8, IP, "generic", 65, 600, 5, "skips"),
    ("A", 1, 8, L2, "generic", 128, 5, 16, "skips"),
    ("A", 1, 1, IP, "ties", 10, 37, 5, "rand"),
    ("A", 3, 5, L2, "ties", 129, 37, 17, "rand"),
    ("A", 3, 8, IP, "generic", 1, 1, 1, "rand"),
    ("A", 6, 8, L2, "generic", 192, 5, 16, "rand"),
    ("A", 6, 4, IP, "ties", 193, 37, 16, "skips"),
    ("A", 10, 8, L2, "ties", 256, 1, 16, "rand"),
    ("A", 10, 5, IP, "generic", 10, 600, 1, "rand"),
    ("A", 64, 8, L2, "generic", 10, 5, 16, "rand"),
    ("A", 64, 8, IP, "ties", 65, 37, 5, "skips"),
    ("A", 128, 8, L2, "generic", 10, 5, 16, "rand"),
    ("A", 128, 8, IP, "ties", 256, 1, 17, "rand"),
    ("A", 16, 1, L2, "ties", 129, 5, 5, "rand"),
    ("A", 8, 4, L2, "generic", 100, 5, 1, "empty_alone"),
    ("A", 8, 4, L2, "ties", 100, 5, 1, "small_alone"),
    ("A", 6, 8, L2, "generic", 100, 1, 1, "small_alone"),
    ("B", 8, 8, L2, "generic", 10, 1, 256, "rand"),
    ("B", 6, 8, IP, "ties", 256, 1, 256, "rand"),
    ("B", 4, 4, L2, "ties", 64, 37, 50, "rand"),
    ("B", 10, 1, IP, "generic", 128, 5, 50, "skips"),
    ("B", 16, 5, L2, "generic", 192, 600, 256, "rand"),
    ("B", 3, 8, L2, "ties", 1, 600, 17, "skips"),
    ("B", 1, 4, IP, "generic", 193, 37, 17, "rand"),
]

def assert_cases_cover_the_issue():
    """What the case table must hold as a whole (run by the CPU and the GPU suite)."""
    C = CASES
    assert 20 <= len(C) <= 30 and len(set(C)) == len(C)
    assert {c[1] for c in C if c[1] % 4} == {1, 3, 6, 10}        # byte path
    assert {c[1] for c in C if c[1] % 4 == 0} == {4, 8, 16, 64, 128}  # word path
    assert {c[2] for c in C} == {1, 4, 5, 8}
    assert all(c[2] == 8 for c in C if c[1] in (64, 128))         # exactly 64 KiB / 128 KiB of LDS
    assert {c[5] for c in C} >= {1, 10, 64, 65, 128, 129, 192, 193, 256}
    assert {c[6] for c in C} == {1, 5, 37, 600}
    assert {c[7] for c in C} == {1, 5, 16, 17, 50, 256}
    assert all(c[0] == "B" for c in C if c[7] in (50, 256)) and all(c[7] >= 17 for c in C if c[0] == "B")
    for path in (lambda c: c[1] % 4 != 0, lambda c: c[1] % 4 == 0):
        sub = [c for c in C if path(c)]
        assert {c[3] for c in sub} == {L2, IP}
        assert {c[4] for c in sub} == {"generic", "ties"}
        assert {(c[5] + 63) // 64 for c in sub} == {1, 2, 3, 4}   # every count of list registers
    assert {c[8] for c in C} == {"rand", "skips", "empty_alone", "small_alone"}
    assert any(c[8] == "small_alone" and c[5] == 100 for c in C)
    # splits of 1, 2 and 16 (ivf_splits of csrc/ivf.hip restated)
    splits = {max(1, min(-(-512 // c[6]), -(-c[7] // 16))) for c in C}
    assert splits >= {1, 2, 16}
    assert any(c[6] >= 512 and c[7] > 16 for c in C)              # one split whatever nprobe is
    # SMALL probed alone under L2 with k above its 20 rows: the NaN-tau row must show, both kinds
    assert {c[4] for c in C if c[8] == "small_alone" and c[3] == L2 and c[5] >= 20} == {"generic", "ties"}


_inputs = {}
_expected = {}


def case_inputs(case):
    """The arrays of one case, made once: D (the lists), lut, probe_l, probe_d, tau (None for IP)."""
    if case not in _inputs:
        name, M, nbits, metric, kind, k, nq, nprobe, probes = case
        D = data_set(name, M, nbits)
        seed = CASES.index(case) if case in CASES else 99
        P = make_probes(D, probes, nq, nprobe, seed)
        PD = list_distances(D, kind, nq, seed)
        _inputs[case] = dict(D=D, lut=make_lut(D, kind, nq, seed), probe_l=P, PD=PD,
                             probe_d=probe_distances(PD, P), tau=D["tau"][kind] if metric == L2 else None)
    return _inputs[case]


def case_expected(case):
    """The rule's (dists, ids) of one case, computed once and shared; do not modify."""
    if case not in _expected:
        I = case_inputs(case)
        D = I["D"]
        dd, ii = search_rule(I["lut"], I["probe_d"], I["probe_l"], D["offsets"], D["codes"], D["ids"], I["tau"],
                             case[3], case[5])
        dd.setflags(write=False)
        ii.setflags(write=False)
        _expected[case] = (dd, ii)
    return _expected[case]


def rows_probed(D, P):
    """Rows of the lists each query probes, (nq,)."""
    sizes = np.concatenate([D["sizes"], [0]])
    return sizes[np.where(P == NO_ID, D["nlist"], P).astype(np.int64)].sum(1)


# The nq > 65,535 input: seven distinct queries tiled over a 4-list, 40-row index.
BIG_NQ = 65541


def tiled_case():
    rng = np.random.default_rng(6)
    M, nbits, nprobe, k = 4, 4, 2, 3
    D = _make_lists([13, 0, 20, 7], M, nbits, rng)
    lut = _quarters(rng, (7, M, 1 << nbits))  # ties: the id order matters in every chunk
    P = np.array([[0, 2], [1, 3], [2, NO_ID], [3, 0], [NO_ID, NO_ID], [1, NO_ID], [2, 3]], np.uint32)
    pd = _quarters(rng, (7, nprobe))
    return dict(D=D, lut=lut, probe_l=P, probe_d=pd, tau=D["tau"]["ties"], k=k, nbits=nbits)


# ------------------------------------------------------------------------------ merge inputs
# (parts, k, nq, kind)
MERGE_CASES = [
    (0, 10, 3, "generic"), (1, 1, 1, "generic"), (1, 256, 5, "ties"), (2, 64, 4, "ties"),
    (2, 10, 130, "generic"), (3, 65, 5, "generic"), (3, 1, 130, "ties"), (17, 10, 4, "ties"),
    (17, 256, 3, "generic"), (17, 65, 130, "generic"), (256, 64, 1, "generic"), (256, 65, 5, "ties"),
    (256, 256, 3, "ties"),
]


def merge_inputs(parts, k, nq, kind):
    """(dists f32 (parts, nq, k), ids uint32 (parts, nq, k)): every (part, query) list sorted by
    (dist, id) with NaN ranked as +inf; whole parts of padding, lists ending in padding, equal
    distances across parts under distinct ids, ids >= 2^31, a few NaN distances."""
    rng = np.random.default_rng([parts, k, nq, 13])
    dd = np.full((parts, nq, k), np.inf, np.float32)
    ii = np.full((parts, nq, k), NO_ID, np.uint32)
    for a in range(nq):
        total = parts * k
        pool = rng.permutation(max(total, 1) * 2)[:total].astype(np.int64)
        hi = rng.random(total) < 0.3
        pool[hi] += 1 << 31  # distinct below and above 2^31, never 0xFFFFFFFF
        pool = pool.reshape(parts, k)
        shared = rng.standard_normal(8).astype(np.float32)  # values that recur across parts
        for p in range(parts):
            mode = (p + a) % 4
            r = 0 if (mode == 1 and parts > 1) else (int(rng.integers(0, k + 1)) if mode == 2 else k)
            if r == 0:
                continue
            if kind == "ties":
                d = (rng.integers(0, 9, r) / 4.0).astype(np.float32)
            else:
                d = rng.standard_normal(r).astype(np.float32)
                pick = rng.random(r) < 0.3
                d[pick] = shared[rng.integers(0, 8, int(pick.sum()))]
            if rng.random() < 0.3:
                d[rng.integers(0, r)] = np.nan
            i = pool[p, :r]
            order = np.lexsort((i, np.where(np.isnan(d), np.inf, d)))
            dd[p, a, :r] = d[order]
            ii[p, a, :r] = i[order].astype(np.uint32)
    return dd, ii
