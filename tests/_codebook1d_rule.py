"""The data-fitted 1-D codebooks of the rank-aware quantizer restated in numpy, and their cases.

Input: one dimension's sample as f32, sorted ascending (``s``, n values); ``w`` bits, k = 2 ** w
levels.  All arithmetic is fp64, every product and quotient rounded on its own (no FMA).

  prefix     ps[0] = pq[0] = 0, ps[i + 1] = ps[i] + s_i, pq[i + 1] = pq[i] + (s_i * s_i), summed
             strictly in ascending order.  For [i, j): S = ps[j] - ps[i], c = (double)(j - i),
             mean = S / c, sse = (pq[j] - pq[i]) - S * S / c.
  degenerate k >= the number of distinct values: the distinct values ascending, padded with the
             last one to k; sse 0.
  exact      the optimal 1-D k-means by dynamic programming: D_1[m] = sse(0, m); for kp = 2..k a
             divide and conquer over m from the root (mlo, mhi, jlo, jhi) = (kp, n, kp - 1, n - 1):
             mid = (mlo + mhi) // 2, candidates j = max(kp - 1, jlo) .. min(mid - 1, jhi) ascending,
             value D_{kp-1}[j] + sse(j, mid), the first strict minimum wins (none: +inf, jlo);
             children (mlo, mid - 1, jlo, arg) when mid > mlo and (mid + 1, mhi, arg, jhi).  The
             levels are the f32 means of the backtracked cells, equal neighbours dropped, padded
             with the last to k; sse = D_k[n].  The search windows are part of the rule.
  lloyd      k-means++ seeding from the raw outputs of mt19937_64(0), then at most 50 passes with
             one empty-cell repair per pass (``lloyd``'s docstring).

Both return f32 levels and an fp64 sse.  The reference leaves the degenerate Lloyd table
unpadded; a level table here always has exactly 2 ** w entries.
"""

from __future__ import annotations

import hashlib

import numpy as np

GOLDEN = "codebook1d_golden.npz"
METHODS = ("exact", "lloyd")
MAX_PASSES = 50
TOL = float(np.float32(1e-6))
M64 = (1 << 64) - 1


# ------------------------------------------------------------------ mt19937_64
class MT19937_64:
    """The 64-bit Mersenne Twister (Matsumoto & Nishimura 2004), seeded like std::mt19937_64."""

    def __init__(self, seed: int = 5489):
        mt = [0] * 312
        mt[0] = seed & M64
        for i in range(1, 312):
            mt[i] = (6364136223846793005 * (mt[i - 1] ^ (mt[i - 1] >> 62)) + i) & M64
        self.mt, self.i = mt, 312

    def _twist(self) -> None:
        mt = self.mt
        for i in range(312):
            x = (mt[i] & 0xFFFFFFFF80000000) | (mt[(i + 1) % 312] & 0x7FFFFFFF)
            mt[i] = mt[(i + 156) % 312] ^ (x >> 1) ^ (0xB5026F5AA96619E9 if x & 1 else 0)
        self.i = 0

    def __call__(self) -> int:
        if self.i >= 312:
            self._twist()
        x = self.mt[self.i]
        self.i += 1
        x ^= (x >> 29) & 0x5555555555555555
        x ^= (x << 17) & 0x71D67FFFEDA60000
        x ^= (x << 37) & 0xFFF7EEE000000000
        x ^= x >> 43
        return x & M64


def draw_index(rng, n: int) -> int:
    """A uniform index in [0, n) from raw 64-bit draws: the high half of draw * n, a draw whose
    low half falls under 2^64 mod n rejected."""
    prod = rng() * n
    low = prod & M64
    if low < n:
        thr = ((1 << 64) - n) % n
        while low < thr:
            prod = rng() * n
            low = prod & M64
    return prod >> 64


def draw_unit(rng) -> float:
    """(double)draw / 2^64, a quotient of 1 replaced by the largest double below 1."""
    u = float(np.float64(np.uint64(rng()))) / 18446744073709551616.0
    return u if u < 1.0 else float(np.nextafter(1.0, 0.0))


# ------------------------------------------------------------------ prefix sums
def prefix(s):
    v = np.asarray(s, dtype=np.float32).astype(np.float64)
    ps = np.cumsum(np.concatenate(([0.0], v)))
    pq = np.cumsum(np.concatenate(([0.0], v * v)))
    return ps, pq


def _mean(ps, a, b):
    return (ps[b] - ps[a]) / np.asarray(b - a, dtype=np.float64)


def _sse(ps, pq, a, b):
    S = ps[b] - ps[a]
    return (pq[b] - pq[a]) - S * S / np.asarray(b - a, dtype=np.float64)


def _seqsum(vals) -> float:
    return float(np.cumsum(np.concatenate(([0.0], np.asarray(vals, dtype=np.float64))))[-1])


def distinct(s) -> np.ndarray:
    s = np.asarray(s, dtype=np.float32)
    return s[np.concatenate(([True], s[1:] != s[:-1]))] if len(s) else s


def _pad(levels, k: int) -> np.ndarray:
    levels = np.asarray(levels, dtype=np.float32)
    return np.concatenate((levels, np.full(k - len(levels), levels[-1], dtype=np.float32)))


def _drop_equal(levels) -> np.ndarray:
    levels = np.asarray(levels, dtype=np.float32)
    return levels[np.concatenate(([True], levels[1:] != levels[:-1]))]


# ------------------------------------------------------------------ exact
def _dp_level(ps, pq, Dprev, n: int, kp: int):
    """One level of the DP, the recursion walked breadth-first: (D_kp, A_kp)."""
    Dcur = np.full(n + 1, np.inf)
    A = np.zeros(n + 1, dtype=np.int64)
    mlo, mhi = np.array([kp]), np.array([n])
    jlo, jhi = np.array([kp - 1]), np.array([n - 1])
    while len(mlo):
        mid = (mlo + mhi) // 2
        lo, hi = np.maximum(kp - 1, jlo), np.minimum(mid - 1, jhi)
        cnt = np.maximum(hi - lo + 1, 0)
        best = np.full(len(mid), np.inf)
        arg = jlo.copy()
        live = np.flatnonzero(cnt > 0)
        if len(live):
            c = cnt[live]
            start = np.concatenate(([0], np.cumsum(c)[:-1]))
            seg = np.repeat(np.arange(len(live)), c)
            pos = np.arange(int(c.sum()))
            j = lo[live][seg] + (pos - start[seg])
            v = Dprev[j] + _sse(ps, pq, j, mid[live][seg])
            vmin = np.minimum.reduceat(v, start)
            first = np.minimum.reduceat(np.where(v == vmin[seg], pos, len(pos)), start)
            hit = vmin < np.inf          # a strict minimum below +inf exists
            best[live[hit]] = vmin[hit]
            arg[live[hit]] = j[first[hit]]
        Dcur[mid], A[mid] = best, arg
        left, right = mid > mlo, mid + 1 <= mhi
        mlo, mhi, jlo, jhi = (np.concatenate((mlo[left], mid[right] + 1)), np.concatenate((mid[left] - 1, mhi[right])),
                              np.concatenate((jlo[left], arg[right])), np.concatenate((arg[left], jhi[right])))
    return Dcur, A


def exact(s, w: int):
    """(levels f32 (2 ** w,), sse)."""
    s = np.asarray(s, dtype=np.float32)
    n, k = len(s), 1 << w
    ds = distinct(s)
    if k >= len(ds):
        return _pad(ds, k), 0.0
    ps, pq = prefix(s)
    m = np.arange(n + 1)
    D = np.full(n + 1, np.inf)
    D[1:] = _sse(ps, pq, np.zeros(n, dtype=np.int64), m[1:])
    As = {}
    for kp in range(2, k + 1):
        D, As[kp] = _dp_level(ps, pq, D, n, kp)
    levels, m = [], n
    for kk in range(k, 0, -1):
        j = int(As[kk][m]) if kk > 1 else 0
        levels.append(np.float32(_mean(ps, j, m)))
        m = j
    return _pad(_drop_equal(levels[::-1]), k), float(D[n])


# ------------------------------------------------------------------ lloyd
def _nudge(c) -> None:
    for i in range(1, len(c)):
        if c[i] <= c[i - 1]:
            c[i] = c[i - 1] + max(1e-9, abs(c[i - 1]) * 1e-6)


def seed_centres(s, k: int, rng=None) -> np.ndarray:
    """k-means++ over the sorted sample: the sorted, nudged fp64 centres."""
    s = np.asarray(s, dtype=np.float32)
    n = len(s)
    rng = rng or MT19937_64(0)
    v = s.astype(np.float64)
    centres = [float(v[draw_index(rng, n)])]
    diff = v - centres[0]
    d2 = diff * diff
    while len(centres) < k:
        acc = np.cumsum(np.concatenate(([0.0], d2)))[1:]
        total = acc[-1]
        if total <= 0.0:
            chosen = draw_index(rng, n)
        else:
            target = draw_unit(rng) * total
            ge = acc >= target
            chosen = int(np.argmax(ge)) if ge.any() else n - 1
        centres.append(float(v[chosen]))
        diff = v - v[chosen]
        dd = diff * diff
        d2 = np.where(dd < d2, dd, d2)
    c = np.sort(np.array(centres))
    _nudge(c)
    return c


def _assign(s, c, n: int) -> np.ndarray:
    mids = (0.5 * (c[:-1] + c[1:])).astype(np.float32)
    inner = np.maximum.accumulate(np.concatenate(([0], np.searchsorted(s, mids, side="right"))))
    return np.concatenate((inner, [n])).astype(np.int64)


def lloyd(s, w: int, max_passes: int = MAX_PASSES, info: dict | None = None):
    """(levels f32 (2 ** w,), sse).  Seeding: seed_centres.  A pass: bnd[i] = #{s <= (float)(0.5
    (c[i-1] + c[i]))} made non-decreasing, bnd[0] = 0, bnd[k] = n; c[i] = the mean of its cell
    where the cell is not empty.  While fewer than 2 k repairs were made and a cell is empty, the
    first empty cell e and the cell of >= 2 points with the largest sse (first on ties) share the
    donor's points: m = a + (b - a) // 2, c[donor] = mean(a, m), c[e] = mean(m, b); sort, nudge,
    next pass without the convergence test.  Otherwise stop when the largest move < (double)1e-6f.
    The sse is that of a last assignment; the levels are the centres rounded to f32, sorted,
    unique, padded.  `info` receives passes / repairs / converged."""
    s = np.asarray(s, dtype=np.float32)
    n, k = len(s), 1 << w
    ds = distinct(s)
    if k >= len(ds):
        return _pad(ds, k), 0.0
    ps, pq = prefix(s)
    c = seed_centres(s, k)
    repairs, passes, converged = 0, 0, False
    for _ in range(max_passes):
        passes += 1
        bnd = _assign(s, c, n)
        a, b = bnd[:-1], bnd[1:]
        full = b > a
        nc = c.copy()
        nc[full] = _mean(ps, a[full], b[full])
        maxmove = float(np.max(np.abs(nc - c)))
        c = nc
        if repairs < 2 * k and not full.all():
            e = int(np.argmin(full))
            donors = np.flatnonzero(b > a + 1)
            if len(donors):
                cost = _sse(ps, pq, a[donors], b[donors])
                best, bsse = k, -1.0
                for j, v in zip(donors, cost):
                    if v > bsse:
                        best, bsse = int(j), v
                if best < k:
                    lo, hi = int(a[best]), int(b[best])
                    m = lo + (hi - lo) // 2
                    c[best] = _mean(ps, lo, m)
                    c[e] = _mean(ps, m, hi)
                    c = np.sort(c)
                    _nudge(c)
                    repairs += 1
                    continue
        if maxmove < TOL:
            converged = True
            break
    bnd = _assign(s, c, n)
    a, b = bnd[:-1], bnd[1:]
    full = b > a
    sse = _seqsum(_sse(ps, pq, a[full], b[full]))
    if info is not None:
        info.update(passes=passes, repairs=repairs, converged=converged)
    return _pad(np.unique(c.astype(np.float32)), k), sse


def fit(s, w: int, method: str):
    return exact(s, w) if method == "exact" else lloyd(s, w)


def table_sse(s, levels) -> float:
    """The sse of the sorted sample on an ascending level table (nearest level, fp64)."""
    v = np.asarray(s, dtype=np.float64)
    lv = np.asarray(levels, dtype=np.float64)
    idx = np.searchsorted(0.5 * (lv[:-1] + lv[1:]), v)
    return float(np.sum((v - lv[idx]) ** 2))


# ------------------------------------------------------------------ cases
def sha(a) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


# name -> (n, width, kind, draw); the sorted f32 column comes from column(name)
COLUMN_CASES = {
    "one": (1, 3, "gauss", 0),                 # n = 1
    "n_eq_k": (16, 4, "gauss", 0),             # n = 2^w: degenerate
    "n_eq_k1": (17, 4, "gauss", 0),            # n = 2^w + 1: the first DP
    "const": (500, 3, "const", 0),             # all values equal
    "few_under": (600, 4, "few15", 0),         # 15 distinct values, k = 16
    "few_over": (600, 4, "few17", 0),          # 17 distinct values, k = 16
    **{f"g1000_w{w}": (1000, w, "gauss", w) for w in range(1, 9)},
    "g4097_w1": (4097, 1, "gauss", 11),
    "g4097_w4": (4097, 4, "gauss", 12),
    "g4097_w8": (4097, 8, "gauss", 13),
    "g3000_w8": (3000, 8, "laplace", 0),       # the deepest DP
    "heavy": (2000, 5, "heavy", 0),            # heavy tails
    "tight": (2000, 5, "tight", 0),            # six tight clusters, k = 32
    "tight_w3": (1000, 3, "tight", 1),
    "gap": (38, 2, "gap", 0),                  # a cell empties in the second pass: one repair
}


def column(name: str) -> np.ndarray:
    n, _, kind, draw = COLUMN_CASES[name]
    rng = np.random.default_rng([n, draw, sum(kind.encode())])
    if kind == "gauss":
        x = rng.standard_normal(n) * 1.7 + 0.3
    elif kind == "laplace":
        x = rng.laplace(size=n)
    elif kind == "const":
        x = np.full(n, 1.25)
    elif kind.startswith("few"):
        x = rng.choice(rng.standard_normal(int(kind[3:])), n)
    elif kind == "gap":
        # seeds -4.9, 0, 20, 1000; the cell {0, 9.9} moves to 4.95 and loses both halves
        x = np.repeat([-4.9, 0.0, 9.9, 11.0, 20.0, 1000.0], [8, 10, 10, 6, 3, 1])
    elif kind == "heavy":
        x = rng.standard_t(1.5, n)
    else:
        x = rng.choice(np.array([-40.0, -3.0, -2.5, 0.0, 7.0, 100.0]), n) + 1e-3 * rng.standard_normal(n)
    return np.sort(x.astype(np.float32))
