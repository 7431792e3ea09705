"""LVQ fixtures: the cases, their inputs, and a numpy restatement of the arithmetic.

Shared by the fixture generator (tests/golden/make_lvq_golden.py, which runs the reference's
LVQQuantizer and FlatQuantizedIndex) and by tests/test_lvq_cpu.py / tests/test_lvq_gpu.py.
Everything here is numpy on the host; nothing of the reference is imported.

The restatement is written one float32 operation per step (every intermediate is a float32
array, every scalar a np.float32), in the order include/mivq.h documents:

    mean   : column sums in ascending row order, then one division by float32(N)
    encode : r = x - mu, lo = min r, hi = max r, span = hi - lo,
             delta = tiny if span == 0 else span / float32(L),
             idx = clip(rint((r - lo) / delta), 0, L)            (rint: half to even)
    row    : idx_t in bits [t B, (t + 1) B) of the bit stream, MSB-first from byte 0, padding
             bits 0; then lo and delta as little-endian float32
    decode : (lo + float32(idx) * delta) + mu
"""

from __future__ import annotations

import hashlib

import numpy as np

F32 = np.float32
TINY = np.finfo(np.float32).tiny  # FLT_MIN

# name -> N, D, B, nq, k.  The first nine are searched (L2 and IP); `wide*` and `beyond` are
# encode / decode only (3072 and 1536: the widths of the benchmarks, 6 and 3 groups of 8
# dimensions per lane; 5000: past the 3072 dimensions the encoder keeps in registers).
SEARCH_CASES = {
    "b8_d128": dict(N=2000, D=128, B=8, nq=16, k=10),
    "b4_d100": dict(N=1500, D=100, B=4, nq=16, k=10),
    "b3_d37": dict(N=1031, D=37, B=3, nq=9, k=10),
    "b1_d200": dict(N=1200, D=200, B=1, nq=9, k=10),
    "b5_d64": dict(N=900, D=64, B=5, nq=9, k=10),
    "b6_d96": dict(N=900, D=96, B=6, nq=9, k=10),
    "b7_d33": dict(N=900, D=33, B=7, nq=9, k=10),
    "b2_d61": dict(N=900, D=61, B=2, nq=9, k=10),
    "b8_tiny": dict(N=7, D=16, B=8, nq=3, k=10),  # k is clamped to N
}
CODEC_CASES = {
    "wide_b8_d3072": dict(N=130, D=3072, B=8, nq=0, k=0),
    "wide_b4_d1536": dict(N=130, D=1536, B=4, nq=0, k=0),
    "beyond_b3_d5000": dict(N=9, D=5000, B=3, nq=0, k=0),
}
CASES = {**SEARCH_CASES, **CODEC_CASES}
METRICS = ("l2", "ip")
# a draw other than 0 replaces a case's seed [N, D, B] by [N, D, B, draw] (used when the
# reference's own result leaves more than OPEN_CAP of a case's positions open)
DRAWS = {}


def sha(a) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def code_size(D: int, B: int) -> int:
    return (D * B + 7) // 8 + 8


def seed_of(name: str):
    c = CASES[name]
    s = [c["N"], c["D"], c["B"]]
    return s + [DRAWS[name]] if DRAWS.get(name) else s


def inputs(name: str):
    """(X, Q, planted) float32 of a case from its seed.  X = N(0,1) U(0.2,3)[per dim] +
    N(0,1)[per dim], Q = N(0,1).  Row `planted` is then set to the mean of X (repeated until the
    float32 mean stops moving, each time 1/N of the previous change), so its residual is 0 in
    every dimension: span == 0, delta = FLT_MIN, every index 0."""
    c = CASES[name]
    N, D, nq = c["N"], c["D"], c["nq"]
    rng = np.random.default_rng(seed_of(name))
    X = (rng.standard_normal((N, D)) * rng.uniform(0.2, 3.0, D) + rng.standard_normal(D)).astype(F32)
    Q = rng.standard_normal((nq, D)).astype(F32)
    planted = int(rng.integers(0, N))
    for _ in range(50):
        mu = X.mean(axis=0)
        if np.array_equal(X[planted], mu):
            break
        X[planted] = mu
    else:
        raise AssertionError(f"{name}: the planted row did not settle on the mean")
    return X, Q, planted


# ------------------------------------------------------------------------------ the restatement
def seq_mean(X) -> np.ndarray:
    """Column sums in ascending row order in float32, then one float32 division by N."""
    X = np.ascontiguousarray(X, dtype=F32)
    acc = np.zeros(X.shape[1], dtype=F32)
    for row in X:
        acc = acc + row
    return acc / F32(X.shape[0])


def quantize(X, mu, B):
    """(idx int32 (N, D), lo float32 (N,), delta float32 (N,))."""
    L = (1 << B) - 1
    R = np.ascontiguousarray(X, dtype=F32) - np.asarray(mu, dtype=F32)
    lo, hi = R.min(axis=1), R.max(axis=1)
    span = hi - lo
    with np.errstate(divide="ignore", invalid="ignore"):
        delta = np.where(span == F32(0.0), TINY, span / F32(L)).astype(F32)
        q = (R - lo[:, None]) / delta[:, None]
    assert R.dtype == span.dtype == q.dtype == F32
    idx = np.clip(np.rint(q), 0, L).astype(np.int32)
    return idx, lo.astype(F32), delta


def pack(idx, lo, delta, B) -> np.ndarray:
    """The code rows: bit b (from the top) of idx_t goes to bit t B + b of the row's stream,
    bit 0 of the stream being the top bit of byte 0."""
    N, D = idx.shape
    ib = (D * B + 7) // 8
    codes = np.zeros((N, ib + 8), dtype=np.uint8)
    for t in range(D):
        for b in range(B):
            pos = t * B + b
            bit = ((idx[:, t] >> (B - 1 - b)) & 1).astype(np.uint8)
            codes[:, pos >> 3] |= bit << np.uint8(7 - (pos & 7))
    codes[:, ib:ib + 4] = np.ascontiguousarray(lo, dtype="<f4").view(np.uint8).reshape(N, 4)
    codes[:, ib + 4:] = np.ascontiguousarray(delta, dtype="<f4").view(np.uint8).reshape(N, 4)
    return codes


def encode(X, mu, B) -> np.ndarray:
    return pack(*quantize(X, mu, B), B)


def unpack(codes, D, B):
    """(idx int32 (N, D), lo, delta) of code rows."""
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    N = codes.shape[0]
    ib = (D * B + 7) // 8
    assert codes.shape[1] == ib + 8
    idx = np.zeros((N, D), dtype=np.int32)
    for t in range(D):
        for b in range(B):
            pos = t * B + b
            bit = (codes[:, pos >> 3] >> np.uint8(7 - (pos & 7))) & 1
            idx[:, t] |= bit.astype(np.int32) << (B - 1 - b)
    lo = codes[:, ib:ib + 4].copy().view("<f4").reshape(N).astype(F32)
    delta = codes[:, ib + 4:].copy().view("<f4").reshape(N).astype(F32)
    return idx, lo, delta


def decode(codes, mu, B) -> np.ndarray:
    mu = np.asarray(mu, dtype=F32)
    idx, lo, delta = unpack(codes, mu.shape[0], B)
    prod = idx.astype(F32) * delta[:, None]
    return (lo[:, None] + prod) + mu[None, :]


def padding_bits(codes, D, B) -> np.ndarray:
    """The bits of the last index byte past D B (all must be 0), per row."""
    ib = (D * B + 7) // 8
    spare = ib * 8 - D * B
    return codes[:, ib - 1] & np.uint8((1 << spare) - 1)


# planted half-to-even ties with mu = 0: (B, leading values, expected leading indices).  The
# row is padded with interior values up to the case's D; min and max are the first and last of
# the leading values, so delta = (max - min) / L is exact and the quotients 0.5, 1.5, 2.5 are ties.
ROUNDING = [
    (2, [0.0, 1.5, 4.5, 7.5, 9.0], [0, 0, 2, 2, 3]),
    (1, [0.0, 0.5, 1.0], [0, 0, 1]),
]


def rounding_row(B, D):
    """(row float32 (D,), expected leading indices) of the planted-rounding case for B."""
    lead, want = next((v, w) for b, v, w in ROUNDING if b == B)
    fill = {2: 3.25, 1: 0.75}[B]  # interior, not a tie
    row = np.full(D, fill, dtype=F32)
    row[:len(lead)] = lead
    return row, want


# ------------------------------------------------------------------------------ fixture cases
def load_fixture(golden_dir) -> dict:
    with np.load(golden_dir / "lvq_golden.npz") as z:
        return {k: z[k] for k in z.files}


class Case:
    """One fixture case: regenerated inputs, the reference's mean, codes (or digest) and
    reconstruction digest, and the restatement's codes and reconstruction (computed once)."""

    def __init__(self, name, lg):
        self.name, self.c, self.lg = name, CASES[name], lg
        self.N, self.D, self.B = self.c["N"], self.c["D"], self.c["B"]
        self.X, self.Q, self.planted = inputs(name)
        assert list(lg[f"{name}_seed"]) == seed_of(name)
        assert sha(self.X) == str(lg[f"{name}_X_sha"]), f"{name}: regenerated X differs from the fixture's"
        assert sha(self.Q) == str(lg[f"{name}_Q_sha"]), f"{name}: regenerated Q differs from the fixture's"
        assert self.planted == int(lg[f"{name}_planted"])
        self.mu = lg[f"{name}_mu"]
        self.codes = encode(self.X, self.mu, self.B)
        self.rec = decode(self.codes, self.mu, self.B)
        self._judges = {}

    def codes_match(self, codes) -> None:
        """`codes` are the reference's (stored in full, or as digest + first rows)."""
        codes = np.ascontiguousarray(codes)
        assert codes.dtype == np.uint8 and codes.shape == (self.N, code_size(self.D, self.B))
        if f"{self.name}_codes" in self.lg:
            np.testing.assert_array_equal(codes, self.lg[f"{self.name}_codes"])
        else:
            np.testing.assert_array_equal(codes[:8], self.lg[f"{self.name}_codes_head"])
            assert sha(codes) == str(self.lg[f"{self.name}_codes_sha"]), f"{self.name}: codes differ"

    def rec_match(self, rec) -> None:
        rec = np.ascontiguousarray(rec)
        assert rec.dtype == np.float32 and rec.shape == (self.N, self.D)
        np.testing.assert_array_equal(rec[:4].view(np.uint32), self.lg[f"{self.name}_rec_head"].view(np.uint32))
        assert sha(rec) == str(self.lg[f"{self.name}_rec_sha"]), f"{self.name}: reconstruction differs"

    def judge(self, metric):
        from _search_rule import Judge

        if metric not in self._judges:
            self._judges[metric] = Judge(self.Q, self.rec, metric, self.c["k"])
        return self._judges[metric]

    def ref(self, metric):
        return self.lg[f"{self.name}_{metric}_ids"], self.lg[f"{self.name}_{metric}_dists"]
