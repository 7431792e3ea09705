"""Two-level LVQ (LVQ-B1xB2) fixtures: the cases, their inputs, and a numpy restatement of the rule.

Shared by tests/test_lvq2_cpu.py and tests/test_lvq2_gpu.py.  Everything here is numpy on the host.
No reference implementation of the second level exists, so this restatement is the definition the
kernels are held to; level 1 is _lvq_rule's, which tests/golden/lvq_golden.npz ties to the reference.

One float32 operation per step (every intermediate is a float32 array), in the order
include/mivq.h documents, L2 = 2^B2 - 1:

    level 1 : r = x - mu, and lo, delta, idx as _lvq_rule.quantize
    level 2 : a = lo + float32(idx) * delta          (the product rounded, then the sum)
              e = r - a
              lo2 = -0.5 * delta, delta2 = delta / float32(L2)     (subnormal quotients kept)
              j = clip(rint((e - lo2) / delta2), 0, L2)            (rint: half to even)
    rows    : codes1 = _lvq_rule.pack(idx, lo, delta); codes2 = j_t in bits [t B2, (t + 1) B2) of the
              row's stream, MSB-first from byte 0, padding bits 0, no trailer
    decode  : ((lo + float32(idx) * delta) + (lo2 + float32(j) * delta2)) + mu
"""

from __future__ import annotations

import functools

import numpy as np

import _lvq_rule as LR
import _rerank_rule as RR  # noqa: F401  (the re-rank rule the two-level tests rank with)

F32 = np.float32

# name -> (the _lvq_rule case whose inputs it takes, B1, B2).  The searched cases pair every
# primary width's own inputs (planted span-0 row included) with a residual width.
SEARCH_CASES = {
    "b4x4_d100": ("b4_d100", 4, 4),
    "b4x8_d100": ("b4_d100", 4, 8),
    "b8x8_d128": ("b8_d128", 8, 8),
    "b1x8_d200": ("b1_d200", 1, 8),
    "b3x4_d37": ("b3_d37", 3, 4),
    "b7x4_d33": ("b7_d33", 7, 4),
    "b2x8_d61": ("b2_d61", 2, 8),
}
# encode / decode only: 6 and 3 groups of 8 dimensions per lane, and past the 3072 dimensions the
# encoder keeps in registers
CODEC_CASES = {
    "wide_b8x8_d3072": ("wide_b8_d3072", 8, 8),
    "wide_b4x4_d1536": ("wide_b4_d1536", 4, 4),
    "beyond_b3x8_d5000": ("beyond_b3_d5000", 3, 8),
}
CASES = {**SEARCH_CASES, **CODEC_CASES}
PAIRS = sorted({(b1, b2) for _, b1, b2 in SEARCH_CASES.values()})


def code_sizes(D: int, B1: int, B2: int):
    return LR.code_size(D, B1), (D * B2 + 7) // 8


# ------------------------------------------------------------------------------ the restatement
def quantize2(X, mu, B1: int, B2: int):
    """(idx int32 (N, D), lo float32 (N,), delta float32 (N,), j int32 (N, D))."""
    L2 = (1 << B2) - 1
    idx, lo, delta = LR.quantize(X, mu, B1)
    R = np.ascontiguousarray(X, dtype=F32) - np.asarray(mu, dtype=F32)
    prod = idx.astype(F32) * delta[:, None]
    a = lo[:, None] + prod
    e = R - a
    lo2 = F32(-0.5) * delta
    with np.errstate(divide="ignore", invalid="ignore", under="ignore"):
        delta2 = delta / F32(L2)
        s = e - lo2[:, None]
        q = s / delta2[:, None]
    assert R.dtype == prod.dtype == a.dtype == e.dtype == lo2.dtype == delta2.dtype == s.dtype == q.dtype == F32
    j = np.clip(np.rint(q), 0, L2).astype(np.int32)
    return idx, lo, delta, j


def pack2(j, B2: int) -> np.ndarray:
    """The residual rows: bit b (from the top) of j_t goes to bit t B2 + b of the row's stream, bit 0
    of the stream being the top bit of byte 0."""
    N, D = j.shape
    codes = np.zeros((N, (D * B2 + 7) // 8), dtype=np.uint8)
    for t in range(D):
        for b in range(B2):
            pos = t * B2 + b
            bit = ((j[:, t] >> (B2 - 1 - b)) & 1).astype(np.uint8)
            codes[:, pos >> 3] |= bit << np.uint8(7 - (pos & 7))
    return codes


def unpack2(codes2, D: int, B2: int) -> np.ndarray:
    """j int32 (N, D) of residual rows."""
    codes2 = np.ascontiguousarray(codes2, dtype=np.uint8)
    assert codes2.shape[1] == (D * B2 + 7) // 8
    j = np.zeros((codes2.shape[0], D), dtype=np.int32)
    for t in range(D):
        for b in range(B2):
            pos = t * B2 + b
            bit = (codes2[:, pos >> 3] >> np.uint8(7 - (pos & 7))) & 1
            j[:, t] |= bit.astype(np.int32) << (B2 - 1 - b)
    return j


def encode2(X, mu, B1: int, B2: int):
    """(codes1, codes2)."""
    idx, lo, delta, j = quantize2(X, mu, B1, B2)
    return LR.pack(idx, lo, delta, B1), pack2(j, B2)


def decode2(codes1, codes2, mu, B1: int, B2: int) -> np.ndarray:
    mu = np.asarray(mu, dtype=F32)
    D = mu.shape[0]
    idx, lo, delta = LR.unpack(codes1, D, B1)
    j = unpack2(codes2, D, B2)
    lo2 = F32(-0.5) * delta
    with np.errstate(under="ignore"):
        delta2 = delta / F32((1 << B2) - 1)
        a = lo[:, None] + (idx.astype(F32) * delta[:, None])
        b = lo2[:, None] + (j.astype(F32) * delta2[:, None])
        out = (a + b) + mu[None, :]
    assert a.dtype == b.dtype == out.dtype == F32
    return out


def padding_bits2(codes2, D: int, B2: int) -> np.ndarray:
    """The bits of the last residual byte past D B2 (all must be 0), per row."""
    spare = codes2.shape[1] * 8 - D * B2
    return codes2[:, -1] & np.uint8((1 << spare) - 1)


# planted half-to-even ties with mu = 0 and B1 = 2: B2 -> (leading values, their idx, their j).
# min and max of the row are the first and last leading values, so delta = max / 3 = L2 and
# delta2 = 1 exactly: the level-2 quotients 7.5, 8.5, ... / 127.5, 128.5, ... are ties.
TIES = {
    4: ([0, 1, 2, 3, 4, 7, 8, 13, 14, 45], [0, 0, 0, 0, 0, 0, 1, 1, 1, 3], [8, 8, 10, 10, 12, 14, 0, 6, 6, 8]),
    8: ([0, 1, 2, 127, 128, 254, 765], [0, 0, 0, 0, 1, 1, 3], [128, 128, 130, 254, 0, 126, 128]),
}
TIE_B1, TIE_FILL = 2, 3.25  # the fill is interior and not a tie


def tie_row(B2: int, D: int):
    """(row float32 (D,), expected leading idx, expected leading j); D at least the lead's length."""
    lead, idx, j = TIES[B2]
    row = np.full(D, TIE_FILL, dtype=F32)
    row[:len(lead)] = lead
    return row, idx, j


# ------------------------------------------------------------------------------ the cases
@functools.lru_cache(maxsize=None)
def case(name: str) -> dict:
    """One case, computed once and left unchanged: the inputs of its _lvq_rule case, mu (numpy's
    float32 column mean, which the planted row equals), and the rule's fields, rows and reconstruction."""
    src, B1, B2 = CASES[name]
    X, Q, planted = LR.inputs(src)
    mu = X.mean(axis=0)
    assert mu.dtype == F32 and np.array_equal(X[planted], mu)
    idx, lo, delta, j = quantize2(X, mu, B1, B2)
    codes1, codes2 = LR.pack(idx, lo, delta, B1), pack2(j, B2)
    for a in (X, Q, mu, idx, j, codes1, codes2):
        a.setflags(write=False)
    rec = decode2(codes1, codes2, mu, B1, B2)
    rec.setflags(write=False)
    return dict(name=name, src=src, B1=B1, B2=B2, N=X.shape[0], D=X.shape[1], X=X, Q=Q, planted=planted, mu=mu,
                idx=idx, lo=lo, delta=delta, j=j, codes1=codes1, codes2=codes2, rec=rec, k=LR.CASES[src]["k"])
