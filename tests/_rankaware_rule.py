"""The rank-aware quantizer restated in numpy, its cases and the bounds its tests use.

A *state* is what compress / decompress need and nothing else: ``mu`` (D,), ``V`` (D, D), the
widths ``bits`` (D,), one ascending level table per dimension ``cb`` (2 ** bits[d] levels), the
bit position ``pos`` of every field in the code row (MSB-first, bit p is bit 7 - p % 8 of byte
p // 8) and the row's ``code_size``.  Dense and whole-byte packings differ only in ``pos``.

  project     Y = (X - mu) . V, fp64 in a fixed summation order (_search_rule.matmul_seq)
  indices     idx[i, d] = #{ j : 0.5 (cb[d][j] + cb[d][j + 1]) < Y[i, d] }   (0 for width 0)
  pack        idx[i, d] in bits[d] bits, MSB first, from bit pos[d]; all other bits 0
  decompress  f32((cb[d][idx[i, d]])_d . V^T + mu), the product in the same fixed order

The library's fp64 GEMM and numpy's BLAS sum the D terms of a projection in other orders, so
indices are compared under ``tie_problems`` and decoded rows under ``decode_slack``.
"""

from __future__ import annotations

import hashlib
from types import SimpleNamespace

import numpy as np

import _search_rule as SR

PACKINGS = ("dense", "ffd")
GOLDEN = "rankaware_golden.npz"
TIE_CAP = 1e-3      # share of the N * D indices that may sit on a tie
U = 2.0 ** -53      # fp64 unit roundoff

# name -> shape, quantizer arguments, and the draw (changed when the generator refuses a case).
# decay: the ratio between the largest and the smallest standard deviation of the spectrum.
CASES = {
    "w08": dict(N=512, D=64, avg_bits=4.0, alpha=0.5, max_bits=8, decay=1e-3, draw=0),     # widths 0..8
    "mse100": dict(N=300, D=100, avg_bits=2.0, alpha=0.0, max_bits=8, decay=3e-2, draw=0),  # D % 32 != 0
    "odd37": dict(N=200, D=37, avg_bits=3.0, alpha=1.0, max_bits=8, decay=1e-2, draw=0),    # odd D
    "all8": dict(N=130, D=32, avg_bits=8.0, alpha=1.0, max_bits=8, decay=1e-1, draw=0),     # every width 8
    "sparse48": dict(N=200, D=48, avg_bits=0.5, alpha=1.0, max_bits=8, decay=1e-2, draw=0),  # most widths 0
    "cap3": dict(N=200, D=64, avg_bits=2.5, alpha=1.0, max_bits=3, decay=1e-2, draw=0),     # cap below 8
}
FIT_CASE = "cap3"   # max_bits <= 5: the N(0,1) Lloyd tables of a fit take well under a second


def sha(a) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def gaussian_rows(N: int, D: int, decay: float, draw: int) -> np.ndarray:
    """(N, D) f32: Gaussian rows with a geometric spectrum, rotated by a seeded orthogonal
    matrix, plus an offset."""
    rng = np.random.default_rng([N, D, draw])
    std = 2.0 * decay ** (np.arange(D) / max(D - 1, 1))
    R, _ = np.linalg.qr(rng.standard_normal((D, D)))
    X = (rng.standard_normal((N, D)) * std) @ R.T + rng.standard_normal(D)
    return np.ascontiguousarray(X, dtype=np.float32)


def inputs(name: str) -> np.ndarray:
    c = CASES[name]
    return gaussian_rows(c["N"], c["D"], c["decay"], c["draw"])


def load_golden(golden_dir) -> dict:
    with np.load(golden_dir / GOLDEN, allow_pickle=False) as f:
        return {k: f[k] for k in f.files}


def fixture_quantizer(z, name: str, packing: str):
    """The library's RankAwareQuantizer holding the fixture's fitted state (needs no device)."""
    from haag_vq.methods.rank_aware_quantization import RankAwareQuantizer

    c = CASES[name]
    q = RankAwareQuantizer(c["avg_bits"], alpha=c["alpha"], max_bits=c["max_bits"], packing=packing)
    q.mu, q.V, q.var, q.bits = z[f"{name}_mu"], z[f"{name}_V"], z[f"{name}_var"], z[f"{name}_bits"]
    q.D = c["D"]
    q.cb = split_cb(z[f"{name}_cb"], q.bits)
    q._levels = [z["levels"][2 ** b - 1:2 ** (b + 1) - 1] for b in range(c["max_bits"] + 1)]
    q._Dg = z["Dg"][:c["max_bits"] + 1]
    q._layout()
    return q


# ------------------------------------------------------------------ states
def make_state(mu, V, bits, cb, pos, code_size, packing="dense"):
    bits = np.asarray(bits, dtype=np.int64)
    return SimpleNamespace(mu=np.asarray(mu, np.float64), V=np.asarray(V, np.float64), bits=bits,
                           cb=[np.asarray(c, np.float64) for c in cb], pos=np.asarray(pos, np.int64),
                           code_size=int(code_size), packing=packing, D=int(bits.shape[0]))


def split_cb(flat, bits):
    ends = np.cumsum(2 ** np.asarray(bits, dtype=np.int64))
    return [np.asarray(flat[e - 2 ** b:e], np.float64) for e, b in zip(ends, bits)]


def fixture_state(z, name: str, packing: str):
    """The reference's fitted state of case `name`, as the fixture stores it."""
    bits = z[f"{name}_bits"]
    if packing == "ffd":
        pos = 8 * z[f"{name}_ffd_byte_idx"] + z[f"{name}_ffd_bit_off"]
    else:
        pos = z[f"{name}_offsets"][:-1]
    pos = np.where(bits > 0, pos, 0)
    return make_state(z[f"{name}_mu"], z[f"{name}_V"], bits, split_cb(z[f"{name}_cb"], bits), pos,
                      int(z[f"{name}_{packing}_code_size"]), packing)


def dense_positions(bits):
    bits = np.asarray(bits, dtype=np.int64)
    return np.concatenate(([0], np.cumsum(bits)))[:-1], (int(bits.sum()) + 7) // 8


def byte_positions(bits):
    """A whole-byte layout by next fit in index order (not FFD: the kernels take any positions)."""
    pos, byte, used = [], 0, 0
    for w in np.asarray(bits, dtype=np.int64):
        if w and used + w > 8:
            byte, used = byte + 1, 0
        pos.append(8 * byte + used if w else 0)
        used += int(w)
    return np.array(pos, dtype=np.int64), byte + (1 if used else 0)


def synthetic_state(bits, packing: str, seed: int, pos=None, code_size=None):
    """Seeded mu, an orthogonal V and strictly ascending level tables for the given widths."""
    bits = np.asarray(bits, dtype=np.int64)
    D = bits.shape[0]
    rng = np.random.default_rng([D, seed])
    V, _ = np.linalg.qr(rng.standard_normal((D, D)))
    cb = [np.sort(rng.standard_normal(2 ** b)) * (1.0 + d % 7) if b else np.zeros(1) for d, b in enumerate(bits)]
    if pos is None:
        pos, code_size = dense_positions(bits) if packing == "dense" else byte_positions(bits)
    return make_state(rng.standard_normal(D), V, bits, cb, pos, code_size, packing)


# ------------------------------------------------------------------ the rule
def boundaries(st, d: int) -> np.ndarray:
    c = st.cb[d]
    return 0.5 * (c[:-1] + c[1:])


def project(X, st) -> np.ndarray:
    return SR.matmul_seq(np.asarray(X, np.float64) - st.mu, st.V)


def indices(Y, st) -> np.ndarray:
    idx = np.zeros(Y.shape, dtype=np.int64)
    for d in np.flatnonzero(st.bits):
        idx[:, d] = np.searchsorted(boundaries(st, d), Y[:, d])
    return idx


def pack(idx, st) -> np.ndarray:
    bitmat = np.zeros((idx.shape[0], 8 * st.code_size), dtype=np.uint8)
    for d in np.flatnonzero(st.bits):
        w, p = int(st.bits[d]), int(st.pos[d])
        for k in range(w):
            bitmat[:, p + k] = (idx[:, d] >> (w - 1 - k)) & 1
    return np.packbits(bitmat, axis=1)


def unpack(codes, st) -> np.ndarray:
    """(N, D) indices of code rows; bits outside the fields are not looked at."""
    bitmat = np.unpackbits(np.ascontiguousarray(codes, dtype=np.uint8), axis=1).astype(np.int64)
    idx = np.zeros((bitmat.shape[0], st.D), dtype=np.int64)
    for d in np.flatnonzero(st.bits):
        w, p = int(st.bits[d]), int(st.pos[d])
        for k in range(w):
            idx[:, d] = (idx[:, d] << 1) | bitmat[:, p + k]
    return idx


def lookup(idx, st) -> np.ndarray:
    return np.stack([st.cb[d][idx[:, d]] for d in range(st.D)], axis=1)


def compress(X, st) -> np.ndarray:
    return pack(indices(project(X, st), st), st)


def decompress(codes, st) -> np.ndarray:
    return (SR.matmul_seq(lookup(unpack(codes, st), st), st.V.T) + st.mu).astype(np.float32)


def field_mask(st) -> np.ndarray:
    """(code_size,) u8: the bits of a row that belong to a field."""
    bitmat = np.zeros(8 * st.code_size, dtype=np.uint8)
    for d in np.flatnonzero(st.bits):
        bitmat[int(st.pos[d]):int(st.pos[d] + st.bits[d])] = 1
    return np.packbits(bitmat)


# ------------------------------------------------------------------ bounds
def tie_slack(X, st) -> np.ndarray:
    """(N, D): 2 (D + 2) 2^-53 ||x_i - mu|| ||V[:, d]||: twice the worst-case rounding of a
    length-D fp64 dot product in any order, once for each of the two sums compared."""
    xc = np.asarray(X, np.float64) - st.mu
    return 2.0 * (st.D + 2) * U * np.linalg.norm(xc, axis=1)[:, None] * np.linalg.norm(st.V, axis=0)[None, :]


def tie_problems(got_idx, want_idx, Y, X, st, cap: float = TIE_CAP) -> list:
    """Why `got_idx` is not `want_idx` up to ties: every differing index must differ by exactly
    one and Y must lie within tie_slack of the boundary between the two levels; at most `cap` of
    all indices may differ.  Y is either side's projection."""
    problems = []
    ii, dd = np.nonzero(got_idx != want_idx)
    if len(ii) > cap * got_idx.size:
        problems.append(f"{len(ii)} of {got_idx.size} indices differ (cap {cap})")
    if len(ii):
        slack = tie_slack(X, st)
    for i, d in zip(ii, dd):
        g, w = int(got_idx[i, d]), int(want_idx[i, d])
        if abs(g - w) != 1:
            problems.append(f"[{i},{d}] index {g} vs {w}")
            continue
        gap = abs(Y[i, d] - boundaries(st, d)[min(g, w)])
        if not gap <= slack[i, d]:
            problems.append(f"[{i},{d}] index {g} vs {w}: {gap:.3e} from the boundary, slack {slack[i, d]:.3e}")
    return problems


def decode_slack(rec, Yhat, D: int) -> np.ndarray:
    """(N, D): 2^-23 |rec| + (D + 2) 2^-52 ||yhat_i||: one f32 ulp where the two fp64 sums fall
    either side of an f32 rounding point, plus the fp64 sums' own difference."""
    return 2.0 ** -23 * np.abs(rec) + (D + 2) * 2.0 ** -52 * np.linalg.norm(Yhat, axis=1)[:, None]
