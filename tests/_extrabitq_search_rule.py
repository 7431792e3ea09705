"""The Extended RaBitQ code search restated in numpy.

P is orthogonal and x_hat = (o_hat P^T) nrm + c, so for a query q

    ||q - x_hat||^2 = ||(q - c) P - y_hat||^2        <q, x_hat> = <q P, y_hat> + <q, c>

with y_hat = o_hat nrm in the rotated domain.  A code row is ceil(D B / 8) bytes of MSB-first
B-bit fields followed by two little-endian f32, nrm and t.  The library's reconstruction is

    o_hat_t = (levels[idx_t] / sqrt(D)) * (double)t        (mivq_extrabitq_dequantize)
    y_hat_t = (float)(o_hat_t * (double)nrm)

every step one IEEE fp64 operation, rounded to f32 once; the distances are the f32 chains of
_rankaware_search_rule over t ascending, against a = f32((q - c) P) (IP: f32(q P)).
"""

from __future__ import annotations

import numpy as np

import _rankaware_search_rule as RS
import _search_rule as SR


def code_size(D: int, B: int) -> int:
    return (D * B + 7) // 8 + 8


def unpack(codes, D: int, B: int):
    """(idx (N, D) int64, nrm (N,) f32, t (N,) f32) of code rows (N, code_size) u8."""
    codes = np.ascontiguousarray(codes, np.uint8)
    ib = (D * B + 7) // 8
    assert codes.ndim == 2 and codes.shape[1] == ib + 8
    bits = np.unpackbits(codes[:, :ib], axis=1)[:, :D * B].reshape(codes.shape[0], D, B).astype(np.int64)
    idx = (bits << np.arange(B - 1, -1, -1)).sum(axis=2)
    tr = np.ascontiguousarray(codes[:, ib:]).view("<f4")
    return idx, tr[:, 0].copy(), tr[:, 1].copy()


def pack(idx, nrm, t, B: int, pad_ones: bool = False) -> np.ndarray:
    """Code rows of the fields idx (N, D), nrm and t (N,); pad_ones sets the bits past D B."""
    idx = np.asarray(idx, np.int64)
    N, D = idx.shape
    bits = ((idx[:, :, None] >> np.arange(B - 1, -1, -1)) & 1).astype(np.uint8).reshape(N, D * B)
    pad = (-D * B) % 8
    bits = np.concatenate([bits, np.full((N, pad), 1 if pad_ones else 0, np.uint8)], axis=1)
    tr = np.stack([np.asarray(nrm, np.float32), np.asarray(t, np.float32)], axis=1).astype("<f4")
    return np.ascontiguousarray(np.concatenate([np.packbits(bits, axis=1), tr.view(np.uint8)], axis=1))


def o_hat(codes, levels, D: int, B: int) -> np.ndarray:
    """(N, D) fp64: the values mivq_extrabitq_dequantize writes."""
    idx, _, t = unpack(codes, D, B)
    return (np.asarray(levels, np.float64)[idx] / np.sqrt(np.float64(D))) * t.astype(np.float64)[:, None]


def y_hat(codes, levels, D: int, B: int) -> np.ndarray:
    """(N, D) f32: the reconstruction in the rotated domain the chains run over."""
    _, nrm, _ = unpack(codes, D, B)
    with np.errstate(over="ignore", invalid="ignore"):
        return (o_hat(codes, levels, D, B) * nrm.astype(np.float64)[:, None]).astype(np.float32)


def rotate(Q, c, P, metric: str = "l2") -> np.ndarray:
    """(nq, D) fp64: (Q - c) P for L2, Q P for IP, in a fixed summation order."""
    Q = np.asarray(Q, np.float64)
    return SR.matmul_seq(Q - np.asarray(c, np.float64) if metric == "l2" else Q, P)


def search(Q, codes, c, P, levels, B: int, k: int, metric: str = "l2"):
    """(ids uint32 (nq, k), dists f32 (nq, k)) as ExtendedRaBitQuantizer.search_codes returns them:
    squared L2 ascending, or inner products (chain + f32(<q, c>)) descending; ties to the smaller id."""
    D = np.asarray(P).shape[0]
    Yh = y_hat(codes, levels, D, B)
    A = rotate(Q, c, P, metric).astype(np.float32)
    ids = np.empty((len(A), k), np.uint32)
    dists = np.empty((len(A), k), np.float32)
    for j, a in enumerate(A):
        if metric == "l2":
            key = RS.chain_l2(a, Yh)
            order = RS.top_ids(key, k)
            dists[j] = key[order]
        else:
            key = -RS.chain_ip(a, Yh)
            order = RS.top_ids(key, k)
            qc = np.float32(np.asarray(Q[j], np.float64) @ np.asarray(c, np.float64))
            dists[j] = (-key[order] + qc).astype(np.float32)
        ids[j] = order
    return ids, dists
