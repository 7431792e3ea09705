"""Whole-byte packing of per-dimension bit fields by first-fit decreasing (host, numpy).

Every dimension's ``b_d``-bit code (``b_d <= byte_cap``) sits wholly inside one byte, so a
decoder reads one byte per field.  The layout is the reference's (``methods/ffd_packing.py``),
element for element: dimensions in order of decreasing width (equal widths by index); for
8-bit bytes the width-4 dimensions are moved behind the width-3 ones (a 4 placed before the
3s takes a 3 and wastes a bit; 4 + 4 fills a byte exactly, so the 4s lose nothing by waiting);
each dimension goes to the first byte with room, at that byte's next free bit from the MSB.

These are layout tools that run once per fit; the per-row packing of ``RankAwareQuantizer`` runs
on the device (``mivq_rankaware_quantize``), which takes the layout as bit positions.
"""

from __future__ import annotations

from typing import Tuple

import numpy as np


def byte_cap_minus(width: int, offset: int, byte_cap: int = 8) -> int:
    """Shift between a ``width``-bit field at ``offset`` bits from the MSB of a ``byte_cap``-bit
    byte and the byte's LSB."""
    return byte_cap - offset - width


def ffd_layout(bits_per_dim, byte_cap: int = 8) -> Tuple[np.ndarray, np.ndarray, int]:
    """(byte_idx (D,), bit_off (D,), n_bytes): the byte of each dimension and its offset from
    that byte's MSB, -1 / -1 for a zero-width dimension."""
    widths = np.asarray(bits_per_dim, dtype=np.int64)
    if np.any(widths > byte_cap) or np.any(widths < 0):
        raise ValueError(f"bits_per_dim must be in [0, {byte_cap}]")
    D = widths.shape[0]
    byte_idx = np.full(D, -1, dtype=np.int64)
    bit_off = np.full(D, -1, dtype=np.int64)
    # stable sort by -width: decreasing width, equal widths in index order
    order = [int(d) for d in np.argsort(-widths, kind="stable") if widths[d] > 0]
    if byte_cap == 8:
        fours = [d for d in order if widths[d] == 4]
        if fours:
            wide = [d for d in order if widths[d] > 4 or widths[d] == 3]
            narrow = [d for d in order if widths[d] <= 2]
            order = wide + fours + narrow
    free = []  # free bits of each open byte
    for d in order:
        w = int(widths[d])
        for b, room in enumerate(free):
            if room >= w:
                break
        else:
            b = len(free)
            free.append(byte_cap)
        byte_idx[d] = b
        bit_off[d] = byte_cap - free[b]
        free[b] -= w
    return byte_idx, bit_off, len(free)


def ffd_encode(codes, bits_per_dim, byte_idx, bit_off, n_bytes: int, byte_cap: int = 8) -> np.ndarray:
    """(N, D) indices (column d below 2^b_d) -> (N, n_bytes) uint8 rows of the layout."""
    codes = np.asarray(codes, dtype=np.uint64)
    widths = np.asarray(bits_per_dim, dtype=np.int64)
    out = np.zeros((codes.shape[0], n_bytes), dtype=np.uint8)
    for d in np.flatnonzero(widths):
        shift = byte_cap_minus(int(widths[d]), int(bit_off[d]), byte_cap)
        out[:, byte_idx[d]] |= codes[:, d].astype(np.uint8) << shift
    return out


def ffd_decode(packed, bits_per_dim, byte_idx, bit_off, D: int, byte_cap: int = 8) -> np.ndarray:
    """Inverse of ffd_encode: (N, D) int64 indices, 0 for zero-width dimensions."""
    packed = np.asarray(packed, dtype=np.uint8)
    widths = np.asarray(bits_per_dim, dtype=np.int64)
    codes = np.zeros((packed.shape[0], D), dtype=np.int64)
    for d in range(D):
        w = int(widths[d])
        if w == 0:
            continue
        shift = byte_cap_minus(w, int(bit_off[d]), byte_cap)
        codes[:, d] = (packed[:, byte_idx[d]].astype(np.int64) >> shift) & ((1 << w) - 1)
    return codes
