"""An arena with guard bands: every buffer of a raw libmivq call carved from one allocation.

The library's contract (include/mivq.h) is that every buffer is the caller's and has exactly the
documented size.  torch.empty cannot test that: the caching allocator pads each request and packs
small blocks side by side, so a store a few bytes past an output lands in memory the process
owns and nothing notices.  Here every pointer of a call is a view into one uint8 tensor filled
with 0xA5, with GUARD bytes of untouched poison on both sides of each view, and
``Arena.violations()`` lists every guard that no longer holds 0xA5, with the distance of the first
changed byte from the buffer: what is needed to find the store.

Sizes are conditions, not measurements: the widest store a wave issues is 64 lanes x 16 B = 1 KiB
and the longest row in the cases of the bounds tests is 12 KiB, so 64 KiB of guard catches an
overrun of several rows, and the 1 MiB TAIL that stays free after the last carve keeps a larger one
inside memory the test owns.  Works on CPU tensors too (tests/test_guard_cpu.py).
"""

from __future__ import annotations

import ctypes
from typing import List, NamedTuple, Optional, Tuple

import numpy as np
import torch

POISON = 0xA5
GUARD = 64 * 1024
TAIL = 1024 * 1024

_DTYPES = {
    "uint8": torch.uint8, "int8": torch.int8, "int16": torch.int16, "int32": torch.int32, "int64": torch.int64,
    "float16": torch.float16, "float32": torch.float32, "float64": torch.float64,
}


class Carve(NamedTuple):
    name: str
    start: int   # offset of the view's first byte in the arena
    nbytes: int
    view: torch.Tensor


def arena_bytes(sizes, align: int = 256) -> int:
    """An arena size that holds carves of the given byte counts at alignments up to `align`."""
    return sum(int(s) + 2 * GUARD + 2 * align + 256 for s in sizes) + TAIL + align + 4096


class Arena:
    def __init__(self, device, nbytes: int):
        self.buf = torch.full((int(nbytes),), POISON, dtype=torch.uint8, device=device)
        self.base = self.buf.data_ptr()
        self.carves: List[Carve] = []
        self._end = 0  # first byte past the last carve's trailing guard

    def carve(self, name: str, nbytes: int, align: int = 256, skew: int = 0, fill=None) -> torch.Tensor:
        """A view of exactly `nbytes` bytes starting `skew` bytes past an `align`-aligned address,
        with GUARD untouched bytes before and after it.  fill: a byte value, or a tensor / array
        of nbytes bytes to copy in; None leaves the poison."""
        nbytes, align, skew = int(nbytes), int(align), int(skew)
        if nbytes < 0 or align < 1 or skew < 0:
            raise ValueError(f"carve {name!r}: bad nbytes={nbytes} align={align} skew={skew}")
        if any(c.name == name for c in self.carves):
            raise ValueError(f"carve {name!r}: name already used")
        addr = self.base + self._end + GUARD
        addr = (addr + align - 1) // align * align + skew
        start = addr - self.base
        end = start + nbytes + GUARD
        if end + TAIL > self.buf.numel():
            raise ValueError(f"carve {name!r}: {nbytes} bytes at {start} would leave less than {TAIL} bytes free "
                             f"after it in an arena of {self.buf.numel()}")
        view = self.buf[start:start + nbytes]
        if fill is not None:
            if isinstance(fill, int):
                view.fill_(fill)
            else:
                if isinstance(fill, np.ndarray):
                    fill = torch.from_numpy(np.ascontiguousarray(fill).reshape(-1).view(np.uint8))
                src = fill.contiguous().reshape(-1).view(torch.uint8)
                if src.numel() != nbytes:
                    raise ValueError(f"carve {name!r}: fill has {src.numel()} bytes, the carve {nbytes}")
                view.copy_(src)
        self.carves.append(Carve(name, start, nbytes, view))
        self._end = end
        return view

    def ptr(self, name: str):
        """The pointer argument of carve `name` (valid for a zero-byte carve too, whose tensor view
        has no data pointer of its own)."""
        for c in self.carves:
            if c.name == name:
                return ctypes.c_void_p(self.base + c.start)
        raise KeyError(name)

    def violations(self) -> List[Tuple[str, str, int, int]]:
        """(name, "before" | "after", distance, count) per guard that is no longer all poison:
        distance = bytes between the buffer and the nearest changed byte (0: the byte next to it),
        count = changed bytes in that guard.  Synchronize the device first."""
        out = []
        for c in self.carves:
            for side, lo in (("before", c.start - GUARD), ("after", c.start + c.nbytes)):
                bad = torch.nonzero(self.buf[lo:lo + GUARD] != POISON).reshape(-1)
                if bad.numel():
                    dist = (GUARD - 1 - int(bad[-1])) if side == "before" else int(bad[0])
                    out.append((c.name, side, dist, int(bad.numel())))
        # the free tail belongs to no carve; a store that jumped every guard shows here
        tail = torch.nonzero(self.buf[self._end:] != POISON).reshape(-1)
        if tail.numel():
            out.append(("<tail>", "after", int(tail[0]), int(tail.numel())))
        return out

    def assert_clean(self, what: str = "") -> None:
        v = self.violations()
        assert not v, f"{what}: stray writes: " + "; ".join(
            f"{cnt} byte(s) {side} buffer {name!r}, nearest {dist} B from it" for name, side, dist, cnt in v)


def typed(view: torch.Tensor, dtype: str, shape=None) -> torch.Tensor:
    """A `dtype` ("float32", "int32", ...) view of a carve; the carve must start at a multiple of
    the element size."""
    t = view.view(_DTYPES[dtype])
    return t if shape is None else t.reshape(shape)


def ptr(view: Optional[torch.Tensor]):
    """The pointer argument of a raw ctypes call (None -> NULL)."""
    return None if view is None else ctypes.c_void_p(view.data_ptr())


def to_numpy(view: torch.Tensor) -> np.ndarray:
    """The bytes of a carve as a host uint8 array (a copy)."""
    return view.detach().cpu().numpy().copy()
