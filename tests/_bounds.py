"""The buffer-contract cases of every device-pointer entry point of include/mivq.h, and the
runner that places one case in a guarded arena (tests/_guard.py).

A case is one entry point at one shape on one dispatch branch.  Its builder returns a ``Call``:
the ctypes argument list with every pointer argument as a ``Buf`` (role in / out / inout, its
exact documented size, an optional misalignment) or a ``Ws`` (the entry's size query and its
arguments), and ``expect``: the reference outputs, computed on the host from the rule modules
(tests/_*_rule.py) and the oracle.  Builders need no GPU (the CPU tests build them for the
coverage and workspace-refusal checks); ``expect`` and ``late`` inputs are evaluated on the GPU
machine only.

The case tables live in tests/_bounds_codec.py and tests/_bounds_search.py; importing this
module's ``all_cases()`` loads both.
"""

from __future__ import annotations

import ctypes
from types import SimpleNamespace
from typing import Callable, Dict, List, Optional

import numpy as np

from _guard import POISON, Arena, arena_bytes, to_numpy

OK = 0
ERR_WORKSPACE = -4
NO_ID = 0xFFFFFFFF
F32 = np.float32
EMPTY_BYTES = 256  # what an output of an empty call gets, so that there are bytes to watch


class Buf:
    """A pointer argument.  data: the bytes uploaded (in / inout); nbytes: the size of a pure
    output; late(ctx): input bytes that only the library can make (a prep buffer), with nbytes;
    host: a host pointer (not carved)."""

    def __init__(self, name: str, role: str, data=None, nbytes: Optional[int] = None, skew: int = 0,
                 align: int = 256, host: bool = False, late: Optional[Callable] = None):
        assert role in ("in", "out", "inout")
        self.name, self.role, self.skew, self.align, self.host, self.late = name, role, skew, align, host, late
        self.data = None if data is None else np.ascontiguousarray(data)
        if self.data is not None:
            nbytes = self.data.nbytes
        assert nbytes is not None and (role == "out" or self.data is not None or late is not None), name
        self.nbytes = int(nbytes)


def In(name, data, skew=0, **kw):
    return Buf(name, "in", data=data, skew=skew, **kw)


def Out(name, nbytes, skew=0, **kw):
    return Buf(name, "out", nbytes=nbytes, skew=skew, **kw)


def InOut(name, data, **kw):
    return Buf(name, "inout", data=data, **kw)


def Host(name, data):
    return Buf(name, "in", data=data, host=True)


class Ws:
    """The (workspace, workspace_bytes) argument pair: exactly query(*qargs) bytes, or `doc`
    bytes where the query returns 0."""

    def __init__(self, query: str, *qargs, doc: int = 0):
        self.query, self.qargs, self.doc = query, qargs, doc


class Call:
    def __init__(self, args: list, expect: Optional[Callable] = None, check: Optional[Dict[str, Callable]] = None,
                 empty_expect: Optional[Dict[str, np.ndarray]] = None):
        self.args, self.expect, self.check, self.empty_expect = args, expect, check or {}, empty_expect or {}

    def bufs(self) -> List[Buf]:
        return [a for a in self.args if isinstance(a, Buf)]

    def ws(self) -> Optional[Ws]:
        w = [a for a in self.args if isinstance(a, Ws)]
        assert len(w) <= 1
        return w[0] if w else None


class Case:
    def __init__(self, entry: str, cid: str, tags: frozenset, build: Callable):
        self.entry, self.id, self.tags, self.build = entry, cid, tags, build

    def __repr__(self):
        return f"{self.entry}[{self.id}]"


CASES: List[Case] = []

# tags: what a case is there for (the coverage check asks for one of each per entry point)
RAGGED, EDGE, EMPTY = "ragged", "edge", "empty"


def add(entry: str, cid: str, tags, build: Callable) -> None:
    """Register a case; build(O) -> Call, O the oracle module."""
    tags = frozenset([tags] if isinstance(tags, str) else tags)
    assert not any(c.entry == entry and c.id == cid for c in CASES), (entry, cid)
    CASES.append(Case(entry, cid, tags, build))


def all_cases() -> List[Case]:
    import _bounds_codec  # noqa: F401  (registers its cases)
    import _bounds_search  # noqa: F401

    return CASES


def rng(*seed) -> np.random.Generator:
    return np.random.default_rng([int(s) for s in seed])


def rows(n: int, d: int, *seed) -> np.ndarray:
    return rng(n, d, *seed).standard_normal((n, d)).astype(F32)


def int_rows(n: int, d: int, *seed, lim: int = 8, dtype=F32) -> np.ndarray:
    """Small integers: every product and sum of a d <= 4096 chain is exact in fp32, whatever the order."""
    return rng(n, d, *seed).integers(-lim, lim + 1, (n, d)).astype(dtype)


def pad_topk(dd, ii, k: int):
    """(nq, kk <= k) lists padded to k with the missing-slot values."""
    nq = dd.shape[0]
    D = np.full((nq, k), np.inf, F32)
    I = np.full((nq, k), NO_ID, np.uint32)
    D[:, :dd.shape[1]] = dd
    I[:, :ii.shape[1]] = ii
    return D, I


def sentinel(nq: int, k: int):
    return {"dists": np.full((nq, k), np.inf, F32), "ids": np.full((nq, k), NO_ID, np.uint32)}


# ------------------------------------------------------------------------------ the runner
def _as_bytes(a) -> np.ndarray:
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


def ws_bytes(lib, w: Ws) -> int:
    need = int(getattr(lib, w.query)(*w.qargs))
    return need if need > 0 else int(w.doc)


def _compare(name: str, got: np.ndarray, want, what: str) -> None:
    want = np.ascontiguousarray(want)
    assert got.nbytes == want.nbytes, f"{what}: output {name!r} has {got.nbytes} bytes, the reference {want.nbytes}"
    np.testing.assert_array_equal(got.view(want.dtype).reshape(want.shape), want, err_msg=f"{what}: output {name!r}")


def run_case(case: Case, dev, O) -> None:
    """P1..P4 of a case with rows, P5 of an empty one (the module docstring of
    tests/test_bounds_codec_gpu.py states them)."""
    import torch
    from haag_vq import _native

    lib = _native.load_library()
    call = case.build(O)
    what = repr(case)
    empty = EMPTY in case.tags
    ctx = SimpleNamespace(O=O, dev=dev, N=_native, lib=lib,
                          t=lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev))
    data = {}
    for b in call.bufs():
        if b.role != "out" and not b.host:
            data[b.name] = _as_bytes(b.late(ctx) if b.late is not None else b.data)
            assert data[b.name].nbytes == b.nbytes, (what, b.name)
    w = call.ws()
    wsn = ws_bytes(lib, w) if w is not None else 0
    outsize = {b.name: (max(b.nbytes, EMPTY_BYTES) if empty else b.nbytes) for b in call.bufs() if b.role == "out"}
    sizes = [b.nbytes for b in call.bufs() if not b.host and b.role != "out"] + list(outsize.values()) + [wsn]
    runs = {}
    for fill in ((POISON,) if empty else (0x00, 0xFF)):
        arena = Arena(dev, arena_bytes(sizes))
        views, argv = {}, []
        for a in call.args:
            if isinstance(a, Buf):
                if a.host:
                    argv.append(a.data.ctypes.data_as(ctypes.c_void_p))
                    continue
                if a.role == "out":
                    views[a.name] = arena.carve(a.name, outsize[a.name], a.align, a.skew, fill=fill)
                else:
                    views[a.name] = arena.carve(a.name, a.nbytes, a.align, a.skew, fill=data[a.name])
                argv.append(arena.ptr(a.name))
            elif isinstance(a, Ws):
                arena.carve("workspace", wsn, 256, 0, fill=fill)
                argv += [arena.ptr("workspace"), wsn]
            else:
                argv.append(a)
        torch.cuda.synchronize()
        rc = getattr(lib, case.entry)(*argv)
        try:
            torch.cuda.synchronize()
        except RuntimeError as e:  # a device fault is sticky: nothing more may run on this GPU
            import pytest

            pytest.exit(f"{what}: the device faulted ({e}); no further GPU test is started", returncode=3)
        assert rc == OK, f"{what}: returned {rc}: {lib.mivq_last_error().decode(errors='replace')}"
        arena.assert_clean(what)  # P1
        for b in call.bufs():  # P2
            if b.role == "in" and not b.host:
                assert np.array_equal(to_numpy(views[b.name]), data[b.name]), f"{what}: input {b.name!r} was written"
        runs[fill] = {b.name: to_numpy(views[b.name]) for b in call.bufs() if b.role != "in"}
        del arena, views
    if empty:  # P5
        for name, got in runs[POISON].items():
            keep = data.get(name)  # an inout buffer keeps its data, a pure output its poison
            if name in call.empty_expect:
                want = _as_bytes(call.empty_expect[name])
                assert np.array_equal(got[:want.nbytes], want), f"{what}: {name!r} is not the documented empty result"
                got, keep = got[want.nbytes:], None if keep is None else keep[want.nbytes:]
            if keep is None:
                assert (got == POISON).all(), f"{what}: {int((got != POISON).sum())} byte(s) of {name!r} written"
            else:
                assert np.array_equal(got, keep), f"{what}: {name!r} changed"
        return
    for name in runs[0x00]:  # P3
        a, b = runs[0x00][name], runs[0xFF][name]
        if not np.array_equal(a, b):
            at = np.flatnonzero(a != b)
            raise AssertionError(f"{what}: output {name!r} depends on what the workspace / output held before: "
                                 f"{at.size} byte(s) differ, the first at byte {int(at[0])} of {a.size}")
    want = call.expect(ctx)  # P4
    assert set(want) == set(runs[0x00]), (what, sorted(want), sorted(runs[0x00]))
    for name, ref in want.items():
        if name in call.check:
            call.check[name](runs[0x00][name], ref, f"{what}: output {name!r}")
        else:
            _compare(name, runs[0x00][name], ref, what)


# ------------------------------------------------------------------------------ host-side refusal
def refusal_codes(case: Case, O, lib):
    """(need, rc with need - 1 bytes, rc with a null workspace of `need` bytes) of the case's
    entry point, every device pointer a fake non-null address: the workspace check is made on the
    host before any launch, so nothing is dereferenced."""
    call = case.build(O)
    w = call.ws()
    need = ws_bytes(lib, w)
    out = []
    for wp, wb in ((ctypes.c_void_p(0x7000000), need - 1), (None, need)):
        argv, fake = [], 0x1000000
        for a in call.args:
            if isinstance(a, Buf):
                if a.host:
                    argv.append(a.data.ctypes.data_as(ctypes.c_void_p))
                else:
                    fake += 0x100000
                    argv.append(ctypes.c_void_p(fake + a.skew))
            elif isinstance(a, Ws):
                argv += [wp, wb]
            else:
                argv.append(a)
        out.append(int(getattr(lib, case.entry)(*argv)))
    return need, out[0], out[1]
