"""CPU: the C ABI and the Python wrappers of the code-domain flat searches
(mivq_sq_flat_search / mivq_rabitq_flat_search) without a device: size queries, argument
validation before any HIP call, wrapper shape / dtype checks, header <-> ctypes table."""

import ctypes
import re
from pathlib import Path

import pytest
import torch

from haag_vq import _native

ROOT = Path(__file__).resolve().parents[1]
PAIRS = (("mivq_sq_flat_search", "mivq_sq_flat_search_workspace_bytes"),
         ("mivq_rabitq_flat_search", "mivq_rabitq_flat_search_workspace_bytes"))
P = ctypes.c_void_p(4096)  # a non-null pointer no validation path dereferences


def test_symbols_in_header_and_table():
    txt = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "mivq.h").read_text(), flags=re.S)
    declared = set(re.findall(r"\b(mivq_[a-z0-9_]+)\s*\(", txt))
    lib = _native.load_library()
    for pair in PAIRS:
        for name in pair:
            assert name in declared, name
            assert name in _native.SIGNATURES, name
            assert hasattr(lib, name), name
    assert lib.mivq_abi_version() == 2


@pytest.mark.parametrize("name", [p[1] for p in PAIRS])
def test_size_queries_need_no_gpu(name):
    fn = getattr(_native.load_library(), name)
    assert fn(1, 1000, 64, 10) > 0  # streaming scan
    assert fn(100, 100_000, 64, 10) > 0  # tiled
    # part lists / key blocks only: far below the decoded database, below even the SQ-8 codes
    assert 0 < fn(1000, 1_000_000, 3072, 10) < 1_000_000 * 3072
    assert 0 < fn(1, 1_000_000, 3072, 10) < 1 << 20
    for bad in ((0, 10, 8, 1), (1, 0, 8, 1), (1, 10, 0, 1), (1, 10, 8, 0), (-1, 10, 8, 1), (1, -5, 8, 1)):
        assert fn(*bad) == 0, bad


def _sq(nq=1, n=10, d=8, nbits=8, metric=1, k=1, id_offset=0, ptr=None, ws=None, wsb=0):
    lib = _native.load_library()
    return lib.mivq_sq_flat_search(ptr, nq, ptr, n, d, ptr, ptr, nbits, metric, k, id_offset, ws, wsb, ptr, ptr, None)


def _rq(nq=1, n=10, d=8, metric=1, k=1, id_offset=0, ptr=None, ws=None, wsb=0):
    lib = _native.load_library()
    return lib.mivq_rabitq_flat_search(ptr, nq, ptr, n, d, ptr, metric, k, id_offset, ws, wsb, ptr, ptr, None)


@pytest.mark.parametrize("call", [_sq, _rq], ids=["sq", "rabitq"])
def test_validation_before_any_hip_call(call):
    """Every argument error returns its code with all pointers null (nothing is launched)."""
    err = _native.load_library().mivq_last_error
    assert call(nq=-1) == _native.MIVQ_ERR_INVALID and b"bad sizes" in err()
    assert call(n=-1) == _native.MIVQ_ERR_INVALID
    assert call(d=0) == _native.MIVQ_ERR_INVALID
    assert call(k=0) == _native.MIVQ_ERR_INVALID
    assert call(k=257) == _native.MIVQ_ERR_UNSUPPORTED and b"k=257" in err()
    assert call(metric=7) == _native.MIVQ_ERR_UNSUPPORTED and b"metric 7" in err()
    assert call(d=1 << 20) == _native.MIVQ_ERR_UNSUPPORTED and b"too large for LDS" in err()
    assert call(id_offset=-1) == _native.MIVQ_ERR_INVALID and b"ids overflow" in err()
    assert call(n=10, id_offset=2 ** 32 - 1 - 9) == _native.MIVQ_ERR_INVALID and b"ids overflow" in err()
    assert call(nq=0) == _native.MIVQ_OK  # nothing to do, nothing dereferenced
    assert call() == _native.MIVQ_ERR_INVALID and b"null pointer" in err()  # outputs
    assert call(n=0) == _native.MIVQ_ERR_INVALID and b"null pointer" in err()
    # inputs present, workspace missing / too small
    assert call(ptr=P) == _native.MIVQ_ERR_WORKSPACE and b"workspace" in err()
    assert call(ptr=P, ws=P, wsb=16) == _native.MIVQ_ERR_WORKSPACE
    with pytest.raises(RuntimeError):
        _native._raise(_native.MIVQ_ERR_WORKSPACE)


def test_sq_validation_of_its_own_arguments():
    err = _native.load_library().mivq_last_error
    for nbits in (0, 1, 5, 12, 32):
        assert _sq(nbits=nbits) == _native.MIVQ_ERR_INVALID
        assert b"num_bits must be 4, 8, or 16" in err()
    with pytest.raises(ValueError):
        _native._raise(_native.MIVQ_ERR_INVALID)
    # 16-bit codes at an odd address
    lib = _native.load_library()
    odd = ctypes.c_void_p(4097)
    rc = lib.mivq_sq_flat_search(P, 1, odd, 10, 8, P, P, 16, 1, 1, 0, P, 1 << 20, P, P, None)
    assert rc == _native.MIVQ_ERR_INVALID and b"2-byte aligned" in err()


def test_wrappers_reject_wrong_codes():
    """Width and dtype of the codes are checked first, so the errors need no device."""
    q = torch.zeros((2, 10))
    lo = den = torch.zeros(10)
    u8 = lambda *s: torch.zeros(s, dtype=torch.uint8)  # noqa: E731
    with pytest.raises(ValueError, match=r"8-bit codes of d=10 must be \(n, 10\)"):
        _native.sq_flat_search(q, u8(5, 9), 10, lo, den, 8, 1)
    with pytest.raises(ValueError, match=r"4-bit codes of d=10 must be \(n, 5\)"):
        _native.sq_flat_search(q, u8(5, 10), 10, lo, den, 4, 1)
    with pytest.raises(ValueError, match="16-bit codes of d=10"):
        _native.sq_flat_search(q, u8(5, 10), 10, lo, den, 16, 1)
    with pytest.raises(ValueError, match="8-bit codes of d=10"):
        _native.sq_flat_search(q, torch.zeros((5, 10), dtype=torch.int16), 10, lo, den, 8, 1)
    with pytest.raises(ValueError, match="8-bit codes of d=10"):
        _native.sq_flat_search(q, u8(50), 10, lo, den, 8, 1)
    with pytest.raises(ValueError, match="num_bits must be 4, 8, or 16"):
        _native.sq_flat_search(q, u8(5, 10), 10, lo, den, 2, 1)
    with pytest.raises(ValueError, match="bytes per row, expected 10"):
        _native.rabitq_flat_search(q, u8(5, 9), 10, None, 1)
    with pytest.raises(ValueError, match="2-D uint8"):
        _native.rabitq_flat_search(q, torch.zeros((5, 10), dtype=torch.int8), 10, None, 1)
    with pytest.raises(ValueError, match="2-D uint8"):
        _native.rabitq_flat_search(q, u8(50), 10, None, 1)
