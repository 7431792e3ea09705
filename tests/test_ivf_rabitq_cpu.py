"""CPU: the ABI and host logic of the IVF-RaBitQ entry points and of RaBitQIVFIndex (no GPU).

The device side (encode, estimator search over probed lists, the index end to end) is held to
the oracle in tests/test_ivf_rabitq_gpu.py.
"""

import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
SYMBOLS = ("mivq_ivf_rabitq_encode", "mivq_ivf_rabitq_search_workspace_bytes", "mivq_ivf_rabitq_search")
GIB = 1 << 30


def test_header_declares_the_ivf_rabitq_symbols():
    txt = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "mivq.h").read_text(), flags=re.S)
    names = set(re.findall(r"\b(mivq_[a-z0-9_]+)\s*\(", txt))
    from haag_vq import _native

    for s in SYMBOLS:
        assert s in names, s
        assert s in _native.SIGNATURES, s
        assert hasattr(_native.load_library(), s), s
    assert "#define MIVQ_ABI_VERSION 2" in txt  # symbols were only added


def test_workspace_query_needs_no_gpu():
    from haag_vq import _native

    fn = _native.load_library().mivq_ivf_rabitq_search_workspace_bytes
    # (nq, n, nlist, nprobe, d, k)
    assert fn(100, 10_000, 16, 4, 64, 10) > 0
    assert fn(100, 10_000, 16, 4, 0, 10) == 0 and fn(100, 10_000, 16, 4, -3, 10) == 0   # d <= 0
    assert fn(100, 10_000, 16, 4, 64, 0) == 0 and fn(100, 10_000, 16, 4, 64, -1) == 0   # k <= 0
    assert fn(100, 10_000, 16, 0, 64, 10) == 0 and fn(100, 10_000, 16, -2, 64, 10) == 0  # nprobe <= 0
    assert fn(100, 10_000, 0, 4, 64, 10) == 0 and fn(-1, 10_000, 16, 4, 64, 10) == 0
    # queries are processed in chunks: unchunked, the pair rows alone are 655 MB at this shape
    # and the k = 256 partial lists 1.3 GB
    for k in (10, 256):
        nb = fn(10_000, 10_000_000, 4096, 64, 1024, k)
        print(f"\n[ivf-rabitq] workspace at nq 10000, n 10M, nlist 4096, nprobe 64, d 1024, k {k}: {nb / 2**20:.1f} MiB")
        assert 0 < nb <= GIB
    # sized on shape alone: the number of stored rows does not enter
    assert fn(100, 10, 16, 4, 64, 10) == fn(100, 10_000_000, 16, 4, 64, 10)


def test_bad_arguments_are_rejected_before_any_hip_call():
    """Null pointers, no GPU: validation comes first."""
    from haag_vq import _native

    lib = _native.load_library()

    def search(nq=4, d=64, nlist=16, nprobe=4, qb=4, metric=1, k=10):
        return lib.mivq_ivf_rabitq_search(None, nq, d, None, nlist, None, nprobe, None, None, None, qb, metric, k,
                                          None, 0, None, None, None)

    assert search(k=300) == _native.MIVQ_ERR_UNSUPPORTED
    with pytest.raises(ValueError, match="k=300"):
        _native._raise(_native.MIVQ_ERR_UNSUPPORTED)
    assert search(nlist=0) == _native.MIVQ_ERR_INVALID
    assert search(d=0) == _native.MIVQ_ERR_INVALID
    assert search(nprobe=0) == _native.MIVQ_ERR_INVALID
    assert search(nq=-1) == _native.MIVQ_ERR_INVALID
    assert search(qb=9) == _native.MIVQ_ERR_UNSUPPORTED
    assert search(metric=7) == _native.MIVQ_ERR_UNSUPPORTED
    assert search() == _native.MIVQ_ERR_INVALID and b"null pointer" in lib.mivq_last_error()
    assert search(nq=0) == _native.MIVQ_OK  # nothing to do

    def encode(n=4, d=64, nlist=16, metric=1):
        return lib.mivq_ivf_rabitq_encode(None, n, d, None, nlist, None, metric, None, None)

    assert encode(d=0) == _native.MIVQ_ERR_INVALID
    assert encode(n=-1) == _native.MIVQ_ERR_INVALID
    assert encode(nlist=0) == _native.MIVQ_ERR_INVALID
    assert encode(metric=5) == _native.MIVQ_ERR_UNSUPPORTED
    assert encode() == _native.MIVQ_ERR_INVALID and b"null pointer" in lib.mivq_last_error()
    assert encode(n=0) == _native.MIVQ_OK


def test_index_host_logic():
    from haag_vq.methods.base_search_index import BaseSearchIndex
    from haag_vq.methods.search import RaBitQIVFIndex

    idx = RaBitQIVFIndex()
    assert isinstance(idx, BaseSearchIndex)
    assert (idx._nlist, idx._nprobe, idx._qb) == (256, 64, 4)
    for qb in (9, -1):
        with pytest.raises(ValueError, match="qb"):
            RaBitQIVFIndex(qb=qb)
    assert RaBitQIVFIndex(qb=0)._qb == 0 and RaBitQIVFIndex(qb=8)._qb == 8
    Q = np.zeros((2, 8), np.float32)
    with pytest.raises(RuntimeError, match="fit"):
        idx.search(Q, 3)
    with pytest.raises(RuntimeError, match="fit"):
        idx.search_with_scores(Q, 3)
    with pytest.raises(RuntimeError, match="fit"):
        idx.search_device(Q, 3)
    assert idx.memory_footprint() == 0 and idx.ntotal == 0
    assert idx.reconstruction_mse(Q) is None


def test_save_before_fit_raises(tmp_path):
    from haag_vq.methods.search import RaBitQIVFIndex

    with pytest.raises(RuntimeError, match="fit"):
        RaBitQIVFIndex().save(tmp_path / "unfit.npz")
    assert not (tmp_path / "unfit.npz").exists()

