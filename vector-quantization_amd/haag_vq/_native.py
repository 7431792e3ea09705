"""ctypes binding of libmivq.so — the MI355X HIP implementation of the hot path.

Every public function here takes torch tensors that already live on the current HIP
device, validates shape / dtype / contiguity on the host, and calls the matching C entry
point of ``include/mivq.h`` on the current torch stream.  There is no CPU fallback: on a
machine without a HIP device (or without the built library) every compute call raises.

The error mapping mirrors the reference's exceptions:
  MIVQ_ERR_INVALID     -> ValueError (AssertionError for "D must be divisible by M",
                          product_quantization.py:61-62)
  MIVQ_ERR_UNSUPPORTED -> ValueError
  MIVQ_ERR_HIP / _WORKSPACE -> RuntimeError
"""

from __future__ import annotations

import ctypes
import os
import threading
from pathlib import Path
from typing import NamedTuple, Optional, Tuple

import numpy as np
import torch  # noqa: F401  (must be imported before libmivq: they share libamdhip64.so.7)

_PKG_ROOT = Path(__file__).resolve().parent.parent  # vector-quantization_amd/
LIB_PATH = Path(os.environ.get("MIVQ_LIB", _PKG_ROOT / "lib" / "libmivq.so"))

MIVQ_OK = 0
MIVQ_ERR_INVALID = -1
MIVQ_ERR_UNSUPPORTED = -2
MIVQ_ERR_HIP = -3
MIVQ_ERR_WORKSPACE = -4
MIVQ_PQ_AUTO = 0
MIVQ_PQ_FORCE_EXACT = 1
MIVQ_PQ_LEGACY_MFMA = 2
MIVQ_PQ_LEGACY_EXACT = 4
METRIC_INNER_PRODUCT = 0
METRIC_L2 = 1
NO_ID = 0xFFFFFFFF
MAX_QUERIES_PER_CALL = 65535  # mivq_ivfpq_search, and mivq_rabitq_search on its generic estimator (grid.y)

_c = ctypes
_vp, _i32, _i64, _u32, _sz = _c.c_void_p, _c.c_int32, _c.c_int64, _c.c_uint32, _c.c_size_t

# name -> (restype, argtypes); exactly the declarations of include/mivq.h
SIGNATURES = {
    "mivq_last_error": (_c.c_char_p, []),
    "mivq_abi_version": (_c.c_int, []),
    "mivq_device_info": (_c.c_int, [_c.c_int, _c.c_char_p, _c.POINTER(_i32), _c.POINTER(_i64), _c.POINTER(_i64)]),
    "mivq_pq_prep_bytes": (_sz, [_i32, _i32, _i32]),
    "mivq_pq_prepare": (_c.c_int, [_vp, _i32, _i32, _i32, _vp, _vp]),
    "mivq_pq_encode_workspace_bytes": (_sz, [_i64, _i32, _i32, _i32]),
    "mivq_pq_encode": (_c.c_int, [_vp, _i64, _i32, _i32, _i32, _vp, _vp, _vp, _sz, _vp, _u32, _vp]),
    "mivq_pq_decode": (_c.c_int, [_vp, _i64, _i32, _i32, _i32, _vp, _vp, _vp]),
    "mivq_pq_unpack": (_c.c_int, [_vp, _i64, _i32, _i32, _vp, _vp]),
    "mivq_kmeans_update": (_c.c_int, [_vp, _i64, _i32, _i32, _i32, _vp, _vp, _vp, _vp]),
    "mivq_opq_rotate": (_c.c_int, [_vp, _i64, _i32, _vp, _i32, _vp, _vp]),
    "mivq_opq_prep_bytes": (_sz, [_i32]),
    "mivq_opq_prepare": (_c.c_int, [_vp, _i32, _i32, _vp, _vp]),
    "mivq_opq_rotate_workspace_bytes": (_sz, [_i64, _i32]),
    "mivq_opq_rotate_prepared": (_c.c_int, [_vp, _i64, _i32, _vp, _vp, _sz, _vp, _vp]),
    "mivq_opq_gram_workspace_bytes": (_sz, [_i64, _i32]),
    "mivq_opq_gram": (_c.c_int, [_vp, _vp, _i64, _i32, _vp, _sz, _vp, _vp]),
    "mivq_sq_encode_f32": (_c.c_int, [_vp, _i64, _i32, _vp, _vp, _i32, _vp, _vp]),
    "mivq_sq_encode_f64": (_c.c_int, [_vp, _i64, _i32, _vp, _vp, _i32, _vp, _vp]),
    "mivq_sq_decode_f32": (_c.c_int, [_vp, _i64, _i32, _vp, _vp, _i32, _vp, _vp]),
    "mivq_sq_decode_f64": (_c.c_int, [_vp, _i64, _i32, _vp, _vp, _i32, _vp, _vp]),
    "mivq_column_mean": (_c.c_int, [_vp, _i64, _i32, _vp, _vp]),
    "mivq_lvq_encode": (_c.c_int, [_vp, _i64, _i32, _vp, _i32, _vp, _vp]),
    "mivq_lvq_decode": (_c.c_int, [_vp, _i64, _i32, _vp, _i32, _vp, _vp]),
    "mivq_lvq2_encode": (_c.c_int, [_vp, _i64, _i32, _vp, _i32, _i32, _vp, _vp, _vp]),
    "mivq_lvq2_decode": (_c.c_int, [_vp, _vp, _i64, _i32, _vp, _i32, _i32, _vp, _vp]),
    "mivq_rabitq_encode": (_c.c_int, [_vp, _i64, _i32, _vp, _i32, _vp, _vp]),
    "mivq_rabitq_decode": (_c.c_int, [_vp, _i64, _i32, _vp, _vp, _vp]),
    "mivq_rabitq_search_workspace_bytes": (_sz, [_i64, _i64, _i32, _i32]),
    "mivq_rabitq_search": (_c.c_int, [_vp, _i64, _i32, _vp, _vp, _i64, _i32, _i32, _i32, _i64, _vp, _sz, _vp, _vp,
                                      _vp]),
    "mivq_extrabitq_normalize": (_c.c_int, [_vp, _i32, _i64, _i32, _vp, _vp, _vp, _vp]),
    "mivq_extrabitq_quantize": (_c.c_int, [_vp, _i64, _i32, _vp, _i32, _vp, _vp, _vp]),
    "mivq_extrabitq_dequantize": (_c.c_int, [_vp, _i64, _i32, _vp, _i32, _vp, _vp]),
    "mivq_extrabitq_finish": (_c.c_int, [_vp, _i64, _i32, _vp, _i32, _vp, _vp, _vp]),
    "mivq_extrabitq_rotate": (_c.c_int, [_vp, _i64, _i32, _vp, _i32, _vp, _vp]),
    "mivq_rankaware_center": (_c.c_int, [_vp, _i32, _i64, _i32, _vp, _vp, _vp]),
    "mivq_rankaware_quantize": (_c.c_int, [_vp, _i64, _i32, _vp, _vp, _vp, _vp, _i32, _vp, _vp]),
    "mivq_rankaware_dequantize": (_c.c_int, [_vp, _i64, _i32, _vp, _vp, _vp, _vp, _i32, _vp, _vp]),
    "mivq_rankaware_finish": (_c.c_int, [_vp, _i64, _i32, _vp, _vp, _vp]),
    "mivq_rankaware_flat_search_workspace_bytes": (_sz, [_i64, _i64, _i32, _i32, _i32]),
    "mivq_rankaware_flat_search": (_c.c_int, [_vp, _i64, _vp, _i64, _i32, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i64,
                                              _vp, _sz, _vp, _vp, _vp]),
    "mivq_codebook1d_workspace_bytes": (_sz, [_i64, _i32, _i32, _i32]),
    "mivq_codebook1d_fit": (_c.c_int, [_vp, _i64, _i32, _vp, _vp, _i32, _vp, _i32, _vp, _sz, _vp, _vp, _vp]),
    "mivq_adc_lut": (_c.c_int, [_vp, _i64, _i32, _i32, _i32, _vp, _i32, _vp, _vp]),
    "mivq_adc_search_workspace_bytes": (_sz, [_i64, _i64, _i32, _i32, _i32]),
    "mivq_adc_search": (_c.c_int, [_vp, _i64, _vp, _i64, _i32, _i32, _i32, _i64, _vp, _sz, _vp, _vp, _c.c_uint32,
                                   _vp]),
    "mivq_flat_search_workspace_bytes": (_sz, [_i64, _i64, _i32, _i32]),
    "mivq_flat_search": (_c.c_int, [_vp, _i64, _vp, _i64, _i32, _i32, _i32, _i64, _vp, _sz, _vp, _vp, _vp]),
    "mivq_sq_flat_search_workspace_bytes": (_sz, [_i64, _i64, _i32, _i32]),
    "mivq_sq_flat_search": (_c.c_int, [_vp, _i64, _vp, _i64, _i32, _vp, _vp, _i32, _i32, _i32, _i64, _vp, _sz, _vp, _vp,
                                       _vp]),
    "mivq_rabitq_flat_search_workspace_bytes": (_sz, [_i64, _i64, _i32, _i32]),
    "mivq_rabitq_flat_search": (_c.c_int, [_vp, _i64, _vp, _i64, _i32, _vp, _i32, _i32, _i64, _vp, _sz, _vp, _vp, _vp]),
    "mivq_lvq_flat_search_workspace_bytes": (_sz, [_i64, _i64, _i32, _i32]),
    "mivq_lvq_flat_search": (_c.c_int, [_vp, _i64, _vp, _i64, _i32, _vp, _i32, _i32, _i32, _i64, _vp, _sz, _vp, _vp,
                                        _vp]),
    "mivq_rerank_f32_workspace_bytes": (_sz, [_i64, _i64, _i32]),
    "mivq_rerank_f32": (_c.c_int, [_vp, _i64, _vp, _i64, _vp, _i64, _i32, _i32, _i32, _i64, _vp, _sz, _vp, _vp, _vp]),
    "mivq_rerank_sq_workspace_bytes": (_sz, [_i64, _i64, _i32]),
    "mivq_rerank_sq": (_c.c_int, [_vp, _i64, _vp, _i64, _vp, _i64, _i32, _vp, _vp, _i32, _i32, _i32, _i64, _vp, _sz, _vp,
                                  _vp, _vp]),
    "mivq_rerank_lvq_workspace_bytes": (_sz, [_i64, _i64, _i32]),
    "mivq_rerank_lvq": (_c.c_int, [_vp, _i64, _vp, _i64, _vp, _i64, _i32, _vp, _i32, _i32, _i32, _i64, _vp, _sz, _vp, _vp,
                                   _vp]),
    "mivq_rerank_lvq2_workspace_bytes": (_sz, [_i64, _i64, _i32]),
    "mivq_rerank_lvq2": (_c.c_int, [_vp, _i64, _vp, _i64, _vp, _vp, _i64, _i32, _vp, _i32, _i32, _i32, _i32, _i64, _vp,
                                    _sz, _vp, _vp, _vp]),
    "mivq_extrabitq_flat_search_workspace_bytes": (_sz, [_i64, _i64, _i32, _i32]),
    "mivq_extrabitq_flat_search": (_c.c_int, [_vp, _i64, _vp, _i64, _i32, _vp, _i32, _i32, _i32, _i64, _vp, _sz, _vp,
                                              _vp, _vp]),
    "mivq_topk_merge": (_c.c_int, [_vp, _vp, _i32, _i64, _i32, _vp, _vp, _vp]),
    "mivq_pairwise_distances": (_c.c_int, [_vp, _i64, _vp, _i64, _i32, _i32, _vp, _vp]),
    "mivq_topk_rows": (_c.c_int, [_vp, _i64, _i64, _i32, _vp, _vp, _vp]),
    "mivq_bucket_sort_workspace_bytes": (_sz, [_i64, _i32]),
    "mivq_bucket_sort": (_c.c_int, [_vp, _i64, _i32, _vp, _vp, _vp, _sz, _vp]),
    "mivq_centroid_update": (_c.c_int, [_vp, _i64, _i32, _i32, _vp, _vp, _vp, _vp, _vp]),
    "mivq_ivf_residuals": (_c.c_int, [_vp, _i64, _i32, _vp, _vp, _vp, _vp]),
    "mivq_gather_rows": (_c.c_int, [_vp, _i64, _vp, _i64, _vp, _vp]),
    "mivq_ivfpq_terms": (_c.c_int, [_vp, _i64, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mivq_ivfpq_search_workspace_bytes": (_sz, [_i64, _i32, _i32]),
    "mivq_ivfpq_search": (_c.c_int, [_vp, _i64, _i32, _i32, _vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _i32, _i32,
                                     _vp, _sz, _vp, _vp, _vp]),
    "mivq_ivf_rabitq_encode": (_c.c_int, [_vp, _i64, _i32, _vp, _i32, _vp, _i32, _vp, _vp]),
    "mivq_ivf_rabitq_search_workspace_bytes": (_sz, [_i64, _i64, _i32, _i32, _i32, _i32]),
    "mivq_ivf_rabitq_search": (_c.c_int, [_vp, _i64, _i32, _vp, _i32, _vp, _i32, _vp, _vp, _vp, _i32, _i32, _i32,
                                          _vp, _sz, _vp, _vp, _vp]),
    "mivq_ivf_sq_fit": (_c.c_int, [_vp, _i64, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _vp]),
    "mivq_ivf_sq_encode": (_c.c_int, [_vp, _i64, _i32, _vp, _i32, _vp, _vp, _vp, _i32, _vp, _vp]),
    "mivq_ivf_sq_decode": (_c.c_int, [_vp, _i64, _i32, _vp, _i32, _vp, _vp, _vp, _i32, _vp, _vp]),
    "mivq_ivf_lvq_encode": (_c.c_int, [_vp, _i64, _i32, _vp, _i32, _vp, _vp, _i32, _vp, _vp]),
    "mivq_ivf_lvq_decode": (_c.c_int, [_vp, _i64, _i32, _vp, _i32, _vp, _vp, _i32, _vp, _vp]),
    "mivq_ivf_sq_search_workspace_bytes": (_sz, [_i64, _i64, _i32, _i32, _i32, _i32, _i32]),
    "mivq_ivf_sq_search": (_c.c_int, [_vp, _i64, _i32, _vp, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32,
                                      _vp, _sz, _vp, _vp, _vp]),
    "mivq_ivf_lvq_search_workspace_bytes": (_sz, [_i64, _i64, _i32, _i32, _i32, _i32, _i32]),
    "mivq_ivf_lvq_search": (_c.c_int, [_vp, _i64, _i32, _vp, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _i32, _i32, _i32,
                                       _vp, _sz, _vp, _vp, _vp]),
    "mivq_ivf_listpq_decode": (_c.c_int, [_vp, _i64, _i32, _i32, _i32, _vp, _vp, _i32, _vp, _vp, _vp]),
    "mivq_ivf_listpq_search_workspace_bytes": (_sz, [_i64, _i64, _i32, _i32, _i32, _i32, _i32, _i32]),
    "mivq_ivf_listpq_search": (_c.c_int, [_vp, _i64, _i32, _i32, _i32, _vp, _vp, _i32, _vp, _i32, _vp, _vp, _vp, _i32,
                                          _i32, _vp, _sz, _vp, _vp, _vp]),
}

ABI_VERSION = 2  # MIVQ_ABI_VERSION of include/mivq.h the table above binds
_lib: Optional[ctypes.CDLL] = None
_lock = threading.Lock()


def load_library() -> ctypes.CDLL:
    """Load libmivq.so and bind every exported symbol (works without a GPU)."""
    global _lib
    with _lock:
        if _lib is None:
            if not LIB_PATH.exists():
                raise RuntimeError(
                    f"libmivq.so not found at {LIB_PATH}; build it with "
                    "`make -C vector-quantization_amd/csrc` (or __graft_entry__.build())"
                )
            lib = ctypes.CDLL(str(LIB_PATH))
            lib.mivq_abi_version.restype = ctypes.c_int
            if lib.mivq_abi_version() != ABI_VERSION:
                raise RuntimeError(f"{LIB_PATH} has ABI {lib.mivq_abi_version()}, this package binds ABI "
                                   f"{ABI_VERSION}: rebuild it (make -C vector-quantization_amd/csrc)")
            for name, (res, args) in SIGNATURES.items():
                fn = getattr(lib, name)
                fn.restype = res
                fn.argtypes = args
            _lib = lib
    return _lib


def require_device() -> torch.device:
    """The HIP device compute runs on; raises when none is visible (no CPU fallback)."""
    if not torch.cuda.is_available():
        raise RuntimeError(
            "haag_vq (MI355X build) needs a HIP device: no GPU is visible and this "
            "implementation has no CPU fallback"
        )
    load_library()
    return torch.device("cuda", torch.cuda.current_device())


def _raise(rc: int) -> None:
    msg = load_library().mivq_last_error().decode(errors="replace")
    if rc == MIVQ_ERR_INVALID:
        if "divisible" in msg:
            raise AssertionError(msg)
        raise ValueError(msg)
    if rc == MIVQ_ERR_UNSUPPORTED:
        raise ValueError(msg)
    raise RuntimeError(msg)


def _call(name: str, *args) -> None:
    rc = getattr(load_library(), name)(*args)
    if rc != MIVQ_OK:
        _raise(rc)


def _stream() -> ctypes.c_void_p:
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _check(t: torch.Tensor, name: str, dtype: torch.dtype, ndim: Optional[int] = None) -> None:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a torch.Tensor")
    if not t.is_cuda:
        raise ValueError(f"{name}: tensor must live on the HIP device")
    if t.dtype != dtype:
        raise ValueError(f"{name}: dtype {t.dtype} != {dtype}")
    if ndim is not None and t.dim() != ndim:
        raise ValueError(f"{name}: expected {ndim}-D, got shape {tuple(t.shape)}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: tensor must be contiguous")


# ----------------------------------------------------------------- workspace
def kernel_source_hash() -> str:
    """sha256 (first 16 hex digits) of the library's sources (csrc/*.hip, csrc/*.h,
    include/mivq.h, in name order): stamps PMC-derived numbers with the build they describe."""
    import hashlib

    h = hashlib.sha256()
    csrc = _PKG_ROOT / "csrc"
    files = sorted(list(csrc.glob("*.hip")) + list(csrc.glob("*.h"))) + [_PKG_ROOT.parent / "include" / "mivq.h"]
    for f in files:
        h.update(f.name.encode())
        h.update(f.read_bytes())
    return h.hexdigest()[:16]


def workspace(nbytes: int, device: torch.device) -> torch.Tensor:
    """Scratch buffer for one library call (the library never allocates).

    Allocated per call from torch's caching allocator on the current stream: the block goes
    back to that stream's pool when the caller drops it, and torch hands it out again only
    to later work on the same stream, which is ordered after the kernels that used it.  No
    module-level cache, so nothing outlives the call or follows a destroyed stream's handle."""
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)


def _search_call(entry: str, size_args: tuple, head: tuple, nq: int, k: int, device: torch.device, tail: tuple = (),
                 out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """The tail of every search wrapper: the outputs (dists f32 (nq, k), ids int32 (nq, k) holding
    uint32 ids; `out`: the rows of a caller that goes through its queries in ranges), the workspace
    <entry>_workspace_bytes(*size_args) asks for, and the call
    <entry>(*head, ws, ws_bytes, dists, ids, *tail, stream)."""
    if out is None:
        out = (torch.empty((nq, k), dtype=torch.float32, device=device),
               torch.empty((nq, k), dtype=torch.int32, device=device))
    ws = workspace(getattr(load_library(), f"{entry}_workspace_bytes")(*size_args), device)
    _call(entry, *head, _ptr(ws), ws.numel(), _ptr(out[0]), _ptr(out[1]), *tail, _stream())
    return out


def _check_query_width(q: torch.Tensor, d: int) -> None:
    if q.shape[1] != d:
        raise ValueError(f"codes have d={d}, queries d={q.shape[1]}")


def _check_dim_vector(t: torch.Tensor, name: str, d: int, what: str) -> None:
    """A per-dimension f32 vector of d entries."""
    _check(t, name, torch.float32, 1)
    if t.numel() != d:
        raise ValueError(f"{what}: {name} has {t.numel()} entries, expected d={d}")


# ----------------------------------------------------------------- device info
def device_info(device: int = 0) -> dict:
    name = ctypes.create_string_buffer(64)
    cus, lds, hbm = _i32(), _i64(), _i64()
    _call("mivq_device_info", device, name, ctypes.byref(cus), ctypes.byref(lds), ctypes.byref(hbm))
    return {"arch": name.value.decode(), "cus": cus.value, "lds_per_cu": lds.value, "hbm_bytes": hbm.value}


# ----------------------------------------------------------------- PQ
def pq_code_size(M: int, nbits: int) -> int:
    return (M * nbits + 7) // 8


def pq_prepare(centroids: torch.Tensor, nbits: int) -> torch.Tensor:
    """centroids (M, ksub, dsub) f32 -> prep bytes for pq_encode."""
    _check(centroids, "centroids", torch.float32, 3)
    M, ksub, dsub = centroids.shape
    if ksub != (1 << nbits):
        raise ValueError(f"centroids have ksub={ksub}, expected 2**{nbits}")
    d = M * dsub
    nb = load_library().mivq_pq_prep_bytes(d, M, nbits)
    prep = torch.empty(nb, dtype=torch.uint8, device=centroids.device)
    _call("mivq_pq_prepare", _ptr(centroids), d, M, nbits, _ptr(prep), _stream())
    return prep


def pq_encode(x: torch.Tensor, centroids: torch.Tensor, prep: torch.Tensor, nbits: int,
              exact: bool = False, out: Optional[torch.Tensor] = None, flags_extra: int = 0) -> torch.Tensor:
    _check(x, "x", torch.float32, 2)
    _check(centroids, "centroids", torch.float32, 3)
    n, d = x.shape
    M, ksub, dsub = centroids.shape
    if d != M * dsub:
        raise ValueError(f"x has d={d}, codebook expects {M * dsub}")
    cs = pq_code_size(M, nbits)
    if out is None:
        out = torch.empty((n, cs), dtype=torch.uint8, device=x.device)
    else:
        _check(out, "out", torch.uint8, 2)
        if tuple(out.shape) != (n, cs):
            raise ValueError(f"out shape {tuple(out.shape)} != {(n, cs)}")
    nb = load_library().mivq_pq_encode_workspace_bytes(n, d, M, nbits)
    ws = workspace(nb, x.device)
    flags = (MIVQ_PQ_FORCE_EXACT if exact else MIVQ_PQ_AUTO) | flags_extra
    _call("mivq_pq_encode", _ptr(x), n, d, M, nbits, _ptr(centroids), _ptr(prep), _ptr(ws), ws.numel(),
          _ptr(out), flags, _stream())
    return out


def pq_decode(codes: torch.Tensor, centroids: torch.Tensor, nbits: int,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
    _check(codes, "codes", torch.uint8, 2)
    _check(centroids, "centroids", torch.float32, 3)
    M, ksub, dsub = centroids.shape
    n = codes.shape[0]
    if codes.shape[1] != pq_code_size(M, nbits):
        raise ValueError(f"codes have {codes.shape[1]} bytes per row, expected {pq_code_size(M, nbits)}")
    d = M * dsub
    if out is None:
        out = torch.empty((n, d), dtype=torch.float32, device=codes.device)
    _call("mivq_pq_decode", _ptr(codes), n, d, M, nbits, _ptr(centroids), _ptr(out), _stream())
    return out


def pq_unpack(codes: torch.Tensor, M: int, nbits: int) -> torch.Tensor:
    _check(codes, "codes", torch.uint8, 2)
    n = codes.shape[0]
    out = torch.empty((n, M), dtype=torch.uint8, device=codes.device)
    _call("mivq_pq_unpack", _ptr(codes), n, M, nbits, _ptr(out), _stream())
    return out


def kmeans_update(x: torch.Tensor, assign: torch.Tensor, centroids: torch.Tensor,
                  counts: torch.Tensor) -> None:
    _check(x, "x", torch.float32, 2)
    _check(assign, "assign", torch.uint8, 2)
    _check(centroids, "centroids", torch.float32, 3)
    _check(counts, "counts", torch.int32, 2)
    n, d = x.shape
    M, ksub, dsub = centroids.shape
    _call("mivq_kmeans_update", _ptr(x), n, d, M, ksub, _ptr(assign), _ptr(centroids), _ptr(counts), _stream())


# ----------------------------------------------------------------- OPQ
def opq_rotate(x: torch.Tensor, A: torch.Tensor, transpose: bool = False,
               out: Optional[torch.Tensor] = None) -> torch.Tensor:
    _check(x, "x", torch.float32, 2)
    _check(A, "A", torch.float32, 2)
    n, d = x.shape
    if tuple(A.shape) != (d, d):
        raise ValueError(f"A must be ({d}, {d}), got {tuple(A.shape)}")
    if out is None:
        out = torch.empty_like(x)
    _call("mivq_opq_rotate", _ptr(x), n, d, _ptr(A), 1 if transpose else 0, _ptr(out), _stream())
    return out


def opq_backend(d: Optional[int] = None) -> str:
    """What the OPQ classes rotate with (for reports)."""
    return "opq_row_scale_kernel + opq_split_gemm_kernel: split-f16 MFMA GEMM, fp32 accuracy"


def opq_prepare(A: torch.Tensor, transpose: bool = False) -> Optional[torch.Tensor]:
    """Scaled f16 hi / lo image of op(A) for opq_rotate_prepared (None when d % 8 != 0)."""
    _check(A, "A", torch.float32, 2)
    d = A.shape[0]
    if tuple(A.shape) != (d, d):
        raise ValueError(f"A must be square, got {tuple(A.shape)}")
    nb = load_library().mivq_opq_prep_bytes(d)
    if nb == 0:
        return None
    prep = torch.empty(nb, dtype=torch.uint8, device=A.device)
    _call("mivq_opq_prepare", _ptr(A), d, 1 if transpose else 0, _ptr(prep), _stream())
    return prep


def opq_rotate_prepared(x: torch.Tensor, prep: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y = x . op(A) for the op(A) that `prep` was built from (opq_prepare)."""
    _check(x, "x", torch.float32, 2)
    _check(prep, "prep", torch.uint8, 1)
    n, d = x.shape
    if prep.numel() != load_library().mivq_opq_prep_bytes(d):
        raise ValueError(f"prep has {prep.numel()} bytes, not the image of a ({d}, {d}) matrix")
    if out is None:
        out = torch.empty_like(x)
    else:
        _check(out, "out", torch.float32, 2)
        if tuple(out.shape) != (n, d):
            raise ValueError(f"out shape {tuple(out.shape)} != {(n, d)}")
    ws = workspace(load_library().mivq_opq_rotate_workspace_bytes(n, d), x.device)
    _call("mivq_opq_rotate_prepared", _ptr(x), n, d, _ptr(prep), _ptr(ws), ws.numel(), _ptr(out), _stream())
    return out


def opq_gram(x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """G = x^T y in fp64 (d, d) on the library's fp64 MFMA kernel (OPQ Procrustes step)."""
    _check(x, "x", torch.float32, 2)
    _check(y, "y", torch.float32, 2)
    if x.shape != y.shape:
        raise ValueError(f"opq_gram: x {tuple(x.shape)} and y {tuple(y.shape)} differ")
    n, d = x.shape
    G = torch.empty((d, d), dtype=torch.float64, device=x.device)
    ws = workspace(load_library().mivq_opq_gram_workspace_bytes(n, d), x.device)
    _call("mivq_opq_gram", _ptr(x), _ptr(y), n, d, _ptr(ws), ws.numel(), _ptr(G), _stream())
    return G


# ----------------------------------------------------------------- SQ
def sq_encode(x: torch.Tensor, lo: torch.Tensor, den: torch.Tensor, nbits: int) -> torch.Tensor:
    if x.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"sq_encode: unsupported dtype {x.dtype}")
    _check(x, "x", x.dtype, 2)
    _check(lo, "lo", x.dtype, 1)
    _check(den, "den", x.dtype, 1)
    n, d = x.shape
    if lo.numel() != d or den.numel() != d:
        raise ValueError(f"sq_encode: min/max have {lo.numel()}/{den.numel()} entries, data has d={d}")
    if nbits == 16:
        out = torch.empty((n, d), dtype=torch.int16, device=x.device)
    elif nbits == 8:
        out = torch.empty((n, d), dtype=torch.uint8, device=x.device)
    elif nbits == 4:
        out = torch.empty((n, (d + 1) // 2), dtype=torch.uint8, device=x.device)
    else:
        raise ValueError(f"num_bits must be 4, 8, or 16, got {nbits}")
    fn = "mivq_sq_encode_f64" if x.dtype == torch.float64 else "mivq_sq_encode_f32"
    _call(fn, _ptr(x), n, d, _ptr(lo), _ptr(den), nbits, _ptr(out), _stream())
    return out


def sq_decode(codes: torch.Tensor, d: int, lo: torch.Tensor, den: torch.Tensor, nbits: int) -> torch.Tensor:
    if not codes.is_contiguous() or not codes.is_cuda:
        raise ValueError("codes must be a contiguous device tensor")
    n = codes.shape[0]
    dt = lo.dtype
    _check(lo, "lo", dt, 1)
    _check(den, "den", dt, 1)
    if lo.numel() != d or den.numel() != d:
        raise ValueError(f"sq_decode: min/max have {lo.numel()}/{den.numel()} entries, expected d={d}")
    want = {4: ((d + 1) // 2, (torch.uint8,)), 8: (d, (torch.uint8,)), 16: (d, (torch.int16, torch.uint16))}
    if nbits not in want:
        raise ValueError(f"num_bits must be 4, 8, or 16, got {nbits}")
    width, dtypes = want[nbits]
    if codes.dim() != 2 or codes.shape[1] != width or codes.dtype not in dtypes:
        raise ValueError(f"sq_decode: {nbits}-bit codes of d={d} must be ({n}, {width}) {dtypes[0]}, "
                         f"got {tuple(codes.shape)} {codes.dtype}")
    out = torch.empty((n, d), dtype=dt, device=codes.device)
    fn = "mivq_sq_decode_f64" if dt == torch.float64 else "mivq_sq_decode_f32"
    _call(fn, _ptr(codes), n, d, _ptr(lo), _ptr(den), nbits, _ptr(out), _stream())
    return out


# ----------------------------------------------------------------- LVQ
def lvq_code_size(d: int, nbits: int) -> int:
    return (d * nbits + 7) // 8 + 8


def _lvq_bits_check(nbits: int) -> None:
    if not 1 <= nbits <= 8:
        raise ValueError(f"num_bits must be in [1, 8], got {nbits}")


def column_mean(x: torch.Tensor) -> torch.Tensor:
    """numpy's X.mean(axis=0) of a C-contiguous f32 array, bit for bit: the fp32 column sums in
    ascending row order, divided by float(n)."""
    _check(x, "x", torch.float32, 2)
    n, d = x.shape
    if n < 1 or d < 1:
        raise ValueError(f"column_mean: empty input {tuple(x.shape)}")
    out = torch.empty((d,), dtype=torch.float32, device=x.device)
    _call("mivq_column_mean", _ptr(x), n, d, _ptr(out), _stream())
    return out


def lvq_encode(x: torch.Tensor, mu: torch.Tensor, nbits: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    _lvq_bits_check(nbits)
    _check(x, "x", torch.float32, 2)
    _check(mu, "mu", torch.float32, 1)
    n, d = x.shape
    if mu.numel() != d:
        raise ValueError(f"lvq_encode: mu has {mu.numel()} entries, data has d={d}")
    cs = lvq_code_size(d, nbits)
    if out is None:
        out = torch.empty((n, cs), dtype=torch.uint8, device=x.device)
    else:
        _check(out, "out", torch.uint8, 2)
        if tuple(out.shape) != (n, cs):
            raise ValueError(f"out shape {tuple(out.shape)} != {(n, cs)}")
    _call("mivq_lvq_encode", _ptr(x), n, d, _ptr(mu), nbits, _ptr(out), _stream())
    return out


def _lvq_code_check(codes: torch.Tensor, d: int, nbits: int, what: str) -> None:
    _lvq_bits_check(nbits)
    if not isinstance(codes, torch.Tensor) or codes.dtype != torch.uint8 or codes.dim() != 2:
        raise ValueError(f"{what}: codes must be a 2-D uint8 tensor, got "
                         f"{tuple(getattr(codes, 'shape', ()))} {getattr(codes, 'dtype', type(codes))}")
    if codes.shape[1] != lvq_code_size(d, nbits):
        raise ValueError(f"codes have {codes.shape[1]} bytes per row, expected {lvq_code_size(d, nbits)}")
    _check(codes, "codes", torch.uint8, 2)


def lvq_decode(codes: torch.Tensor, mu: torch.Tensor, nbits: int) -> torch.Tensor:
    _check(mu, "mu", torch.float32, 1)
    d = mu.numel()
    _lvq_code_check(codes, d, nbits, "lvq_decode")
    n = codes.shape[0]
    out = torch.empty((n, d), dtype=torch.float32, device=codes.device)
    _call("mivq_lvq_decode", _ptr(codes), n, d, _ptr(mu), nbits, _ptr(out), _stream())
    return out


# ----------------------------------------------------------------- two-level LVQ
def _lvq2_bits_check(nbits1: int, nbits2: int) -> None:
    if not 1 <= nbits1 <= 8:
        raise ValueError(f"primary num_bits must be in [1, 8], got {nbits1}")
    if nbits2 not in (4, 8):
        raise ValueError(f"residual num_bits must be 4 or 8, got {nbits2}")


def lvq2_code_sizes(d: int, nbits1: int, nbits2: int) -> Tuple[int, int]:
    """Bytes per row of (codes1, codes2): the LVQ row at nbits1, and ceil(d nbits2 / 8) without a trailer."""
    return lvq_code_size(d, nbits1), (d * nbits2 + 7) // 8


def _lvq2_code_check(codes1: torch.Tensor, codes2: torch.Tensor, d: int, nbits1: int, nbits2: int, what: str) -> None:
    _lvq2_bits_check(nbits1, nbits2)
    for name, c, size in zip(("codes1", "codes2"), (codes1, codes2), lvq2_code_sizes(d, nbits1, nbits2)):
        if not isinstance(c, torch.Tensor) or c.dtype != torch.uint8 or c.dim() != 2:
            raise ValueError(f"{what}: {name} must be a 2-D uint8 tensor, got "
                             f"{tuple(getattr(c, 'shape', ()))} {getattr(c, 'dtype', type(c))}")
        if c.shape[1] != size:
            raise ValueError(f"{name} has {c.shape[1]} bytes per row, expected {size}")
        _check(c, name, torch.uint8, 2)
    if codes1.shape[0] != codes2.shape[0]:
        raise ValueError(f"{what}: codes1 has {codes1.shape[0]} rows, codes2 {codes2.shape[0]}")


def lvq2_encode(x: torch.Tensor, mu: torch.Tensor, nbits1: int, nbits2: int, out1: Optional[torch.Tensor] = None,
                out2: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(codes1, codes2) of mivq_lvq2_encode: codes1 is lvq_encode(x, mu, nbits1) byte for byte."""
    _lvq2_bits_check(nbits1, nbits2)
    _check(x, "x", torch.float32, 2)
    _check(mu, "mu", torch.float32, 1)
    n, d = x.shape
    if mu.numel() != d:
        raise ValueError(f"lvq2_encode: mu has {mu.numel()} entries, data has d={d}")
    outs = []
    for name, out, size in zip(("out1", "out2"), (out1, out2), lvq2_code_sizes(d, nbits1, nbits2)):
        if out is None:
            out = torch.empty((n, size), dtype=torch.uint8, device=x.device)
        else:
            _check(out, name, torch.uint8, 2)
            if tuple(out.shape) != (n, size):
                raise ValueError(f"{name} shape {tuple(out.shape)} != {(n, size)}")
        outs.append(out)
    _call("mivq_lvq2_encode", _ptr(x), n, d, _ptr(mu), nbits1, nbits2, _ptr(outs[0]), _ptr(outs[1]), _stream())
    return outs[0], outs[1]


def lvq2_decode(codes1: torch.Tensor, codes2: torch.Tensor, mu: torch.Tensor, nbits1: int, nbits2: int) -> torch.Tensor:
    _check(mu, "mu", torch.float32, 1)
    d = mu.numel()
    _lvq2_code_check(codes1, codes2, d, nbits1, nbits2, "lvq2_decode")
    n = codes1.shape[0]
    out = torch.empty((n, d), dtype=torch.float32, device=codes1.device)
    _call("mivq_lvq2_decode", _ptr(codes1), _ptr(codes2), n, d, _ptr(mu), nbits1, nbits2, _ptr(out), _stream())
    return out


# ----------------------------------------------------------------- RaBitQ
def rabitq_code_size(d: int) -> int:
    return (d + 7) // 8 + 8


def rabitq_encode(x: torch.Tensor, centroid: Optional[torch.Tensor], metric: int,
                  out: Optional[torch.Tensor] = None) -> torch.Tensor:
    _check(x, "x", torch.float32, 2)
    n, d = x.shape
    if centroid is not None:
        _check(centroid, "centroid", torch.float32, 1)
    cs = rabitq_code_size(d)
    if out is None:
        out = torch.empty((n, cs), dtype=torch.uint8, device=x.device)
    else:
        _check(out, "out", torch.uint8, 2)
        if tuple(out.shape) != (n, cs):
            raise ValueError(f"out shape {tuple(out.shape)} != {(n, cs)}")
    _call("mivq_rabitq_encode", _ptr(x), n, d, _ptr(centroid), metric, _ptr(out), _stream())
    return out


def rabitq_decode(codes: torch.Tensor, d: int, centroid: Optional[torch.Tensor]) -> torch.Tensor:
    _check(codes, "codes", torch.uint8, 2)
    if codes.shape[1] != rabitq_code_size(d):
        raise ValueError(f"codes have {codes.shape[1]} bytes per row, expected {rabitq_code_size(d)}")
    n = codes.shape[0]
    out = torch.empty((n, d), dtype=torch.float32, device=codes.device)
    _call("mivq_rabitq_decode", _ptr(codes), n, d, _ptr(centroid), _ptr(out), _stream())
    return out


def rabitq_search(codes: torch.Tensor, d: int, centroid: Optional[torch.Tensor], q: torch.Tensor, qb: int,
                  metric: int, k: int, id_offset: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """IndexRaBitQ estimator search: (keys f32 (nq, k), ids int32 (nq, k) holding uint32 ids);
    L2 keys are distance estimates, IP keys negated inner-product estimates (ascending)."""
    _check(codes, "codes", torch.uint8, 2)
    _check(q, "q", torch.float32, 2)
    if centroid is not None:
        _check(centroid, "centroid", torch.float32, 1)
    if codes.shape[1] != rabitq_code_size(d) or q.shape[1] != d:
        raise ValueError(f"codes rows {codes.shape[1]} B / queries d={q.shape[1]} do not match d={d}")
    n, nq = codes.shape[0], q.shape[0]
    dists = torch.empty((nq, k), dtype=torch.float32, device=q.device)
    ids = torch.empty((nq, k), dtype=torch.int32, device=q.device)
    # the generic estimator (qb = 0, d % 32 != 0 or unaligned codes) takes at most
    # MAX_QUERIES_PER_CALL queries per call (its grid.y); queries are independent, so ranges of
    # them give the rows of one call
    generic = qb == 0 or d % 32 != 0 or codes.data_ptr() % 4 != 0
    step = MAX_QUERIES_PER_CALL if generic else max(nq, 1)
    for s in range(0, max(nq, 1), step):
        c = min(nq, s + step) - s
        _search_call("mivq_rabitq_search", (c, n, d, k),
                     (_ptr(codes), n, d, _ptr(centroid), _ptr(q[s:s + c]), c, qb, metric, k, id_offset),
                     c, k, q.device, out=(dists[s:s + c], ids[s:s + c]))
    return dists, ids


# ----------------------------------------------------------------- fp64 GEMM
def gemm_f64(a: torch.Tensor, b: torch.Tensor, transpose: bool) -> torch.Tensor:
    """a . b (or a . b^T) for (n, d) a and (d, d) b in fp64 on the library's MFMA GEMM
    (csrc/gemm_f64.hip; the C entry point keeps its first user's name, mivq_extrabitq_rotate)."""
    _check(a, "a", torch.float64, 2)
    _check(b, "b", torch.float64, 2)
    n, d = a.shape
    if tuple(b.shape) != (d, d):
        raise ValueError(f"b shape {tuple(b.shape)} != {(d, d)}")
    out = torch.empty((n, d), dtype=torch.float64, device=a.device)
    _call("mivq_extrabitq_rotate", _ptr(a), n, d, _ptr(b), 1 if transpose else 0, _ptr(out), _stream())
    return out


# ----------------------------------------------------------------- Extended RaBitQ
extrabitq_rotate = gemm_f64  # the o . P / o_hat . P^T rotations (extended_rabitq.py:140,196)


def extrabitq_code_size(d: int, nbits: int) -> int:
    return (d * nbits + 7) // 8 + 8


def _extrabitq_bits_check(nbits: int) -> None:
    if nbits not in range(1, 9):
        raise ValueError(f"num_bits must be in [1, 8], got {nbits}")


def extrabitq_normalize(x: torch.Tensor, c: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(o (n, d) f64, nrm (n,) f64) of mivq_extrabitq_normalize: r = x - c, nrm = ||r||,
    o = r / max(nrm, 1e-12); x is f32 or f64 rows."""
    if not isinstance(x, torch.Tensor) or x.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"extrabitq: unsupported dtype {getattr(x, 'dtype', type(x))}")
    _check(x, "x", x.dtype, 2)
    _check(c, "c", torch.float64, 1)
    n, d = x.shape
    if c.numel() != d:
        raise ValueError(f"extrabitq: c has {c.numel()} entries, data has d={d}")
    o = torch.empty((n, d), dtype=torch.float64, device=x.device)
    nrm = torch.empty((n,), dtype=torch.float64, device=x.device)
    _call("mivq_extrabitq_normalize", _ptr(x), 1 if x.dtype == torch.float64 else 0, n, d, _ptr(c), _ptr(o),
          _ptr(nrm), _stream())
    return o, nrm


def extrabitq_quantize(s_raw: torch.Tensor, levels: torch.Tensor, nbits: int, nrm: torch.Tensor,
                       out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Code rows (n, code_size) u8 of mivq_extrabitq_quantize from the rotated unit rows
    s_raw = o . P (n, d) f64 and their norms: the B-bit level indices of s_raw * sqrt(d), MSB-first,
    then f32 nrm and f32 t."""
    _extrabitq_bits_check(nbits)
    _check(s_raw, "s_raw", torch.float64, 2)
    _check(levels, "levels", torch.float64, 1)
    _check(nrm, "nrm", torch.float64, 1)
    n, d = s_raw.shape
    if levels.numel() != 1 << nbits:
        raise ValueError(f"extrabitq: levels has {levels.numel()} entries, expected {1 << nbits}")
    if nrm.numel() != n:
        raise ValueError(f"extrabitq: nrm has {nrm.numel()} entries, data has n={n}")
    cs = extrabitq_code_size(d, nbits)
    if out is None:
        out = torch.empty((n, cs), dtype=torch.uint8, device=s_raw.device)
    else:
        _check(out, "out", torch.uint8, 2)
        if tuple(out.shape) != (n, cs):
            raise ValueError(f"out shape {tuple(out.shape)} != {(n, cs)}")
    _call("mivq_extrabitq_quantize", _ptr(s_raw), n, d, _ptr(levels), nbits, _ptr(nrm), _ptr(out), _stream())
    return out


def extrabitq_encode(x: torch.Tensor, c: torch.Tensor, P: torch.Tensor, levels: torch.Tensor,
                     nbits: int) -> torch.Tensor:
    """Codes of ExtendedRaBitQuantizer.compress (the o . P rotation on gemm_f64)."""
    o, nrm = extrabitq_normalize(x, c)
    return extrabitq_quantize(gemm_f64(o, P, False), levels, nbits, nrm)


def _extrabitq_code_check(codes: torch.Tensor, d: int, nbits: int, what: str) -> None:
    _extrabitq_bits_check(nbits)
    if not isinstance(codes, torch.Tensor) or codes.dtype != torch.uint8 or codes.dim() != 2:
        raise ValueError(f"{what}: codes must be a 2-D uint8 tensor, got "
                         f"{tuple(getattr(codes, 'shape', ()))} {getattr(codes, 'dtype', type(codes))}")
    if codes.shape[1] != extrabitq_code_size(d, nbits):
        raise ValueError(f"codes have {codes.shape[1]} bytes per row, expected {extrabitq_code_size(d, nbits)}")
    _check(codes, "codes", torch.uint8, 2)


def extrabitq_dequantize(codes: torch.Tensor, levels: torch.Tensor, nbits: int, d: int) -> torch.Tensor:
    """The unit-sphere levels (n, d) f64 the code rows name, times each row's t
    (mivq_extrabitq_dequantize): o_hat of decode, before the P^T rotation."""
    _extrabitq_code_check(codes, d, nbits, "extrabitq_dequantize")
    _check(levels, "levels", torch.float64, 1)
    if levels.numel() != 1 << nbits:
        raise ValueError(f"extrabitq: levels has {levels.numel()} entries, expected {1 << nbits}")
    n = codes.shape[0]
    o_hat = torch.empty((n, d), dtype=torch.float64, device=codes.device)
    _call("mivq_extrabitq_dequantize", _ptr(codes), n, d, _ptr(levels), nbits, _ptr(o_hat), _stream())
    return o_hat


def extrabitq_finish(y: torch.Tensor, codes: torch.Tensor, c: torch.Tensor, nbits: int) -> torch.Tensor:
    """(n, d) f32 of mivq_extrabitq_finish: f32(y * nrm + c), y = o_hat . P^T (n, d) f64 and nrm the
    f32 norm stored in each code row."""
    _check(y, "y", torch.float64, 2)
    n, d = y.shape
    _extrabitq_code_check(codes, d, nbits, "extrabitq_finish")
    _check(c, "c", torch.float64, 1)
    if codes.shape[0] != n or c.numel() != d:
        raise ValueError(f"extrabitq_finish: {codes.shape[0]} code rows / c of {c.numel()} for y {tuple(y.shape)}")
    out = torch.empty((n, d), dtype=torch.float32, device=y.device)
    _call("mivq_extrabitq_finish", _ptr(y), n, d, _ptr(codes), nbits, _ptr(c), _ptr(out), _stream())
    return out


def extrabitq_decode(codes: torch.Tensor, c: torch.Tensor, P: torch.Tensor, levels: torch.Tensor,
                     nbits: int) -> torch.Tensor:
    _check(P, "P", torch.float64, 2)
    y = gemm_f64(extrabitq_dequantize(codes, levels, nbits, P.shape[0]), P, True)
    return extrabitq_finish(y, codes, c, nbits)


def extrabitq_flat_search(qy: torch.Tensor, codes: torch.Tensor, levels: torch.Tensor, nbits: int, k: int,
                          metric: int = METRIC_L2, id_offset: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """Exact top-k of the rotated queries qy over Extended RaBitQ codes without decoding them
    (mivq_extrabitq_flat_search): the same (dists f32 (nq, k), ids int32 (nq, k) holding uint32
    ids) as flat_search(qy, y_hat) with y_hat = (float)(extrabitq_dequantize(codes) * nrm)."""
    _check(qy, "qy", torch.float32, 2)
    d = qy.shape[1]
    _extrabitq_code_check(codes, d, nbits, "extrabitq_flat_search")
    _check(levels, "levels", torch.float64, 1)
    if levels.numel() != 1 << nbits:
        raise ValueError(f"extrabitq: levels has {levels.numel()} entries, expected {1 << nbits}")
    nq, n = qy.shape[0], codes.shape[0]
    return _search_call("mivq_extrabitq_flat_search", (nq, n, d, k),
                        (_ptr(qy), nq, _ptr(codes), n, d, _ptr(levels), nbits, metric, k, id_offset),
                        nq, k, qy.device)


# ----------------------------------------------------------------- rank-aware quantizer
class RankAwareState(NamedTuple):
    """The device side of a fitted RankAwareQuantizer: mu (d,) f64, V (d, d) f64 and the four
    format tables of include/mivq.h (lv f64, lv_off / pos / width int32).  ``lv32`` is lv rounded
    to f32, the table of the code search; rankaware_lv32 derives it where a state was built
    without it."""
    mu: torch.Tensor
    V: torch.Tensor
    lv: torch.Tensor
    lv_off: torch.Tensor
    pos: torch.Tensor
    width: torch.Tensor
    code_size: int
    lv32: Optional[torch.Tensor] = None


def rankaware_tables(cb, bits, pos, code_size: int):
    """Host arrays (lv f64, lv_off, pos, width int32) of a per-dimension codebook list `cb`,
    widths `bits` and field positions `pos`, checked: widths in [0, 8], 2^width levels per
    dimension, every field inside the row, no two fields on one bit."""
    import numpy as np

    width = np.asarray(bits, dtype=np.int64)
    pos = np.asarray(pos, dtype=np.int64)
    d = width.shape[0]
    code_size = int(code_size)
    if width.ndim != 1 or d < 1 or pos.shape != (d,) or len(cb) != d:
        raise ValueError(f"rankaware: {len(cb)} codebooks, widths {width.shape} and positions {pos.shape} differ")
    if code_size < 1:
        raise ValueError(f"rankaware: code_size must be positive, got {code_size}")
    if np.any(width < 0) or np.any(width > 8):
        raise ValueError("rankaware: widths must be in [0, 8]")
    sizes = np.array([np.asarray(c).shape[0] for c in cb], dtype=np.int64)
    if np.any(sizes != 2 ** width):
        j = int(np.flatnonzero(sizes != 2 ** width)[0])
        raise ValueError(f"rankaware: dimension {j} has {sizes[j]} levels for {width[j]} bits")
    on = width > 0
    pos = np.where(on, pos, 0)
    if np.any(pos < 0) or np.any(pos + width > 8 * code_size):
        raise ValueError(f"rankaware: a field lies outside the {code_size}-byte row")
    used = np.zeros(8 * code_size + 1, dtype=np.int64)
    np.add.at(used, pos[on], 1)
    np.add.at(used, (pos + width)[on], -1)
    if np.any(np.cumsum(used) > 1):
        raise ValueError("rankaware: fields overlap")
    lv_off = np.concatenate(([0], np.cumsum(sizes)))
    if lv_off[-1] >= 2 ** 31:
        raise ValueError("rankaware: level tables too large")
    lv = np.concatenate([np.asarray(c, dtype=np.float64) for c in cb])
    return lv, lv_off.astype(np.int32), pos.astype(np.int32), width.astype(np.int32)


def rankaware_state(mu, V, cb, bits, pos, code_size: int, device: Optional[torch.device] = None) -> RankAwareState:
    """Check the format (rankaware_tables) and put the model on the device."""
    import numpy as np

    lv, lv_off, pos, width = rankaware_tables(cb, bits, pos, code_size)
    d = width.shape[0]
    mu = np.ascontiguousarray(mu, dtype=np.float64)
    V = np.ascontiguousarray(V, dtype=np.float64)
    if mu.shape != (d,) or V.shape != (d, d):
        raise ValueError(f"rankaware: mu {mu.shape} / V {V.shape} do not match d={d}")
    dev = device if device is not None else require_device()
    st = RankAwareState(*(torch.from_numpy(a).to(dev) for a in (mu, V, lv, lv_off, pos, width)), int(code_size))
    return st._replace(lv32=st.lv.to(torch.float32))


def _rankaware_check(st: RankAwareState) -> int:
    _check(st.mu, "mu", torch.float64, 1)
    _check(st.V, "V", torch.float64, 2)
    _check(st.lv, "lv", torch.float64, 1)
    d = st.mu.numel()
    for t, nm, ln in ((st.lv_off, "lv_off", d + 1), (st.pos, "pos", d), (st.width, "width", d)):
        _check(t, nm, torch.int32, 1)
        if t.numel() != ln:
            raise ValueError(f"rankaware: {nm} has {t.numel()} entries, expected {ln}")
    if tuple(st.V.shape) != (d, d):
        raise ValueError(f"rankaware: V shape {tuple(st.V.shape)} != {(d, d)}")
    return d


def rankaware_center(x: torch.Tensor, mu: torch.Tensor) -> torch.Tensor:
    """(double)x - mu, (n, d) f64, for f32 or f64 rows."""
    if x.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"rankaware: unsupported dtype {x.dtype}")
    _check(x, "x", x.dtype, 2)
    _check(mu, "mu", torch.float64, 1)
    n, d = x.shape
    if mu.numel() != d:
        raise ValueError(f"rankaware_center: mu has {mu.numel()} entries, data has d={d}")
    xc = torch.empty((n, d), dtype=torch.float64, device=x.device)
    _call("mivq_rankaware_center", _ptr(x), 1 if x.dtype == torch.float64 else 0, n, d, _ptr(mu), _ptr(xc), _stream())
    return xc


def rankaware_quantize(y: torch.Tensor, st: RankAwareState, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Code rows (n, code_size) u8 of the rotated rows y (n, d) f64."""
    d = _rankaware_check(st)
    _check(y, "y", torch.float64, 2)
    if y.shape[1] != d:
        raise ValueError(f"rankaware_quantize: y has d={y.shape[1]}, the state d={d}")
    n = y.shape[0]
    if out is None:
        codes = torch.empty((n, st.code_size), dtype=torch.uint8, device=y.device)
    else:
        _check(out, "out", torch.uint8, 2)
        if tuple(out.shape) != (n, st.code_size):
            raise ValueError(f"out shape {tuple(out.shape)} != {(n, st.code_size)}")
        codes = out
    _call("mivq_rankaware_quantize", _ptr(y), n, d, _ptr(st.lv), _ptr(st.lv_off), _ptr(st.pos), _ptr(st.width),
          st.code_size, _ptr(codes), _stream())
    return codes


def rankaware_dequantize(codes: torch.Tensor, st: RankAwareState) -> torch.Tensor:
    """The levels (n, d) f64 the code rows name."""
    d = _rankaware_check(st)
    _check(codes, "codes", torch.uint8, 2)
    if codes.shape[1] != st.code_size:
        raise ValueError(f"codes have {codes.shape[1]} bytes per row, expected {st.code_size}")
    n = codes.shape[0]
    y_hat = torch.empty((n, d), dtype=torch.float64, device=codes.device)
    _call("mivq_rankaware_dequantize", _ptr(codes), n, d, _ptr(st.lv), _ptr(st.lv_off), _ptr(st.pos), _ptr(st.width),
          st.code_size, _ptr(y_hat), _stream())
    return y_hat


def rankaware_finish(z: torch.Tensor, mu: torch.Tensor) -> torch.Tensor:
    """(float)(z + mu), (n, d) f32."""
    _check(z, "z", torch.float64, 2)
    _check(mu, "mu", torch.float64, 1)
    n, d = z.shape
    if mu.numel() != d:
        raise ValueError(f"rankaware_finish: mu has {mu.numel()} entries, data has d={d}")
    out = torch.empty((n, d), dtype=torch.float32, device=z.device)
    _call("mivq_rankaware_finish", _ptr(z), n, d, _ptr(mu), _ptr(out), _stream())
    return out


def rankaware_encode(x: torch.Tensor, st: RankAwareState) -> torch.Tensor:
    """Codes of RankAwareQuantizer.compress: center, (x - mu) . V on gemm_f64, quantize."""
    return rankaware_quantize(gemm_f64(rankaware_center(x, st.mu), st.V, False), st)


def rankaware_decode(codes: torch.Tensor, st: RankAwareState) -> torch.Tensor:
    """RankAwareQuantizer.decompress: dequantize, y_hat . V^T on gemm_f64, finish."""
    return rankaware_finish(gemm_f64(rankaware_dequantize(codes, st), st.V, True), st.mu)


_LV32_CACHE: dict = {}  # states built without lv32: (lv storage, version) -> (lv, its f32 rounding)


def rankaware_lv32(st: RankAwareState) -> torch.Tensor:
    """The f32 level table of the code search: st.lv rounded to nearest, derived once per state."""
    if st.lv32 is not None:
        return st.lv32
    key = (st.lv.data_ptr(), st.lv.numel(), st.lv._version, st.lv.device)
    hit = _LV32_CACHE.get(key)
    if hit is None or hit[0] is not st.lv:
        if len(_LV32_CACHE) >= 16:
            _LV32_CACHE.clear()
        hit = _LV32_CACHE[key] = (st.lv, st.lv.to(torch.float32))
    return hit[1]


def rankaware_flat_search(qy: torch.Tensor, codes: torch.Tensor, st: RankAwareState, k: int, metric: int = METRIC_L2,
                          id_offset: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """Exact top-k of the rotated queries qy over rank-aware codes without decoding them
    (mivq_rankaware_flat_search): the same (dists f32 (nq, k), ids int32 (nq, k) holding uint32
    ids) as flat_search(qy, rankaware_dequantize(codes, st).float())."""
    d = _rankaware_check(st)
    if not isinstance(codes, torch.Tensor) or codes.dtype != torch.uint8 or codes.dim() != 2:
        raise ValueError(f"rankaware_flat_search: codes must be a 2-D uint8 tensor, got "
                         f"{tuple(getattr(codes, 'shape', ()))} {getattr(codes, 'dtype', type(codes))}")
    if codes.shape[1] != st.code_size:
        raise ValueError(f"codes have {codes.shape[1]} bytes per row, expected {st.code_size}")
    _check(codes, "codes", torch.uint8, 2)
    if not codes.is_contiguous():
        raise ValueError("codes must be a contiguous device tensor")
    _check(qy, "qy", torch.float32, 2)
    if not qy.is_contiguous():
        raise ValueError("qy must be contiguous")
    _check_query_width(qy, d)
    lv32 = rankaware_lv32(st)
    _check(lv32, "lv32", torch.float32, 1)
    if lv32.numel() != st.lv.numel():
        raise ValueError(f"rankaware: lv32 has {lv32.numel()} entries, lv {st.lv.numel()}")
    nq, n = qy.shape[0], codes.shape[0]
    return _search_call("mivq_rankaware_flat_search", (nq, n, d, st.code_size, k),
                        (_ptr(qy), nq, _ptr(codes), n, d, _ptr(lv32), _ptr(st.lv_off), _ptr(st.pos), _ptr(st.width),
                         st.code_size, metric, k, id_offset), nq, k, qy.device)


# ----------------------------------------------------------------- fitted 1-D codebooks
CB1D_EXACT = 0
CB1D_LLOYD = 1
CB1D_METHODS = {"exact": CB1D_EXACT, "lloyd": CB1D_LLOYD}
CB1D_WORKSPACE_BUDGET = 8 << 30   # bytes of workspace one codebook1d_fit call may ask for
CB1D_DRAWS = 320                  # 2^8 seeds plus room for rejected index draws


def mt19937_64(seed: int, count: int) -> list:
    """The first `count` raw outputs of the 64-bit Mersenne Twister seeded like std::mt19937_64."""
    m64 = (1 << 64) - 1
    mt = [seed & m64]
    for i in range(1, 312):
        mt.append((6364136223846793005 * (mt[-1] ^ (mt[-1] >> 62)) + i) & m64)
    out = []
    while len(out) < count:
        for i in range(312):
            x = (mt[i] & 0xFFFFFFFF80000000) | (mt[(i + 1) % 312] & 0x7FFFFFFF)
            mt[i] = mt[(i + 156) % 312] ^ (x >> 1) ^ (0xB5026F5AA96619E9 if x & 1 else 0)
        for x in mt:
            x ^= (x >> 29) & 0x5555555555555555
            x ^= (x << 17) & 0x71D67FFFEDA60000
            x ^= (x << 37) & 0xFFF7EEE000000000
            out.append((x ^ (x >> 43)) & m64)
    return out[:count]


def codebook1d_tables(width) -> Tuple[np.ndarray, np.ndarray]:
    """(width int32 (d,), lv_off int32 (d + 1,)) of per-dimension tables of 2 ** width levels."""
    width = np.ascontiguousarray(np.asarray(width).reshape(-1), dtype=np.int32)
    if width.size and (width.min() < 0 or width.max() > 8):
        raise ValueError("codebook1d: widths must be in [0, 8]")
    lv_off = np.concatenate(([0], np.cumsum(np.int64(1) << width.astype(np.int64))))
    if lv_off[-1] >= 2 ** 31:
        raise ValueError("codebook1d: level tables too large")
    return width, np.ascontiguousarray(lv_off, dtype=np.int32)


def codebook1d_workspace(n: int, width, method: str, device: Optional[torch.device] = None) -> Tuple[int, int]:
    """(bytes, slots) of the workspace codebook1d_fit allocates by default: slots of the widest
    dimension (mivq_codebook1d_workspace_bytes), one per dimension of non-zero width, as many as
    fit into CB1D_WORKSPACE_BUDGET and into half of the device memory that is free now, at least
    one.  Narrower dimensions, fitted later in the call, get more slots out of the same bytes."""
    width, _ = codebook1d_tables(width)
    live = int(np.count_nonzero(width))
    if method not in CB1D_METHODS:
        raise ValueError(f"codebook1d: method must be 'exact' or 'lloyd', got {method!r}")
    slot = load_library().mivq_codebook1d_workspace_bytes(n, int(width.max()) if live else 0, CB1D_METHODS[method], 1)
    if slot == 0:
        raise ValueError(f"codebook1d: n={n} is not supported")
    budget = CB1D_WORKSPACE_BUDGET
    if device is not None and torch.cuda.is_available():
        budget = min(budget, torch.cuda.mem_get_info(device)[0] // 2)
    slots = max(1, min(max(live, 1), budget // slot))
    return slot * slots, slots


def codebook1d_fit(cols_sorted: torch.Tensor, width, method: str, seed: int = 0,
                   workspace_bytes: Optional[int] = None) -> Tuple[torch.Tensor, np.ndarray, torch.Tensor]:
    """Fit 2 ** width[j] levels to every row of cols_sorted ((d, n) f32, each row ascending) with
    mivq_codebook1d_fit: method "exact" (optimal 1-D k-means) or "lloyd" (k-means++ from
    mt19937_64(seed), <= 50 passes).  Returns (levels f32 (lv_off[d],) on the device, lv_off
    int32 (d + 1,) on the host, sse f64 (d,) on the device); a width-0 dimension keeps level 0
    and sse 0.  The workspace is codebook1d_workspace's (or `workspace_bytes`, at least one slot);
    its size changes how many dimensions run at once, never the result."""
    if method not in CB1D_METHODS:
        raise ValueError(f"codebook1d: method must be 'exact' or 'lloyd', got {method!r}")
    _check(cols_sorted, "cols_sorted", torch.float32, 2)
    d, n = cols_sorted.shape
    width, lv_off = codebook1d_tables(width)
    if width.shape[0] != d:
        raise ValueError(f"codebook1d: {width.shape[0]} widths for {d} rows")
    dev = cols_sorted.device
    levels = torch.zeros(int(lv_off[-1]), dtype=torch.float32, device=dev)
    sse = torch.zeros(d, dtype=torch.float64, device=dev)
    live = int(np.count_nonzero(width))
    if n == 0 or live == 0:
        return levels, lv_off, sse
    m = CB1D_METHODS[method]
    if workspace_bytes is None:
        workspace_bytes = codebook1d_workspace(n, width, method, dev)[0]
    ws = workspace(workspace_bytes, dev)
    draws = None
    if m == CB1D_LLOYD:
        draws = torch.from_numpy(np.array(mt19937_64(seed, CB1D_DRAWS), dtype=np.uint64).view(np.int64)).to(dev)
    _call("mivq_codebook1d_fit", _ptr(cols_sorted), n, d, width.ctypes.data_as(_vp), lv_off.ctypes.data_as(_vp), m,
          _ptr(draws), CB1D_DRAWS if draws is not None else 0, _ptr(ws), int(workspace_bytes), _ptr(levels), _ptr(sse),
          _stream())
    return levels, lv_off, sse


# ----------------------------------------------------------------- ADC / flat search
def adc_lut(q: torch.Tensor, centroids: torch.Tensor, nbits: int, metric: int = METRIC_L2) -> torch.Tensor:
    _check(q, "q", torch.float32, 2)
    _check(centroids, "centroids", torch.float32, 3)
    nq, d = q.shape
    M, ksub, dsub = centroids.shape
    if d != M * dsub:
        raise ValueError(f"queries have d={d}, codebook expects {M * dsub}")
    lut = torch.empty((nq, M, ksub), dtype=torch.float32, device=q.device)
    _call("mivq_adc_lut", _ptr(q), nq, d, M, nbits, _ptr(centroids), metric, _ptr(lut), _stream())
    return lut


# mivq_adc_search flags (include/mivq.h): the product path always passes ADC_AUTO; the others are
# diagnostics (FORCE_EXACT: same results on the fp32 scan) and test hooks (NO_RERUN leaves the
# queries the filter cannot certify NaN)
ADC_AUTO, ADC_FORCE_EXACT, ADC_NO_RERUN, ADC_SMALL_RERUN_GRID = 0, 1, 2, 4


def adc_search(lut: torch.Tensor, codes_u8: torch.Tensor, k: int, nbits: int,
               id_offset: int = 0, flags: int = ADC_AUTO) -> Tuple[torch.Tensor, torch.Tensor]:
    """Returns (dists f32 (nq, k), ids int32 (nq, k) holding uint32 bit patterns)."""
    _check(lut, "lut", torch.float32, 3)
    _check(codes_u8, "codes", torch.uint8, 2)
    nq, M, ksub = lut.shape
    n = codes_u8.shape[0]
    if codes_u8.shape[1] != M:
        raise ValueError(f"codes have {codes_u8.shape[1]} sub-codes, LUT has M={M}")
    return _search_call("mivq_adc_search", (nq, n, M, nbits, k), (_ptr(lut), nq, _ptr(codes_u8), n, M, nbits, k, id_offset),
                        nq, k, lut.device, tail=(flags,))


def flat_search(q: torch.Tensor, x: torch.Tensor, k: int, metric: int = METRIC_L2,
                id_offset: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    _check(q, "q", torch.float32, 2)
    _check(x, "x", torch.float32, 2)
    nq, d = q.shape
    n = x.shape[0]
    if x.shape[1] != d:
        raise ValueError(f"database has d={x.shape[1]}, queries d={d}")
    return _search_call("mivq_flat_search", (nq, n, d, k), (_ptr(q), nq, _ptr(x), n, d, metric, k, id_offset),
                        nq, k, q.device)


def _sq_code_check(codes: torch.Tensor, d: int, nbits: int, what: str) -> None:
    want = {4: ((d + 1) // 2, (torch.uint8,)), 8: (d, (torch.uint8,)), 16: (d, (torch.int16, torch.uint16))}
    if nbits not in want:
        raise ValueError(f"num_bits must be 4, 8, or 16, got {nbits}")
    width, dtypes = want[nbits]
    if not isinstance(codes, torch.Tensor) or codes.dim() != 2 or codes.shape[1] != width or codes.dtype not in dtypes:
        raise ValueError(f"{what}: {nbits}-bit codes of d={d} must be (n, {width}) {dtypes[0]}, "
                         f"got {tuple(getattr(codes, 'shape', ()))} {getattr(codes, 'dtype', type(codes))}")


def sq_flat_search(q: torch.Tensor, codes: torch.Tensor, d: int, lo: torch.Tensor, den: torch.Tensor, nbits: int,
                   k: int, metric: int = METRIC_L2, id_offset: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """Exact top-k over SQ codes without decoding them (mivq_sq_flat_search): the same
    (dists f32 (nq, k), ids int32 (nq, k) holding uint32 ids) as flat_search(q, sq_decode(codes))."""
    _sq_code_check(codes, d, nbits, "sq_flat_search")
    if not codes.is_contiguous() or not codes.is_cuda:
        raise ValueError("codes must be a contiguous device tensor")
    _check(q, "q", torch.float32, 2)
    _check(lo, "lo", torch.float32, 1)
    _check(den, "den", torch.float32, 1)
    if lo.numel() != d or den.numel() != d:
        raise ValueError(f"sq_flat_search: min/max have {lo.numel()}/{den.numel()} entries, expected d={d}")
    _check_query_width(q, d)
    nq, n = q.shape[0], codes.shape[0]
    return _search_call("mivq_sq_flat_search", (nq, n, d, k),
                        (_ptr(q), nq, _ptr(codes), n, d, _ptr(lo), _ptr(den), nbits, metric, k, id_offset),
                        nq, k, q.device)


def rabitq_flat_search(q: torch.Tensor, codes: torch.Tensor, d: int, centroid: Optional[torch.Tensor], k: int,
                       metric: int = METRIC_L2, id_offset: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """Exact top-k over RaBitQ-1 codes without decoding them (mivq_rabitq_flat_search): the same
    result as flat_search(q, rabitq_decode(codes)); not the estimator search rabitq_search."""
    if not isinstance(codes, torch.Tensor) or codes.dtype != torch.uint8 or codes.dim() != 2:
        raise ValueError(f"rabitq_flat_search: codes must be a 2-D uint8 tensor, got "
                         f"{tuple(getattr(codes, 'shape', ()))} {getattr(codes, 'dtype', type(codes))}")
    if codes.shape[1] != rabitq_code_size(d):
        raise ValueError(f"codes have {codes.shape[1]} bytes per row, expected {rabitq_code_size(d)}")
    _check(codes, "codes", torch.uint8, 2)
    _check(q, "q", torch.float32, 2)
    if centroid is not None:
        _check_dim_vector(centroid, "centroid", d, "rabitq_flat_search")
    _check_query_width(q, d)
    nq, n = q.shape[0], codes.shape[0]
    return _search_call("mivq_rabitq_flat_search", (nq, n, d, k),
                        (_ptr(q), nq, _ptr(codes), n, d, _ptr(centroid), metric, k, id_offset), nq, k, q.device)


def lvq_flat_search(q: torch.Tensor, codes: torch.Tensor, mu: torch.Tensor, nbits: int, k: int,
                    metric: int = METRIC_L2, id_offset: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """Exact top-k over LVQ codes without decoding them (mivq_lvq_flat_search): the same
    (dists f32 (nq, k), ids int32 (nq, k) holding uint32 ids) as flat_search(q, lvq_decode(codes))."""
    _check(mu, "mu", torch.float32, 1)
    d = mu.numel()
    _lvq_code_check(codes, d, nbits, "lvq_flat_search")
    _check(q, "q", torch.float32, 2)
    _check_query_width(q, d)
    nq, n = q.shape[0], codes.shape[0]
    return _search_call("mivq_lvq_flat_search", (nq, n, d, k),
                        (_ptr(q), nq, _ptr(codes), n, d, _ptr(mu), nbits, metric, k, id_offset), nq, k, q.device)


def rerank(kind: str, q: torch.Tensor, cand: torch.Tensor, store: torch.Tensor, params: Tuple[torch.Tensor, ...],
           nbits: int, k: int, metric: int = METRIC_L2, id_offset: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """Exact top-k of every query among its own candidate rows (mivq_rerank_*): cand (nq, r) int32
    holding the uint32 global ids a first stage returned; slots outside [id_offset, id_offset + n)
    are skipped, the 0xFFFFFFFF padding among them.  store / params / nbits by kind: 'f32' the
    (n, d) f32 rows, () and 0; 'sq' the code rows of sq_encode, (lo, den) and 4 / 8 / 16; 'lvq' the
    code rows of lvq_encode, (mu,) and 1..8.  Returns (dists f32 (nq, k), ids int32 (nq, k) holding
    uint32 ids), the rows the matching flat search reports for those candidates: ascending keys, IP
    keys negated inner products, missing slots (+inf, 0xFFFFFFFF)."""
    if kind not in ("f32", "sq", "lvq"):
        raise ValueError(f"rerank: kind must be 'f32', 'sq' or 'lvq', got {kind!r}")
    _check(q, "q", torch.float32, 2)
    _check(cand, "cand", torch.int32, 2)
    nq, d = q.shape
    r = cand.shape[1]
    if cand.shape[0] != nq:
        raise ValueError(f"rerank: {cand.shape[0]} candidate lists for {nq} queries")
    names = {"f32": (), "sq": ("lo", "den"), "lvq": ("mu",)}[kind]
    if len(params) != len(names):
        raise ValueError(f"rerank: {kind} takes the parameters {names}")
    for name, t in zip(names, params):
        _check_dim_vector(t, name, d, "rerank")
    if kind == "f32":
        _check(store, "x", torch.float32, 2)
        if store.shape[1] != d:
            raise ValueError(f"database has d={store.shape[1]}, queries d={d}")
        extra = ()
    elif kind == "sq":
        _sq_code_check(store, d, nbits, "rerank")
        if not store.is_contiguous() or not store.is_cuda:
            raise ValueError("codes must be a contiguous device tensor")
        extra = (_ptr(params[0]), _ptr(params[1]), nbits)
    else:
        _lvq_code_check(store, d, nbits, "rerank")
        extra = (_ptr(params[0]), nbits)
    n = store.shape[0]
    return _search_call(f"mivq_rerank_{kind}", (nq, r, k),
                        (_ptr(q), nq, _ptr(cand), r, _ptr(store), n, d, *extra, metric, k, id_offset),
                        nq, k, q.device)


def rerank_lvq2(q: torch.Tensor, cand: torch.Tensor, codes1: torch.Tensor, codes2: torch.Tensor, mu: torch.Tensor,
                nbits1: int, nbits2: int, k: int, metric: int = METRIC_L2,
                id_offset: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """rerank() over the two arrays of lvq2_encode (mivq_rerank_lvq2): the keys are those of
    flat_search(q, lvq2_decode(codes1, codes2)) for the candidates, bit for bit."""
    _check(q, "q", torch.float32, 2)
    _check(cand, "cand", torch.int32, 2)
    nq, d = q.shape
    r = cand.shape[1]
    if cand.shape[0] != nq:
        raise ValueError(f"rerank_lvq2: {cand.shape[0]} candidate lists for {nq} queries")
    _check_dim_vector(mu, "mu", d, "rerank_lvq2")
    _lvq2_code_check(codes1, codes2, d, nbits1, nbits2, "rerank_lvq2")
    n = codes1.shape[0]
    return _search_call("mivq_rerank_lvq2", (nq, r, k),
                        (_ptr(q), nq, _ptr(cand), r, _ptr(codes1), _ptr(codes2), n, d, _ptr(mu), nbits1, nbits2, metric, k,
                         id_offset), nq, k, q.device)


def topk_merge(dists: torch.Tensor, ids: torch.Tensor, k: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """(parts, nq, k) sorted lists -> (nq, k) sorted list, same (dist, id) order."""
    _check(dists, "dists", torch.float32, 3)
    _check(ids, "ids", torch.int32, 3)
    parts, nq, kk = dists.shape
    if kk != k:
        raise ValueError("list length != k")
    od = torch.empty((nq, k), dtype=torch.float32, device=dists.device)
    oi = torch.empty((nq, k), dtype=torch.int32, device=dists.device)
    _call("mivq_topk_merge", _ptr(dists), _ptr(ids), parts, nq, k, _ptr(od), _ptr(oi), _stream())
    return od, oi


# ----------------------------------------------------------------- IVF
def pairwise_distances(x: torch.Tensor, y: torch.Tensor, metric: int = METRIC_L2,
                       out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(n, m) exact chains: L2 sum (x-y)^2, IP -(x . y)."""
    _check(x, "x", torch.float32, 2)
    _check(y, "y", torch.float32, 2)
    n, d = x.shape
    m = y.shape[0]
    if y.shape[1] != d:
        raise ValueError(f"pairwise_distances: d mismatch {d} vs {y.shape[1]}")
    if out is None:
        out = torch.empty((n, m), dtype=torch.float32, device=x.device)
    else:
        _check(out, "out", torch.float32, 2)
        if tuple(out.shape) != (n, m):
            raise ValueError("pairwise_distances: out has the wrong shape")
    _call("mivq_pairwise_distances", _ptr(x), n, _ptr(y), m, d, metric, _ptr(out), _stream())
    return out


def topk_rows(dist: torch.Tensor, k: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """Per row the k smallest (value, column); ids int32 holding uint32 bit patterns."""
    _check(dist, "dist", torch.float32, 2)
    n, m = dist.shape
    od = torch.empty((n, k), dtype=torch.float32, device=dist.device)
    oi = torch.empty((n, k), dtype=torch.int32, device=dist.device)
    _call("mivq_topk_rows", _ptr(dist), n, m, k, _ptr(od), _ptr(oi), _stream())
    return od, oi


def bucket_sort(assign: torch.Tensor, K: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """Stable bucket sort of (n,) int32 assignments: (offsets int64 (K+1), order int32 (n))."""
    _check(assign, "assign", torch.int32, 1)
    n = assign.shape[0]
    offsets = torch.empty(K + 1, dtype=torch.int64, device=assign.device)
    order = torch.empty(n, dtype=torch.int32, device=assign.device)
    nb = load_library().mivq_bucket_sort_workspace_bytes(n, K)
    ws = workspace(nb, assign.device)
    _call("mivq_bucket_sort", _ptr(assign), n, K, _ptr(offsets), _ptr(order), _ptr(ws), ws.numel(), _stream())
    return offsets, order


def centroid_update(x: torch.Tensor, offsets: torch.Tensor, order: torch.Tensor, centroids: torch.Tensor,
                    counts: torch.Tensor) -> None:
    _check(x, "x", torch.float32, 2)
    _check(offsets, "offsets", torch.int64, 1)
    _check(order, "order", torch.int32, 1)
    _check(centroids, "centroids", torch.float32, 2)
    _check(counts, "counts", torch.int32, 1)
    n, d = x.shape
    K = centroids.shape[0]
    if centroids.shape[1] != d or offsets.shape[0] != K + 1 or counts.shape[0] != K or order.shape[0] != n:
        raise ValueError("centroid_update: shape mismatch")
    _call("mivq_centroid_update", _ptr(x), n, d, K, _ptr(offsets), _ptr(order), _ptr(centroids), _ptr(counts),
          _stream())


def ivf_residuals(x: torch.Tensor, coarse: torch.Tensor, assign: torch.Tensor,
                  out: Optional[torch.Tensor] = None) -> torch.Tensor:
    _check(x, "x", torch.float32, 2)
    _check(coarse, "coarse", torch.float32, 2)
    _check(assign, "assign", torch.int32, 1)
    n, d = x.shape
    if coarse.shape[1] != d or assign.shape[0] != n:
        raise ValueError("ivf_residuals: shape mismatch")
    r = torch.empty_like(x) if out is None else out
    _call("mivq_ivf_residuals", _ptr(x), n, d, _ptr(coarse), _ptr(assign), _ptr(r), _stream())
    return r


def gather_rows(src: torch.Tensor, order: torch.Tensor) -> torch.Tensor:
    """dst[i] = src[order[i]] for a contiguous (n, ...) tensor whose rows are 4-byte multiples."""
    _check(order, "order", torch.int32, 1)
    if not src.is_cuda or not src.is_contiguous():
        raise ValueError("gather_rows: src must be a contiguous device tensor")
    row_bytes = src[0].numel() * src.element_size() if src.shape[0] else src.element_size()
    dst = torch.empty((order.shape[0],) + tuple(src.shape[1:]), dtype=src.dtype, device=src.device)
    _call("mivq_gather_rows", _ptr(src), row_bytes, _ptr(order), order.shape[0], _ptr(dst), _stream())
    return dst


def ivfpq_terms(codes_u8: torch.Tensor, pq_centroids: torch.Tensor, prep: torch.Tensor, coarse: torch.Tensor,
                assign: torch.Tensor, nbits: int) -> torch.Tensor:
    _check(codes_u8, "codes", torch.uint8, 2)
    _check(pq_centroids, "pq_centroids", torch.float32, 3)
    _check(coarse, "coarse", torch.float32, 2)
    _check(assign, "assign", torch.int32, 1)
    n, M = codes_u8.shape
    d = coarse.shape[1]
    tau = torch.empty(n, dtype=torch.float32, device=codes_u8.device)
    _call("mivq_ivfpq_terms", _ptr(codes_u8), n, d, M, nbits, _ptr(pq_centroids), _ptr(prep), _ptr(coarse),
          _ptr(assign), _ptr(tau), _stream())
    return tau


def ivfpq_search(lut: torch.Tensor, probe_d: torch.Tensor, probe_l: torch.Tensor, offsets: torch.Tensor,
                 list_codes: torch.Tensor, list_ids: torch.Tensor, tau: Optional[torch.Tensor], metric: int,
                 k: int, nbits: int) -> Tuple[torch.Tensor, torch.Tensor]:
    _check(lut, "lut", torch.float32, 3)
    _check(probe_d, "probe_d", torch.float32, 2)
    _check(probe_l, "probe_l", torch.int32, 2)
    _check(offsets, "offsets", torch.int64, 1)
    _check(list_codes, "list_codes", torch.uint8, 2)
    _check(list_ids, "list_ids", torch.int32, 1)
    if tau is not None:
        _check(tau, "tau", torch.float32, 1)
    nq, M, _ = lut.shape
    nprobe = probe_l.shape[1]
    nlist = offsets.shape[0] - 1
    if probe_d.shape != probe_l.shape or probe_l.shape[0] != nq:
        raise ValueError("ivfpq_search: probe_d / probe_l must both be (nq, nprobe)")
    dists = torch.empty((nq, k), dtype=torch.float32, device=lut.device)
    ids = torch.empty((nq, k), dtype=torch.int32, device=lut.device)
    # one call takes at most MAX_QUERIES_PER_CALL queries (the scan's grid.y); queries are
    # independent, so ranges of them give the rows of one call
    for s in range(0, max(nq, 1), MAX_QUERIES_PER_CALL):
        c = min(nq, s + MAX_QUERIES_PER_CALL) - s
        _search_call("mivq_ivfpq_search", (c, nprobe, k),
                     (_ptr(lut[s:s + c]), c, M, nbits, _ptr(probe_d[s:s + c]), _ptr(probe_l[s:s + c]), nprobe, nlist,
                      _ptr(offsets), _ptr(list_codes), _ptr(list_ids), _ptr(tau), metric, k),
                     c, k, lut.device, out=(dists[s:s + c], ids[s:s + c]))
    return dists, ids


def ivf_rabitq_encode(x: torch.Tensor, coarse: torch.Tensor, assign: torch.Tensor, metric: int,
                      out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """RaBitQ-1 code rows whose centre is the row's list centroid coarse[assign[i]]; bit-identical
    to rabitq_encode(row, coarse[assign[i]], metric).  assign values >= nlist are undefined."""
    _check(x, "x", torch.float32, 2)
    _check(coarse, "coarse", torch.float32, 2)
    _check(assign, "assign", torch.int32, 1)
    n, d = x.shape
    if coarse.shape[1] != d or assign.shape[0] != n:
        raise ValueError("ivf_rabitq_encode: shape mismatch")
    if out is None:
        out = torch.empty((n, rabitq_code_size(d)), dtype=torch.uint8, device=x.device)
    else:
        _check(out, "out", torch.uint8, 2)
        if tuple(out.shape) != (n, rabitq_code_size(d)):
            raise ValueError("ivf_rabitq_encode: out has the wrong shape")
    _call("mivq_ivf_rabitq_encode", _ptr(x), n, d, _ptr(coarse), coarse.shape[0], _ptr(assign), metric, _ptr(out),
          _stream())
    return out


def _ivf_list_search(entry: str, what: str, q: torch.Tensor, coarse: torch.Tensor, probe_l: torch.Tensor,
                     offsets: torch.Tensor, list_codes: torch.Tensor, list_ids: torch.Tensor, size_extra: tuple,
                     mid: tuple, metric: int, k: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """The call of a search over probed lists: mivq_ivf_<entry>_search with the workspace its
    _workspace_bytes asks for.  size_extra: that query's arguments between d and k; mid: the
    search's between list_ids and the metric.  q, coarse and list_codes are checked by the caller."""
    _check(probe_l, "probe_l", torch.int32, 2)
    _check(offsets, "offsets", torch.int64, 1)
    _check(list_ids, "list_ids", torch.int32, 1)
    nq, d = q.shape
    nlist, nprobe = coarse.shape[0], probe_l.shape[1]
    n = list_codes.shape[0]
    if probe_l.shape[0] != nq or offsets.shape[0] != nlist + 1 or list_ids.shape[0] != n:
        raise ValueError(f"{what}: shape mismatch")
    return _search_call(f"mivq_ivf_{entry}_search", (nq, n, nlist, nprobe, d, *size_extra, k),
                        (_ptr(q), nq, d, _ptr(coarse), nlist, _ptr(probe_l), nprobe, _ptr(offsets), _ptr(list_codes),
                         _ptr(list_ids), *mid, metric, k), nq, k, q.device)


def ivf_rabitq_search(q: torch.Tensor, coarse: torch.Tensor, probe_l: torch.Tensor, offsets: torch.Tensor,
                      list_codes: torch.Tensor, list_ids: torch.Tensor, qb: int, metric: int,
                      k: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """RaBitQ estimator search over the probed lists: (keys f32 (nq, k), ids int32 (nq, k) holding
    uint32 ids), ascending; IP keys are negated estimates; missing slots hold (+inf, 0xFFFFFFFF)."""
    _check(q, "q", torch.float32, 2)
    _check(coarse, "coarse", torch.float32, 2)
    _check(list_codes, "list_codes", torch.uint8, 2)
    d = q.shape[1]
    if coarse.shape[1] != d or list_codes.shape[1] != rabitq_code_size(d):
        raise ValueError(f"ivf_rabitq_search: code rows {list_codes.shape[1]} B / coarse d={coarse.shape[1]} do not "
                         f"match d={d}")
    return _ivf_list_search("rabitq", "ivf_rabitq_search", q, coarse, probe_l, offsets, list_codes, list_ids, (), (qb,),
                            metric, k)


# ----------------------------------------------------------------- IVF over per-list SQ / LVQ codes
def sq_code_width(d: int, nbits: int) -> int:
    """Elements per SQ code row (uint8; int16 at 16 bits)."""
    if nbits not in (4, 8, 16):
        raise ValueError(f"num_bits must be 4, 8, or 16, got {nbits}")
    return (d + 1) // 2 if nbits == 4 else d


def _ivf_code_check(coarse: torch.Tensor, assign: Optional[torch.Tensor], params, n: int, d: int, what: str) -> None:
    _check(coarse, "coarse", torch.float32, 2)
    if assign is not None:
        _check(assign, "assign", torch.int32, 1)
    if coarse.shape[1] != d or (assign is not None and assign.shape[0] != n):
        raise ValueError(f"{what}: shape mismatch")
    for name, t in params:
        _check(t, name, torch.float32, 2)
        if tuple(t.shape) != tuple(coarse.shape):
            raise ValueError(f"{what}: {name} is {tuple(t.shape)}, expected {tuple(coarse.shape)}")


def ivf_sq_fit(x: torch.Tensor, coarse: torch.Tensor, offsets: torch.Tensor,
               order: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(lo, den) (nlist, d) of the per-list scalar quantizers: min and (max - min) + 1e-8 of the
    residuals x - coarse[list] over each list's rows (offsets / order: bucket_sort of the lists)."""
    _check(x, "x", torch.float32, 2)
    _check(coarse, "coarse", torch.float32, 2)
    _check(offsets, "offsets", torch.int64, 1)
    _check(order, "order", torch.int32, 1)
    n, d = x.shape
    nlist = coarse.shape[0]
    if coarse.shape[1] != d or offsets.shape[0] != nlist + 1 or order.shape[0] != n:
        raise ValueError("ivf_sq_fit: shape mismatch")
    lo = torch.empty_like(coarse)
    den = torch.empty_like(coarse)
    _call("mivq_ivf_sq_fit", _ptr(x), n, d, _ptr(coarse), nlist, _ptr(offsets), _ptr(order), _ptr(lo), _ptr(den),
          _stream())
    return lo, den


def ivf_sq_encode(x: torch.Tensor, coarse: torch.Tensor, assign: torch.Tensor, lo: torch.Tensor, den: torch.Tensor,
                  nbits: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """SQ code rows of x - coarse[assign[i]] with row assign[i] of lo / den; bit-identical to
    sq_encode(residual, lo[l], den[l]).  assign values >= nlist are undefined."""
    _check(x, "x", torch.float32, 2)
    n, d = x.shape
    _ivf_code_check(coarse, assign, (("lo", lo), ("den", den)), n, d, "ivf_sq_encode")
    shape = (n, sq_code_width(d, nbits))
    dt = torch.int16 if nbits == 16 else torch.uint8
    if out is None:
        out = torch.empty(shape, dtype=dt, device=x.device)
    else:
        _check(out, "out", dt, 2)
        if tuple(out.shape) != shape:
            raise ValueError("ivf_sq_encode: out has the wrong shape")
    _call("mivq_ivf_sq_encode", _ptr(x), n, d, _ptr(coarse), coarse.shape[0], _ptr(assign), _ptr(lo), _ptr(den), nbits,
          _ptr(out), _stream())
    return out


def ivf_sq_decode(codes: torch.Tensor, coarse: torch.Tensor, assign: torch.Tensor, lo: torch.Tensor,
                  den: torch.Tensor, nbits: int) -> torch.Tensor:
    """x^ (n, d) f32: sq_decode(row, lo[l], den[l]) + coarse[l], l = assign[i]."""
    d = coarse.shape[1]
    _sq_code_check(codes, d, nbits, "ivf_sq_decode")
    n = codes.shape[0]
    _ivf_code_check(coarse, assign, (("lo", lo), ("den", den)), n, d, "ivf_sq_decode")
    out = torch.empty((n, d), dtype=torch.float32, device=codes.device)
    _call("mivq_ivf_sq_decode", _ptr(codes), n, d, _ptr(coarse), coarse.shape[0], _ptr(assign), _ptr(lo), _ptr(den),
          nbits, _ptr(out), _stream())
    return out


def ivf_lvq_encode(x: torch.Tensor, coarse: torch.Tensor, assign: torch.Tensor, mu: torch.Tensor, nbits: int,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """LVQ code rows of x - coarse[assign[i]] with mu = row assign[i] of mu (nlist, d); bit-identical
    to lvq_encode(residual, mu[l]).  assign values >= nlist are undefined."""
    _lvq_bits_check(nbits)
    _check(x, "x", torch.float32, 2)
    n, d = x.shape
    _ivf_code_check(coarse, assign, (("mu", mu),), n, d, "ivf_lvq_encode")
    shape = (n, lvq_code_size(d, nbits))
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=x.device)
    else:
        _check(out, "out", torch.uint8, 2)
        if tuple(out.shape) != shape:
            raise ValueError("ivf_lvq_encode: out has the wrong shape")
    _call("mivq_ivf_lvq_encode", _ptr(x), n, d, _ptr(coarse), coarse.shape[0], _ptr(assign), _ptr(mu), nbits, _ptr(out),
          _stream())
    return out


def ivf_lvq_decode(codes: torch.Tensor, coarse: torch.Tensor, assign: torch.Tensor, mu: torch.Tensor,
                   nbits: int) -> torch.Tensor:
    """x^ (n, d) f32: lvq_decode(row, mu[l]) + coarse[l], l = assign[i]."""
    d = coarse.shape[1]
    _lvq_code_check(codes, d, nbits, "ivf_lvq_decode")
    n = codes.shape[0]
    _ivf_code_check(coarse, assign, (("mu", mu),), n, d, "ivf_lvq_decode")
    out = torch.empty((n, d), dtype=torch.float32, device=codes.device)
    _call("mivq_ivf_lvq_decode", _ptr(codes), n, d, _ptr(coarse), coarse.shape[0], _ptr(assign), _ptr(mu), nbits,
          _ptr(out), _stream())
    return out


def ivf_code_search(kind: str, q: torch.Tensor, coarse: torch.Tensor, probe_l: torch.Tensor, offsets: torch.Tensor,
                    list_codes: torch.Tensor, list_ids: torch.Tensor, params: Tuple[torch.Tensor, ...], nbits: int,
                    metric: int, k: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """Exact search over the probed lists of per-list SQ (kind 'sq', params (lo, den)) or LVQ
    (kind 'lvq', params (mu,)) codes: (keys f32 (nq, k), ids int32 (nq, k) holding uint32 ids),
    ascending; IP keys are negated inner products; missing slots hold (+inf, 0xFFFFFFFF)."""
    if kind not in ("sq", "lvq"):
        raise ValueError(f"ivf_code_search: kind must be 'sq' or 'lvq', got {kind!r}")
    _check(q, "q", torch.float32, 2)
    d = q.shape[1]
    if kind == "sq":
        _sq_code_check(list_codes, d, nbits, "ivf_code_search")
        names = ("lo", "den")
    else:
        _lvq_code_check(list_codes, d, nbits, "ivf_code_search")
        names = ("mu",)
    if len(params) != len(names):
        raise ValueError(f"ivf_code_search: {kind} takes the parameters {names}")
    _ivf_code_check(coarse, None, tuple(zip(names, params)), list_codes.shape[0], d, "ivf_code_search")
    return _ivf_list_search(kind, "ivf_code_search", q, coarse, probe_l, offsets, list_codes, list_ids, (nbits,),
                            (*[_ptr(t) for t in params], nbits), metric, k)


# ----------------------------------------------------------------- IVF with a PQ codebook per list
def _ivf_listpq_check(codes: torch.Tensor, codebooks: torch.Tensor, coarse: torch.Tensor, nbits: int, what: str) -> int:
    """Shapes of (n, M) u8 codes, (nlist, M, 2^nbits, dsub) codebooks and (nlist, d) centroids; returns d."""
    _check(codes, "codes", torch.uint8, 2)
    _check(codebooks, "codebooks", torch.float32, 4)
    _check(coarse, "coarse", torch.float32, 2)
    nlist, M, ksub, dsub = codebooks.shape
    if not 1 <= nbits <= 8:
        raise ValueError(f"{what}: nbits={nbits} not in [1, 8]")
    if ksub != 1 << nbits or codes.shape[1] != M or tuple(coarse.shape) != (nlist, M * dsub):
        raise ValueError(f"{what}: codes {tuple(codes.shape)}, codebooks {tuple(codebooks.shape)} and coarse "
                         f"{tuple(coarse.shape)} do not match at nbits={nbits}")
    return M * dsub


def ivf_listpq_decode(codes: torch.Tensor, codebooks: torch.Tensor, coarse: torch.Tensor, assign: torch.Tensor,
                      nbits: int) -> torch.Tensor:
    """x^ (n, d) f32: pq_decode(row, codebooks[l]) + coarse[l], l = assign[i]; codes (n, M) one byte
    per sub-code, rows in any order."""
    d = _ivf_listpq_check(codes, codebooks, coarse, nbits, "ivf_listpq_decode")
    _check(assign, "assign", torch.int32, 1)
    n = codes.shape[0]
    if assign.shape[0] != n:
        raise ValueError("ivf_listpq_decode: shape mismatch")
    out = torch.empty((n, d), dtype=torch.float32, device=codes.device)
    _call("mivq_ivf_listpq_decode", _ptr(codes), n, d, codebooks.shape[1], nbits, _ptr(codebooks), _ptr(coarse),
          coarse.shape[0], _ptr(assign), _ptr(out), _stream())
    return out


def ivf_listpq_search(q: torch.Tensor, codebooks: torch.Tensor, coarse: torch.Tensor, probe_l: torch.Tensor,
                      offsets: torch.Tensor, list_codes: torch.Tensor, list_ids: torch.Tensor, nbits: int, metric: int,
                      k: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """ADC search over the probed lists of an IVF with one PQ codebook per list: (keys f32 (nq, k),
    ids int32 (nq, k) holding uint32 ids), ascending; IP keys are negated inner products; missing
    slots hold (+inf, 0xFFFFFFFF).  Bit-identical to adc_lut(q, codebooks[l] + coarse[l]) +
    adc_search over every probed list, merged by (key, id)."""
    _check(q, "q", torch.float32, 2)
    d = _ivf_listpq_check(list_codes, codebooks, coarse, nbits, "ivf_listpq_search")
    _check(probe_l, "probe_l", torch.int32, 2)
    _check(offsets, "offsets", torch.int64, 1)
    _check(list_ids, "list_ids", torch.int32, 1)
    nq = q.shape[0]
    nlist, M = codebooks.shape[0], codebooks.shape[1]
    n, nprobe = list_codes.shape[0], probe_l.shape[1]
    if q.shape[1] != d or probe_l.shape[0] != nq or offsets.shape[0] != nlist + 1 or list_ids.shape[0] != n:
        raise ValueError("ivf_listpq_search: shape mismatch")
    return _search_call("mivq_ivf_listpq_search", (nq, n, nlist, nprobe, d, M, nbits, k),
                        (_ptr(q), nq, d, M, nbits, _ptr(codebooks), _ptr(coarse), nlist, _ptr(probe_l), nprobe,
                         _ptr(offsets), _ptr(list_codes), _ptr(list_ids), metric, k), nq, k, q.device)
