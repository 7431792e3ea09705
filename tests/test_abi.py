"""CPU: libmivq.so builds, loads and exports exactly the C ABI declared in include/mivq.h."""

import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]


def _declared():
    txt = (ROOT / "include" / "mivq.h").read_text()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(mivq_[a-z0-9_]+)\s*\(", txt)))


def test_header_declares_the_boundary():
    names = _declared()
    for must in ("mivq_pq_encode", "mivq_pq_decode", "mivq_opq_rotate", "mivq_sq_encode_f32",
                 "mivq_rabitq_encode", "mivq_adc_lut", "mivq_adc_search", "mivq_topk_merge",
                 "mivq_last_error", "mivq_device_info"):
        assert must in names


def test_library_exports_every_declared_symbol():
    from haag_vq import _native

    lib = _native.load_library()
    for name in _declared():
        assert hasattr(lib, name), name
    assert set(_declared()) == set(_native.SIGNATURES), "ctypes table out of sync with mivq.h"
    assert lib.mivq_abi_version() == 2


def test_size_queries_need_no_gpu():
    from haag_vq import _native

    lib = _native.load_library()
    assert lib.mivq_pq_prep_bytes(1536, 16, 8) > 16 * 256 * 4
    assert lib.mivq_pq_prep_bytes(1000, 16, 8) == 0  # D % M != 0
    assert lib.mivq_pq_encode_workspace_bytes(1000, 1536, 16, 8) > 0
    assert lib.mivq_adc_search_workspace_bytes(100, 10000, 16, 8, 10) > 0


def test_error_path_needs_no_gpu():
    """Argument validation happens before any HIP call and maps to the reference's exceptions."""
    from haag_vq import _native

    lib = _native.load_library()
    rc = lib.mivq_pq_encode(None, 10, 1000, 16, 8, None, None, None, 0, None, 0, None)
    assert rc == _native.MIVQ_ERR_INVALID
    assert b"divisible" in lib.mivq_last_error()
    with pytest.raises(AssertionError):
        _native._raise(rc)
    rc = lib.mivq_sq_encode_f32(None, 1, 4, None, None, 5, None, None)
    assert rc == _native.MIVQ_ERR_INVALID
    with pytest.raises(ValueError):
        _native._raise(rc)


def test_compute_without_gpu_fails_loudly():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from haag_vq.methods.product_quantization import ProductQuantizer

    pq = ProductQuantizer(M=4, B=8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pq.fit([[0.0] * 8] * 300)


def test_no_packed_fp32_on_lds_loads():
    """The built library's gfx950 code never feeds an LDS-read register to a packed fp32
    instruction (v_pk_add/mul/fma_f32): beside another kernel's LDS DMA + MFMAs (hipBLASLt bf16
    GEMMs, for one) those lose lanes 48..63.  tools/isa_audit.py disassembles
    libmivq.so's device code objects and tracks LDS-loaded registers per kernel."""
    import sys

    if not Path("/opt/rocm/lib/llvm/bin/llvm-objdump").exists():
        pytest.skip("ROCm LLVM tools not present")
    sys.path.insert(0, str(ROOT / "tools"))
    import isa_audit

    from haag_vq import _native

    walked = []
    findings = isa_audit.audit(Path(_native.LIB_PATH), walked)
    for k in ("pq_encode_cs_kernel", "pq_resolve_merged_kernel", "adc_lut_kernel", "adc_qscan_kernel",
              "adc_rerank_kernel", "opq_split_gemm_kernel", "pairwise_kernel"):
        assert any(k in w for w in walked), (k, len(walked))  # the audit really read the library
    assert not findings, {k[:80]: v[:2] for k, v in findings.items()}


def test_adc_search_workspace_bounded():
    """The filtered search's part lists and the re-run's lists are bounded: 10M rows
    x 10,000 queries at k = 32 needs well under a gigabyte (unbounded re-run lists: ~10.5 GB),
    100,000 queries stay within a few GB (the output alone is 25.6 MB per 1,000 queries)."""
    from haag_vq import _native

    lib = _native.load_library()
    nb = lib.mivq_adc_search_workspace_bytes(10_000, 10_000_000, 16, 8, 32)
    assert 0 < nb < 800 * 2 ** 20, nb
    nb = lib.mivq_adc_search_workspace_bytes(100_000, 10_000_000, 16, 8, 32)
    assert 0 < nb < 3 * 2 ** 30, nb


def test_rabitq_search_workspace_bounded():
    """The screened estimator search's candidate lists (keys + ids, worst case every key of a
    block) are capped at 2^27 entries (1 GiB) per block, and its dense first block needs only
    8,192 columns: at 1,000 queries x 1M codes x 3072 the whole workspace stays near 1.1 GiB
    (the pre-screen tiled search alone held a 256 MiB key block), and at 100,000 queries it is
    dominated by the per-query int8 / fp32 rows, not by the lists."""
    from haag_vq import _native

    lib = _native.load_library()
    nb = lib.mivq_rabitq_search_workspace_bytes(1000, 1_000_000, 3072, 10)
    assert 0 < nb < 1.25 * 2 ** 30, nb
    nb = lib.mivq_rabitq_search_workspace_bytes(100_000, 10_000_000, 3072, 10)
    rows = 100_000 * 3072 * 5  # qq (int8) + qr (fp32) rows
    assert 0 < nb < rows + 3 * 2 ** 30, nb


def test_search_workspace_sizes_pinned():
    """Every search entry point takes its pointers from the layout its size query reports, so the
    sizes are part of the ABI callers allocate by.  The numbers were read from the library before
    each layout moved into one function: filtered ADC shapes (M = 16 / 32, nbits = 8, k <= 32;
    the last one past the 1 GiB cap of the filtered part lists), fp32-only ADC shapes, the
    streaming and the tiled flat search, the screened RaBitQ search."""
    from haag_vq import _native

    lib = _native.load_library()
    adc = {  # (nq, n, M, nbits, k)
        (1, 1, 16, 8, 1): 68096,
        (100, 10_000, 16, 8, 10): 3604992,
        (1000, 1_000_000, 16, 8, 10): 51332864,
        (1000, 1_000_000, 32, 8, 32): 154085632,
        (1000, 1_000_000, 16, 8, 33): 8448000,
        (17, 5000, 8, 8, 256): 2785280,
        (17, 5000, 12, 6, 10): 109056,
        (100_000, 10_000_000, 16, 8, 32): 1763600128,
    }
    flat = {  # (nq, n, d, k)
        (1, 100, 7, 1): 512,
        (15, 1_000_000, 1536, 10): 2361856,
        (16, 4096, 1536, 10): 266240,
        (1000, 1_000_000, 3072, 100): 276544512,
    }
    rabitq = {  # (nq, n, d, k)
        (1000, 1_000_000, 3072, 10): 1121636608,
        (100_000, 10_000_000, 3072, 10): 4226000128,
    }
    for fn, table in ((lib.mivq_adc_search_workspace_bytes, adc), (lib.mivq_flat_search_workspace_bytes, flat),
                      (lib.mivq_rabitq_search_workspace_bytes, rabitq)):
        for shape, want in table.items():
            assert fn(*shape) == want, (fn.__name__, shape, fn(*shape), want)

    # The four exact searches (f32, SQ, RaBitQ-1, LVQ codes), read from the library while the f32
    # search still had a scan and a layout of its own.  Both sides of the tiled threshold
    # (nq 15 / 16, n 4095 / 4096); the last d and the first d past each queries-per-workgroup step
    # (8, 4, 2, 1, none) of the format's LDS policy, at 15 queries so that the step changes the
    # number of query blocks (f32: 96 KiB of queries; the code formats: 128 KiB of queries plus
    # two (SQ) or one parameter rows; 160 KiB at one query); 1, 2 and 3 queries, where the code
    # formats narrow the query block to the batch; no streaming scan past the last step.
    either_side = {(15, 4095, 1536, 10): 76800, (15, 4096, 1536, 10): 76800, (16, 4095, 1536, 10): 81920,
                   (16, 4096, 1536, 10): 266240}
    small_batch = {(1, 1_000_000, 3072, 100): 3136000, (2, 1_000_000, 3072, 100): 6272000,
                   (3, 1_000_000, 3072, 100): 9408000}
    by_step = (2361856, 1190400, 1190400, 614400, 614400, 326656, 326656, 0)
    steps = (
        (lib.mivq_flat_search_workspace_bytes, (3072, 3076, 6144, 6148, 12288, 12292, 40960, 40964)),
        (lib.mivq_sq_flat_search_workspace_bytes, (3276, 3280, 5460, 5464, 8192, 8196, 13652, 13656)),
        (lib.mivq_rabitq_flat_search_workspace_bytes, (3640, 3644, 6552, 6556, 10920, 10924, 20480, 20484)),
        (lib.mivq_lvq_flat_search_workspace_bytes, (3640, 3644, 6552, 6556, 10920, 10924, 20480, 20484)),
    )
    for fn, ds in steps:
        table = {**either_side, **small_batch, **{(15, 1_000_000, d, 10): want for d, want in zip(ds, by_step)},
                 (1, 5000, ds[-1], 256): 0, (16, 4096, ds[-1], 10): 266240}
        for shape, want in table.items():
            assert fn(*shape) == want, (fn.__name__, shape, fn(*shape), want)


def test_qscan_valu_counts_match_bench():
    """bench.py prices the filtered ADC scan's roofline from the static VALU count of one
    wave-step of adc_qscan_kernel (QSCAN_VALU_PER_STEP); that count must be the built library's."""
    import sys

    if not Path("/opt/rocm/lib/llvm/bin/llvm-objdump").exists():
        pytest.skip("ROCm LLVM tools not present")
    sys.path.insert(0, str(ROOT / "tools"))
    sys.path.insert(0, str(ROOT))
    import bench
    import isa_qscan
    from haag_vq import _native

    got = isa_qscan.count(Path(_native.LIB_PATH))
    for M, v in bench.QSCAN_VALU_PER_STEP.items():
        assert got[str(M)]["valu_32bit"] == v["valu_32bit"] and got[str(M)]["valu_64bit"] == v["valu_64bit"], got
        assert got[str(M)]["ds_read_b128"] == M  # one 16-B table read per subspace
