"""CPU: the rank-aware quantizer's host side (FFD layouts, Lloyd tables, the allocation greedy,
errors, index state), the numpy rule against the reference's fixture, and the C ABI's argument
checks.  The fixture is tests/golden/rankaware_golden.npz (make_rankaware_golden.py)."""

import io
import re
from pathlib import Path

import numpy as np
import pytest

import _rankaware_rule as RR

ROOT = Path(__file__).resolve().parents[1]
NEW_SYMBOLS = ("mivq_rankaware_center", "mivq_rankaware_quantize", "mivq_rankaware_dequantize",
               "mivq_rankaware_finish")


@pytest.fixture(scope="module")
def z(golden_dir):
    return RR.load_golden(golden_dir)


_quantizer = RR.fixture_quantizer


# ------------------------------------------------------------------ layout and registry
@pytest.mark.parametrize("name", list(RR.CASES))
def test_ffd_layout_equals_the_fixture(z, name):
    from haag_vq.methods import ffd_packing as F

    bits = z[f"{name}_bits"]
    byte_idx, bit_off, n_bytes = F.ffd_layout(bits)
    assert byte_idx.dtype == np.int64 and bit_off.dtype == np.int64
    assert np.array_equal(byte_idx, z[f"{name}_ffd_byte_idx"])
    assert np.array_equal(bit_off, z[f"{name}_ffd_bit_off"])
    assert n_bytes == int(z[f"{name}_ffd_code_size"])
    # the reference's ffd codes are ffd_encode of the indices they hold, and decode back
    st = RR.fixture_state(z, name, "ffd")
    codes = z[f"{name}_ffd_codes"]
    idx = RR.unpack(codes, st)
    assert np.array_equal(F.ffd_encode(idx, bits, byte_idx, bit_off, n_bytes), codes)
    got = F.ffd_decode(codes, bits, byte_idx, bit_off, len(bits))
    assert got.dtype == np.int64 and np.array_equal(got, idx)


def test_ffd_lone_four_packs_optimally():
    from haag_vq.methods import ffd_packing as F

    # 4 + 3 + 3 + 3 = 13 bits: two bytes.  A lone 4 among four 3s and four 2s (24 bits): three
    # bytes as {3, 3, 2}, {3, 3, 2}, {4, 2, 2}; plain FFD starts with {4, 3} (a bit wasted), is left
    # with {3, 3, 2}, {3, 2, 2} and opens a fourth byte for the last 2.
    for widths, best in (([4, 3, 3, 3], 2), ([2, 3, 4, 3, 2, 3, 2, 3, 2], 3)):
        byte_idx, bit_off, n_bytes = F.ffd_layout(np.array(widths))
        assert n_bytes == best == -(-sum(widths) // 8), (widths, n_bytes)
        used = np.zeros((n_bytes, 8), dtype=int)
        for w, b, o in zip(widths, byte_idx, bit_off):
            assert 0 <= o and o + w <= 8
            used[b, o:o + w] += 1
        assert used.max() == 1
    # the 3s go first (by index), then the 4, then the 2s
    assert byte_idx.tolist() == [0, 0, 2, 0, 1, 1, 2, 1, 2] and bit_off.tolist() == [6, 0, 0, 3, 6, 0, 4, 3, 6]


def test_ffd_round_trip_byte_cap_and_errors():
    from haag_vq.methods import ffd_packing as F

    rng = np.random.default_rng(0)
    bits = rng.integers(0, 9, size=50)
    byte_idx, bit_off, n_bytes = F.ffd_layout(bits)
    assert np.all(byte_idx[bits == 0] == -1) and np.all(bit_off[bits == 0] == -1)
    idx = rng.integers(0, 2 ** 62, size=(20, 50)) % (2 ** bits)
    packed = F.ffd_encode(idx, bits, byte_idx, bit_off, n_bytes)
    assert packed.shape == (20, n_bytes) and packed.dtype == np.uint8
    assert np.array_equal(F.ffd_decode(packed, bits, byte_idx, bit_off, 50), idx)
    # byte_cap: 6-bit bins hold 3 + 3 and 4 + 2 but not 4 + 3; no 4-fix outside 8-bit bytes
    byte_idx, bit_off, n_bytes = F.ffd_layout(np.array([4, 3, 3, 2]), byte_cap=6)
    assert n_bytes == 2 and byte_idx.tolist() == [0, 1, 1, 0] and bit_off.tolist() == [0, 0, 3, 4]
    assert F.byte_cap_minus(3, 2) == 3 and F.byte_cap_minus(3, 2, byte_cap=6) == 1
    with pytest.raises(ValueError, match=r"bits_per_dim must be in \[0, 8\]"):
        F.ffd_layout(np.array([1, 9]))
    with pytest.raises(ValueError, match=r"bits_per_dim must be in \[0, 6\]"):
        F.ffd_layout(np.array([7]), byte_cap=6)
    with pytest.raises(ValueError):
        F.ffd_layout(np.array([-1, 2]))


def test_registry_still_out_of_scope_and_class_exported():
    from haag_vq.benchmarks import method_registry as reg
    from haag_vq.methods import RankAwareQuantizer
    from haag_vq.methods.rank_aware_quantization import RankAwareQuantizer as C

    assert RankAwareQuantizer is C
    for m in ("rankaware", "perdim_mse", "rankaware_exact", "perdim_mse_exact"):
        with pytest.raises(ValueError, match="out of scope"):
            reg.build_quantizer(m, 4, 128)


# ------------------------------------------------------------------ the rule against the fixture
@pytest.mark.parametrize("packing", RR.PACKINGS)
@pytest.mark.parametrize("name", list(RR.CASES))
def test_rule_reproduces_the_fixture(z, name, packing):
    X = RR.inputs(name)
    assert RR.sha(X) == str(z[f"{name}_X_sha"])
    st = RR.fixture_state(z, name, packing)
    codes = z[f"{name}_{packing}_codes"]
    assert codes.shape == (RR.CASES[name]["N"], st.code_size)
    Y = RR.project(X, st)
    ref_idx = RR.unpack(codes, st)
    assert np.array_equal(RR.pack(ref_idx, st), codes)      # no bit outside the fields
    assert np.all(codes & ~RR.field_mask(st) == 0)
    assert not RR.tie_problems(RR.indices(Y, st), ref_idx, Y, X, st)
    rec = RR.decompress(codes, st)
    want = z[f"{name}_rec"]
    assert rec.dtype == np.float32
    assert np.all(np.abs(rec.astype(np.float64) - want) <= RR.decode_slack(want, RR.lookup(ref_idx, st), st.D))


def test_all8_dense_and_ffd_bytes_identical(z):
    assert np.all(z["all8_bits"] == 8)
    assert np.array_equal(z["all8_dense_codes"], z["all8_ffd_codes"])


# ------------------------------------------------------------------ allocation, tables, errors
def test_lloyd_tables_bit_for_bit(z):
    from haag_vq.methods import rank_aware_quantization as M

    for b in range(6):
        lv, dmse = M._lloyd_1d_normal(2 ** b, seed=b)
        assert lv.dtype == np.float64 and np.array_equal(lv, z["levels"][2 ** b - 1:2 ** (b + 1) - 1]), b
        if b:
            assert dmse == z["Dg"][b], b
        lv[0] = 99.0                                       # the cache hands out copies
        assert M._lloyd_1d_normal(2 ** b, seed=b)[0][0] != 99.0
    assert z["Dg"][0] == 1.0 and np.all(np.diff(z["Dg"]) < 0)


@pytest.mark.parametrize("name", list(RR.CASES))
def test_allocation_and_layout_from_the_fixture_var(z, name):
    from haag_vq.methods.rank_aware_quantization import allocate_bits

    c = RR.CASES[name]
    bits = allocate_bits(z[f"{name}_var"], z["Dg"], c["avg_bits"], c["alpha"], c["max_bits"])
    assert bits.dtype == np.int64 and np.array_equal(bits, z[f"{name}_bits"])
    for packing in RR.PACKINGS:
        q = _quantizer(z, name, packing)
        assert q._offsets.dtype == np.int64 and np.array_equal(q._offsets, z[f"{name}_offsets"])
        assert q.code_size == int(z[f"{name}_{packing}_code_size"])
        assert np.array_equal(q.field_positions(), RR.fixture_state(z, name, packing).pos)
        if packing == "ffd":
            assert q._ffd_n_bytes == q.code_size
        else:
            assert q._ffd_byte_idx is None
        assert q.get_compression_ratio(np.empty((1, c["D"]))) == c["D"] * 4 / q.code_size
        for d in range(c["D"]):  # cb[d] = levels[bits[d]] * sqrt(var[d])
            assert np.array_equal(q.cb[d], q._levels[bits[d]] * np.sqrt(z[f"{name}_var"][d]))


def test_allocation_stops_at_the_cap():
    from haag_vq.methods.rank_aware_quantization import allocate_bits

    Dg = np.array([1.0, 0.36, 0.12, 0.03])
    bits = allocate_bits(np.array([4.0, 1.0, 0.25]), Dg, avg_bits=5.0, alpha=1.0, max_bits=3)
    assert bits.tolist() == [3, 3, 3]          # budget 15, only 9 can be spent


def test_constructor_and_fit_errors(z):
    from haag_vq.methods.rank_aware_quantization import RankAwareQuantizer

    for bad in (0, 9):
        with pytest.raises(ValueError, match=r"max_bits must be in \[1, 8\]"):
            RankAwareQuantizer(4, max_bits=bad)
    with pytest.raises(ValueError, match="packing must be 'dense' or 'ffd'"):
        RankAwareQuantizer(4, packing="bytes")
    with pytest.raises(ValueError, match="codebook must be 'gaussian', 'lloyd', or 'exact'"):
        RankAwareQuantizer(4, codebook="kmeans")
    for cb in ("lloyd", "exact"):
        q = RankAwareQuantizer(4, codebook=cb)     # accepted, as in the reference
        with pytest.raises(ValueError, match="SAQ engine.*out of scope"):
            q.fit(np.zeros((10, 4), np.float32))
    q = RankAwareQuantizer(4)
    assert (q.avg_bits, q.alpha, q.max_bits, q.seed, q.packing, q.codebook) == (4.0, 1.0, 8, 0, "dense", "gaussian")
    assert q.mu is None and q.V is None and q.bits is None and q.cb is None and q.code_size is None
    with pytest.raises(RuntimeError, match="must be fit before compress"):
        q.compress(np.zeros((1, 4), np.float32))
    with pytest.raises(RuntimeError, match="must be fit before decompress"):
        q.decompress(np.zeros((1, 4), np.uint8))
    q = _quantizer(z, "odd37", "dense")
    with pytest.raises(ValueError, match=r"compress\(\) got D=36, but fit\(\) saw D=37"):
        q.compress(np.zeros((2, 36), np.float32))


def test_table_checks():
    from haag_vq import _native

    cb = [np.zeros(1), np.array([-1.0, 1.0]), np.arange(8.0)]
    lv, lv_off, pos, width = _native.rankaware_tables(cb, [0, 1, 3], [0, 0, 1], 1)
    assert lv.dtype == np.float64 and lv.tolist() == [0.0, -1.0, 1.0] + list(range(8))
    assert lv_off.dtype == np.int32 and lv_off.tolist() == [0, 1, 3, 11]
    assert pos.tolist() == [0, 0, 1] and width.tolist() == [0, 1, 3] and width.dtype == np.int32
    for bits, p, cs, msg in (([0, 1, 3], [0, 0, 6], 1, "outside"), ([0, 1, 3], [0, 1, 1], 1, "overlap"),
                             ([0, 2, 3], [0, 0, 2], 1, "levels"), ([0, 1, 9], [0, 0, 1], 2, "widths"),
                             ([0, 1, 3], [0, -1, 1], 1, "outside"), ([0, 1, 3], [0, 0, 1], 0, "code_size")):
        with pytest.raises(ValueError, match=msg):
            _native.rankaware_tables(cb, bits, p, cs)


@pytest.mark.parametrize("packing", RR.PACKINGS)
def test_quantizer_state_round_trip(z, packing):
    from haag_vq.methods.search.flat_quantized_index import quantizer_from_state, quantizer_state

    q = _quantizer(z, "w08", packing)
    st = quantizer_state(q)
    assert str(st["qtype"]) == "rankaware" and str(st["packing"]) == packing
    assert all(isinstance(v, np.ndarray) and v.dtype != object for v in st.values())
    buf = io.BytesIO()
    np.savez(buf, **st)
    buf.seek(0)
    with np.load(buf, allow_pickle=False) as f:
        q2 = quantizer_from_state(f)
    assert (q2.avg_bits, q2.alpha, q2.max_bits, q2.seed, q2.packing, q2.codebook) == \
        (q.avg_bits, q.alpha, q.max_bits, q.seed, packing, "gaussian")
    for a in ("mu", "V", "var", "bits", "_offsets", "_Dg"):
        assert np.array_equal(getattr(q2, a), getattr(q, a)) and getattr(q2, a).dtype == getattr(q, a).dtype, a
    assert q2.D == q.D and q2.code_size == q.code_size and q2.bits.dtype == np.int64
    assert len(q2.cb) == q.D and all(np.array_equal(a, b) for a, b in zip(q2.cb, q.cb))
    assert all(np.array_equal(a, b) for a, b in zip(q2._levels, q._levels))
    assert np.array_equal(q2.field_positions(), q.field_positions())


# ------------------------------------------------------------------ ABI
def test_symbols_declared_and_bound():
    from haag_vq import _native

    txt = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "mivq.h").read_text(), flags=re.S)
    declared = set(re.findall(r"\b(mivq_[a-z0-9_]+)\s*\(", txt))
    lib = _native.load_library()
    for s in NEW_SYMBOLS:
        assert s in declared and s in _native.SIGNATURES and hasattr(lib, s), s
    assert declared == set(_native.SIGNATURES)
    assert lib.mivq_abi_version() == 2 and "#define MIVQ_ABI_VERSION 2" in txt


def test_argument_checks_need_no_gpu():
    import ctypes

    from haag_vq import _native

    lib = _native.load_library()
    one = ctypes.c_void_p(16)  # never dereferenced: every call below fails (or returns) before a launch
    inv = _native.MIVQ_ERR_INVALID
    q = lib.mivq_rankaware_quantize
    assert q(one, -1, 4, one, one, one, one, 1, one, None) == inv
    assert q(one, 1, 0, one, one, one, one, 1, one, None) == inv
    assert q(one, 1, 4, one, one, one, one, 0, one, None) == inv
    for k in (0, 3, 4, 5, 6, 8):
        args = [one, 1, 4, one, one, one, one, 1, one, None]
        args[k] = None
        assert q(*args) == inv, k
        assert b"null pointer" in lib.mivq_last_error()
    assert q(None, 0, 4, None, None, None, None, 1, None, None) == 0
    dq = lib.mivq_rankaware_dequantize
    assert dq(one, -1, 4, one, one, one, one, 1, one, None) == inv
    assert dq(one, 1, -2, one, one, one, one, 1, one, None) == inv
    assert dq(one, 1, 4, one, one, one, one, -1, one, None) == inv
    assert dq(None, 1, 4, one, one, one, one, 1, one, None) == inv
    assert dq(one, 1, 4, one, one, one, one, 1, None, None) == inv
    assert dq(None, 0, 4, None, None, None, None, 1, None, None) == 0
    assert dq(one, 1, 4, one, one, one, one, 70000, one, None) == _native.MIVQ_ERR_UNSUPPORTED
    c = lib.mivq_rankaware_center
    assert c(one, 0, -1, 4, one, one, None) == inv and c(one, 0, 1, 0, one, one, None) == inv
    assert c(None, 0, 1, 4, one, one, None) == inv and c(one, 1, 1, 4, None, one, None) == inv
    assert c(one, 0, 1, 4, one, None, None) == inv and c(None, 0, 0, 4, None, None, None) == 0
    f = lib.mivq_rankaware_finish
    assert f(one, -1, 4, one, one, None) == inv and f(one, 1, 0, one, one, None) == inv
    assert f(None, 1, 4, one, one, None) == inv and f(one, 1, 4, None, one, None) == inv
    assert f(one, 1, 4, one, None, None) == inv and f(None, 0, 4, None, None, None) == 0
    with pytest.raises(ValueError):
        _native._raise(inv)
