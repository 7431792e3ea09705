"""CPU: the LVQ entry points' ABI and host logic, and the fixture against a numpy restatement.

tests/golden/lvq_golden.npz (tests/golden/make_lvq_golden.py) holds what the reference's
LVQQuantizer and FlatQuantizedIndex(LVQQuantizer(B)) produced for the cases of tests/_lvq_rule.py.
Here: the inputs regenerate to the stored digests; the restatement of the arithmetic in
explicit float32 steps (_lvq_rule: the sequential-sum mean, encode, the MSB-first packing,
decode) reproduces every stored mean, code row and reconstruction bit for bit, the planted
span == 0 rows and the planted half-to-even ties included; the reference's search result passes
the rule of tests/_search_rule.py within OPEN_CAP.  The device is held to the same fixture in
tests/test_lvq_gpu.py.
"""

import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

import _lvq_rule as LR
import _search_rule as SR

ROOT = Path(__file__).resolve().parents[1]
SYMBOLS = ("mivq_column_mean", "mivq_lvq_encode", "mivq_lvq_decode", "mivq_lvq_flat_search_workspace_bytes",
           "mivq_lvq_flat_search")


@pytest.fixture(scope="module")
def lg(golden_dir):
    return LR.load_fixture(golden_dir)


_made = {}


@pytest.fixture(scope="module")
def cases(lg):
    def get(name) -> LR.Case:
        if name not in _made:
            _made[name] = LR.Case(name, lg)
        return _made[name]

    return get


# ------------------------------------------------------------------------------ ABI
def test_header_declares_the_lvq_symbols():
    txt = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "mivq.h").read_text(), flags=re.S)
    names = set(re.findall(r"\b(mivq_[a-z0-9_]+)\s*\(", txt))
    from haag_vq import _native

    for s in SYMBOLS:
        assert s in names, s
        assert s in _native.SIGNATURES, s
        assert hasattr(_native.load_library(), s), s
    assert "#define MIVQ_ABI_VERSION 2" in txt


def test_workspace_query_needs_no_gpu():
    from haag_vq import _native

    lib = _native.load_library()
    fn = lib.mivq_lvq_flat_search_workspace_bytes
    assert fn(0, 100, 16, 10) == 0 and fn(4, 0, 16, 10) == 0
    # part lists / key blocks only: far below the codes, let alone decoded rows; the layout of
    # the RaBitQ-1 search, which also keeps one per-dimension parameter in LDS
    for shape in ((1, 1_000_000, 3072, 10), (1000, 1_000_000, 3072, 10), (4, 65536, 256, 10), (16, 4096, 64, 256)):
        assert 0 < fn(*shape) < 1_000_000 * 3072
        assert fn(*shape) == lib.mivq_rabitq_flat_search_workspace_bytes(*shape)
    assert fn(4, 65536, 256, 10) < 1 << 20


@pytest.mark.parametrize("nbits", [0, 9, -1])
def test_bad_nbits_is_invalid_before_any_hip_call(nbits):
    """No GPU, null pointers: the argument check comes first and maps to ValueError."""
    from haag_vq import _native

    lib = _native.load_library()
    calls = [
        lambda: lib.mivq_lvq_encode(None, 4, 16, None, nbits, None, None),
        lambda: lib.mivq_lvq_decode(None, 4, 16, None, nbits, None, None),
        lambda: lib.mivq_lvq_flat_search(None, 2, None, 4, 16, None, nbits, 1, 3, 0, None, 0, None, None, None),
    ]
    for call in calls:
        rc = call()
        assert rc == _native.MIVQ_ERR_INVALID
        assert b"num_bits must be in [1, 8]" in lib.mivq_last_error()
        with pytest.raises(ValueError, match=r"num_bits must be in \[1, 8\]"):
            _native._raise(rc)


def test_other_bad_arguments_need_no_gpu():
    from haag_vq import _native

    lib = _native.load_library()
    assert lib.mivq_column_mean(None, 0, 16, None, None) == _native.MIVQ_ERR_INVALID  # no rows: no mean
    assert lib.mivq_column_mean(None, 5, 16, None, None) == _native.MIVQ_ERR_INVALID  # null pointers
    assert lib.mivq_lvq_encode(None, 4, 0, None, 4, None, None) == _native.MIVQ_ERR_INVALID
    assert lib.mivq_lvq_encode(None, 4, 16, None, 4, None, None) == _native.MIVQ_ERR_INVALID
    assert lib.mivq_lvq_encode(None, 0, 16, None, 4, None, None) == _native.MIVQ_OK  # nothing to do
    assert lib.mivq_lvq_decode(None, 0, 16, None, 4, None, None) == _native.MIVQ_OK
    rc = lib.mivq_lvq_flat_search(None, 2, None, 4, 16, None, 4, 1, 257, 0, None, 0, None, None, None)
    assert rc == _native.MIVQ_ERR_UNSUPPORTED  # k > 256, as the other searches
    rc = lib.mivq_lvq_flat_search(None, 2, None, 4, 16, None, 4, 1, 3, ctypes.c_int64(2 ** 32 - 4), None, 0, None,
                                  None, None)
    assert rc == _native.MIVQ_ERR_INVALID and b"ids overflow" in lib.mivq_last_error()


# ------------------------------------------------------------------------------ host classes
@pytest.mark.parametrize("nbits", [0, 9, -3])
def test_quantizer_rejects_bad_num_bits(nbits):
    from haag_vq.methods.lvq_quantization import LVQQuantizer

    with pytest.raises(ValueError, match=r"num_bits must be in \[1, 8\]"):
        LVQQuantizer(nbits)


def test_quantizer_before_fit_and_defaults():
    from haag_vq.methods.base_quantizer import BaseQuantizer
    from haag_vq.methods.lvq_quantization import LVQQuantizer

    q = LVQQuantizer()
    assert isinstance(q, BaseQuantizer) and q.num_bits == 8 and q.mu is None
    with pytest.raises(RuntimeError, match="fit"):
        q.compress(np.zeros((2, 8), np.float32))
    with pytest.raises(RuntimeError, match="fit"):
        q.decompress(np.zeros((2, 16), np.uint8))
    q.mu = np.arange(5, dtype=np.float64)
    assert q.mu.dtype == np.float32 and q.mu.shape == (5,)


@pytest.mark.parametrize("D,B", [(128, 4), (37, 3), (3072, 8), (1, 1), (200, 1), (33, 7)])
def test_compression_ratio(D, B):
    from haag_vq.methods.lvq_quantization import LVQQuantizer

    q = LVQQuantizer(B)
    want = 4 * D / (-(-D * B // 8) + 8)
    assert q.get_compression_ratio(np.empty((3, D), np.float32)) == want
    assert q.code_size(D) == LR.code_size(D, B) == -(-D * B // 8) + 8


def test_registry_builds_lvq():
    from haag_vq.benchmarks import method_registry as reg
    from haag_vq.benchmarks import method_registry_saq as saq
    from haag_vq.benchmarks.quantizer_adapters import FaissQuantizerAdapter
    from haag_vq.methods.lvq_quantization import LVQQuantizer

    a = reg.build_quantizer("lvq", 4, 128)
    assert isinstance(a, FaissQuantizerAdapter) and isinstance(a.quantizer, LVQQuantizer) and a.quantizer.num_bits == 4
    assert reg.build_quantizer("lvq", 2.6, 64).quantizer.num_bits == 3
    assert saq.build_saq_quantizer("lvq", 8, 16).quantizer.num_bits == 8
    assert "lvq" in reg.SUPPORTED_SAQ_METHODS and "lvq" in saq.SUPPORTED_SAQ_METHODS and "lvq" in reg.SAQ_METHODS
    with pytest.raises(ValueError, match=r"num_bits must be in \[1, 8\]"):
        reg.build_quantizer("lvq", 9, 128)
    with pytest.raises(ValueError, match="out of scope"):  # the research methods still are
        reg.build_quantizer("rankaware", 4, 128)


def test_quantizer_state_round_trip():
    from haag_vq.methods.lvq_quantization import LVQQuantizer
    from haag_vq.methods.search.flat_quantized_index import quantizer_from_state, quantizer_state

    q = LVQQuantizer(5)
    q.mu = np.random.default_rng(3).standard_normal(37).astype(np.float32)
    st = quantizer_state(q)
    assert str(st["qtype"]) == "lvq" and int(st["num_bits"]) == 5
    for v in st.values():
        assert np.asarray(v).dtype.kind in "iufU"  # plain arrays: saved with allow_pickle=False
    back = quantizer_from_state(st)
    assert isinstance(back, LVQQuantizer) and back.num_bits == 5
    assert back.mu.dtype == np.float32
    np.testing.assert_array_equal(back.mu.view(np.uint32), q.mu.view(np.uint32))


# ------------------------------------------------------------------------------ fixture vs restatement
def test_fixture_lists_every_case(lg):
    assert list(map(str, lg["cases"])) == list(LR.CASES)
    for v in lg.values():
        assert v.dtype.kind in "iufbU", v.dtype  # plain arrays: numbers, masks, digests
    assert (ROOT / "tests" / "golden" / "lvq_golden.npz").stat().st_size < 1 << 20


@pytest.mark.parametrize("name", list(LR.CASES))
def test_restatement_reproduces_the_reference(cases, name):
    """mean (sequential fp32 column sums / N), codes and reconstructions, bit for bit."""
    cs = cases(name)
    mu = LR.seq_mean(cs.X)
    np.testing.assert_array_equal(mu.view(np.uint32), cs.mu.view(np.uint32))
    cs.codes_match(cs.codes)
    cs.rec_match(cs.rec)
    assert not LR.padding_bits(cs.codes, cs.D, cs.B).any()
    # the planted row: residual 0 everywhere, span == 0, delta = FLT_MIN, every index 0
    idx, lo, delta = LR.unpack(cs.codes[cs.planted:cs.planted + 1], cs.D, cs.B)
    assert delta[0] == LR.TINY and lo[0] == 0.0 and not idx.any()
    np.testing.assert_array_equal(cs.rec[cs.planted], cs.mu)
    # every level of the format is used somewhere, and decode is row-independent
    all_idx, _, _ = LR.unpack(cs.codes, cs.D, cs.B)
    assert all_idx.min() == 0 and all_idx.max() == (1 << cs.B) - 1
    pick = np.array([cs.N - 1, 0, cs.planted])
    np.testing.assert_array_equal(LR.decode(cs.codes[pick], cs.mu, cs.B), cs.rec[pick])


@pytest.mark.parametrize("n,d", [(70000, 16), (4097, 130), (1000, 37), (300, 2)])
def test_numpy_mean_is_the_sequential_sum(n, d):
    """numpy's float32 mean over axis 0 of a C-contiguous (N, D >= 2) array adds the rows in
    order (no pairwise blocks), at sizes the fixture does not hold too.  (With D == 1 the
    reduced axis is the contiguous one and numpy sums it pairwise; the library's definition
    stays the sequential sum.)"""
    rng = np.random.default_rng([n, d])
    X = (rng.standard_normal((n, d)) * 3.0 + rng.standard_normal(d)).astype(np.float32)
    np.testing.assert_array_equal(LR.seq_mean(X).view(np.uint32), X.mean(axis=0).view(np.uint32))


@pytest.mark.parametrize("B,lead,want", LR.ROUNDING)
def test_planted_ties_round_half_to_even(lg, B, lead, want):
    """mu = 0: the quotients 0.5, 1.5, 2.5 are exact ties; half-up would give 1, 2, 3."""
    D = lg[f"round_b{B}_rec"].shape[1]
    row, expect = LR.rounding_row(B, D)
    assert expect == want
    mu = np.zeros(D, np.float32)
    idx, lo, delta = LR.quantize(row[None, :], mu, B)
    assert list(idx[0, :len(want)]) == want
    half_up = np.floor((row - lo[0]) / delta[0] + np.float32(0.5)).astype(np.int32)
    assert list(half_up[:len(want)]) != want
    codes = LR.encode(row[None, :], mu, B)
    np.testing.assert_array_equal(codes, lg[f"round_b{B}_codes"])
    np.testing.assert_array_equal(LR.decode(codes, mu, B).view(np.uint32), lg[f"round_b{B}_rec"].view(np.uint32))


@pytest.mark.parametrize("name", list(LR.SEARCH_CASES))
@pytest.mark.parametrize("metric", LR.METRICS)
def test_reference_search_passes_the_rule(cases, name, metric):
    cs = cases(name)
    j = cs.judge(metric)
    ids, dists = cs.ref(metric)
    print(f"\n[lvq-golden] reference {name} {metric}: open share {j.open_share:.4f}, "
          f"max |dist - key| / e {j.ratio(ids, dists):.4f}")
    np.testing.assert_array_equal(j.open, cs.lg[f"{name}_{metric}_open"])  # derived here = stored
    assert j.open_share <= SR.OPEN_CAP
    j.check(ids, dists, f"reference {name} {metric}")
    assert ids.shape == (cs.c["nq"], min(cs.c["k"], cs.N))
