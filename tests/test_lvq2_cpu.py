"""CPU: the two-level LVQ rule (tests/_lvq2_rule.py) checked against itself and against the
single-level rule, its planted rows, and every refusal that needs no device: the argument checks of
mivq_lvq2_encode / mivq_lvq2_decode / mivq_rerank_lvq2 (made before any HIP call), the workspace
size, TwoLevelLVQQuantizer and LVQ2Index."""

import ctypes

import numpy as np
import pytest

import _lvq2_rule as L2R
import _lvq_rule as LR

F32 = np.float32


# ------------------------------------------------------------------------------ the rule
@pytest.mark.parametrize("name", list(L2R.CASES))
def test_rows_round_trip_and_padding_is_zero(name):
    c = L2R.case(name)
    s1, s2 = L2R.code_sizes(c["D"], c["B1"], c["B2"])
    assert c["codes1"].shape == (c["N"], s1) and c["codes2"].shape == (c["N"], s2)
    np.testing.assert_array_equal(L2R.unpack2(c["codes2"], c["D"], c["B2"]), c["j"])
    assert c["j"].min() >= 0 and c["j"].max() <= (1 << c["B2"]) - 1
    assert not L2R.padding_bits2(c["codes2"], c["D"], c["B2"]).any()
    if c["B2"] == 8:
        np.testing.assert_array_equal(c["codes2"], c["j"].astype(np.uint8))
    else:  # the even dimension in the high nibble
        jp = np.zeros((c["N"], 2 * s2), np.int32)
        jp[:, :c["D"]] = c["j"]
        np.testing.assert_array_equal(c["codes2"], ((jp[:, 0::2] << 4) | jp[:, 1::2]).astype(np.uint8))


@pytest.mark.parametrize("name", list(L2R.CASES))
def test_level_one_is_single_level_lvq(name):
    c = L2R.case(name)
    np.testing.assert_array_equal(c["codes1"], LR.encode(c["X"], c["mu"], c["B1"]))
    a, b = L2R.encode2(c["X"], c["mu"], c["B1"], c["B2"])
    np.testing.assert_array_equal(a, c["codes1"])
    np.testing.assert_array_equal(b, c["codes2"])


@pytest.mark.parametrize("name", list(L2R.SEARCH_CASES))
def test_second_level_cuts_the_error(name):
    """MSE of the reconstruction, two-level over primary: below 1/100 at 4 residual bits and 1/10 000
    at 8 (a uniform step cut in 15 / 255 would give 1/225 and 1/65 025; measured on these inputs
    1/190 and 1/55 000 at the worst)."""
    c = L2R.case(name)
    X = c["X"].astype(np.float64)
    one = np.mean((LR.decode(c["codes1"], c["mu"], c["B1"]).astype(np.float64) - X) ** 2)
    two = np.mean((c["rec"].astype(np.float64) - X) ** 2)
    print(f"{name}: primary MSE {one:.4g}, two-level {two:.4g}, ratio 1/{one / two:.0f}")
    assert two * (100 if c["B2"] == 4 else 10_000) < one


@pytest.mark.parametrize("B2", [4, 8])
def test_planted_ties_round_half_to_even(B2):
    lead, want_idx, want_j = L2R.TIES[B2]
    for D in (len(lead), 37):
        row, _, _ = L2R.tie_row(B2, D)
        idx, lo, delta, j = L2R.quantize2(row[None, :], np.zeros(D, F32), L2R.TIE_B1, B2)
        assert lo[0] == 0.0 and delta[0] == F32((1 << B2) - 1)  # delta2 = 1 exactly
        assert idx[0, :len(lead)].tolist() == want_idx
        assert j[0, :len(lead)].tolist() == want_j
        # round-half-away would differ on every tie
        half_away = np.floor((row[:len(lead)] - idx[0, :len(lead)] * delta[0]) + F32(0.5 * delta[0]) + F32(0.5))
        assert (np.clip(half_away, 0, (1 << B2) - 1).astype(int) != np.array(want_j)).any()


@pytest.mark.parametrize("name", list(L2R.SEARCH_CASES))
def test_span_zero_row(name):
    """The planted row equals mu: delta = FLT_MIN, delta2 subnormal (not flushed), every quotient
    7.4999... / 127.498...; the reconstruction is mu wherever float32 absorbs the 2^-131 left over."""
    c = L2R.case(name)
    p = c["planted"]
    assert c["delta"][p] == LR.TINY and c["lo"][p] == 0.0 and not c["idx"][p].any()
    delta2 = c["delta"][p] / F32((1 << c["B2"]) - 1)
    assert 0.0 < delta2 < LR.TINY
    assert (c["j"][p] == (7 if c["B2"] == 4 else 127)).all()
    big = np.abs(c["mu"]) >= F32(2.0 ** -100)
    assert big.any()
    np.testing.assert_array_equal(c["rec"][p][big], c["mu"][big])
    left = F32(-0.5) * LR.TINY + F32(c["j"][p][0]) * delta2
    np.testing.assert_array_equal(c["rec"][p].view(np.uint32), (left + c["mu"]).astype(F32).view(np.uint32))


# ------------------------------------------------------------------------------ the C ABI
def _fake(n=16):
    return ctypes.c_void_p(n)  # non-null, never dereferenced: every check below precedes the launch


def test_argument_errors_need_no_gpu():
    from haag_vq import _native

    lib = _native.load_library()
    p = _fake()
    INV, UNS, WS, OK = _native.MIVQ_ERR_INVALID, _native.MIVQ_ERR_UNSUPPORTED, _native.MIVQ_ERR_WORKSPACE, _native.MIVQ_OK

    def enc(b1=4, b2=8, n=10, d=8, x=p, mu=p, c1=p, c2=p):
        return lib.mivq_lvq2_encode(x, n, d, mu, b1, b2, c1, c2, None)

    def dec(b1=4, b2=8, n=10, d=8, c1=p, c2=p, mu=p, out=p):
        return lib.mivq_lvq2_decode(c1, c2, n, d, mu, b1, b2, out, None)

    def rr(b1=4, b2=8, nq=2, r=4, n=10, d=8, metric=1, k=3, off=0, q=p, cand=p, c1=p, c2=p, mu=p, ws=p, nb=1 << 20,
           out=p):
        return lib.mivq_rerank_lvq2(q, nq, cand, r, c1, c2, n, d, mu, b1, b2, metric, k, off, ws, nb, out, out, None)

    for fn in (enc, dec, rr):
        for b1 in (0, 9, -1):
            assert fn(b1=b1) == INV, (fn.__name__, b1)
        assert b"[1, 8]" in lib.mivq_last_error()
        for b2 in (0, 1, 5, 7, 16):
            assert fn(b2=b2) == UNS, (fn.__name__, b2)
        assert b"4 or 8" in lib.mivq_last_error()
        assert fn(b1=0, b2=5) == INV  # the primary width is checked first
    for fn in (enc, dec):
        for bad in (dict(n=-1), dict(d=0), dict(d=(1 << 27) + 1), dict(mu=None), dict(c1=None), dict(c2=None)):
            assert fn(**bad) == INV, (fn.__name__, bad)
        assert fn(n=0, mu=None, c1=None, c2=None) == OK  # nothing to do
    assert enc(x=None) == INV and dec(out=None) == INV
    assert b"lvq2_decode" in lib.mivq_last_error()

    for bad in (dict(nq=-1), dict(n=-1), dict(r=0), dict(d=0), dict(q=None), dict(cand=None), dict(c1=None),
                dict(c2=None), dict(mu=None), dict(out=None), dict(off=-1), dict(off=2 ** 32 - 5)):
        assert rr(**bad) == INV, bad
    assert b"rerank_lvq2" in lib.mivq_last_error()
    for bad in (dict(k=0), dict(k=257), dict(metric=7), dict(d=20484)):
        assert rr(**bad) == UNS, bad
    assert rr(d=20480, nb=0) == WS  # the last d whose query and mu rows fit the LDS passes the size check
    need = lib.mivq_rerank_lvq2_workspace_bytes(2, 4, 3)
    assert need > 0 and rr(nb=need - 1) == WS and rr(ws=None) == WS
    assert rr(nq=0, q=None, cand=None, c1=None, c2=None, mu=None, ws=None, nb=0, out=None) == OK
    with pytest.raises(ValueError):
        _native._raise(UNS)


def test_workspace_is_the_single_level_one():
    from haag_vq import _native

    lib = _native.load_library()
    for shape in ((1000, 250, 10), (3, 600, 10), (70_000, 2, 1), (1, 1, 1), (16, 40, 256), (0, 10, 10), (5, 0, 10),
                  (5, 10, 0), (5, 10, 257)):
        assert lib.mivq_rerank_lvq2_workspace_bytes(*shape) == lib.mivq_rerank_lvq_workspace_bytes(*shape), shape
    assert lib.mivq_rerank_lvq2_workspace_bytes(1000, 250, 10) == 2 * 4 * 1000 * 10 * 4
    assert _native.lvq2_code_sizes(100, 4, 4) == (58, 50) and _native.lvq2_code_sizes(37, 3, 8) == (22, 37)
    assert _native.lvq2_code_sizes(33, 7, 4) == (37, 17)


# ------------------------------------------------------------------------------ the classes, host logic
def test_quantizer_refusals():
    from haag_vq.methods.base_quantizer import BaseQuantizer
    from haag_vq.methods.lvq2_quantization import TwoLevelLVQQuantizer
    from haag_vq.methods.lvq_quantization import LVQQuantizer

    for b1 in (0, 9):
        with pytest.raises(ValueError, match="primary_bits"):
            TwoLevelLVQQuantizer(b1, 8)
    for b2 in (0, 2, 5, 16):
        with pytest.raises(ValueError, match="residual_bits"):
            TwoLevelLVQQuantizer(4, b2)
    q = TwoLevelLVQQuantizer()
    assert isinstance(q, BaseQuantizer) and not isinstance(q, LVQQuantizer)
    assert (q.primary_bits, q.residual_bits) == (4, 8)
    assert q.code_size(100) == 58 + 100 and q.code_sizes(100) == (58, 100)
    assert q.get_compression_ratio(np.zeros((1, 100), F32)) == 400 / 158
    for call in (lambda: q.compress(np.zeros((2, 8), F32)), lambda: q.decompress(np.zeros((2, 20), np.uint8)),
                 lambda: q.split(np.zeros((2, 20), np.uint8))):
        with pytest.raises(RuntimeError, match="fit"):
            call()
    q.mu = np.arange(8)
    prim = q.primary()
    assert isinstance(prim, LVQQuantizer) and prim.num_bits == 4 and prim.mu.dtype == F32
    np.testing.assert_array_equal(prim.mu, np.arange(8, dtype=F32))
    codes = np.arange(2 * 20, dtype=np.uint8).reshape(2, 20)  # 4 + 8 primary bytes, 8 residual bytes
    c1, c2 = q.split(codes)
    assert c1.flags.c_contiguous and c2.flags.c_contiguous
    np.testing.assert_array_equal(np.concatenate([c1, c2], axis=1), codes)
    assert c1.shape == (2, 12)
    with pytest.raises(ValueError, match="expected"):
        q.split(codes[:, :19])


def test_index_refusals(tmp_path):
    from haag_vq.methods.search import LVQ2Index

    with pytest.raises(ValueError, match="primary_bits"):
        LVQ2Index(9, 8)
    with pytest.raises(ValueError, match="residual_bits"):
        LVQ2Index(4, 5)
    for bad in (0, -3):
        with pytest.raises(ValueError, match="refine_factor"):
            LVQ2Index(4, 8, refine_factor=bad)
    ix = LVQ2Index()
    assert (ix.primary_bits, ix.residual_bits, ix.refine_factor, ix.ntotal, ix.memory_footprint()) == (4, 8, 10, 0, 0)
    with pytest.raises(RuntimeError, match="fit"):
        ix.search_with_scores(np.zeros((2, 8), F32), 5)
    with pytest.raises(RuntimeError, match="fit"):
        ix.save(tmp_path / "x.npz")
    with pytest.raises(ValueError, match="metric"):
        ix.fit(np.zeros((4, 8), F32), "cosine")
    ix._N = 4096
    assert ix.candidate_count(10) == 100 and ix.candidate_count(25) == 250
    with pytest.raises(ValueError, match=r"26 \* 10 = 260.*at most 256"):  # RefinedIndex's wording
        ix.candidate_count(26)
    with pytest.raises(ValueError, match="at most 256"):
        ix.search_with_scores(np.zeros((2, 8), F32), 26)
    ix._N = 37
    assert ix.candidate_count(10) == 37  # r is capped at N

    path = tmp_path / "lvq2.npz"
    with open(path, "wb") as f:
        np.savez(f, codes1=np.zeros((3, 12), np.uint8), codes2=np.zeros((3, 4), np.uint8), mu=np.zeros(8, F32),
                 primary_bits=np.array(4), residual_bits=np.array(4), metric=np.array("l2"),
                 refine_factor=np.array(10), N=np.array(3), D=np.array(8))
    for b1, b2 in ((4, 8), (3, 4)):
        with pytest.raises(ValueError, match="holds LVQ-4x4 codes"):
            LVQ2Index(b1, b2).load(path)
    with open(path, "wb") as f:  # the widths agree, the shapes do not
        np.savez(f, codes1=np.zeros((3, 12), np.uint8), codes2=np.zeros((3, 5), np.uint8), mu=np.zeros(8, F32),
                 primary_bits=np.array(4), residual_bits=np.array(4), metric=np.array("l2"),
                 refine_factor=np.array(10), N=np.array(3), D=np.array(8))
    with pytest.raises(ValueError, match="not a consistent"):
        LVQ2Index(4, 4).load(path)
