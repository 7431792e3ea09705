"""CPU: the argument checks of the fast-Hadamard entry points (before any HIP call), the
quantizer's keyword and state, and the rule's own fp64 run against its longdouble run."""

import ctypes

import numpy as np
import pytest

import _fht_rule as F

P = ctypes.c_void_p(64)  # never dereferenced: every case below fails a check first


@pytest.mark.parametrize("entry", ("rotate", "encode", "decode"))
@pytest.mark.parametrize("n,d,rounds,nbits,ptr,rc,word", (
    (-1, 8, 4, 4, P, "INVALID", b"bad sizes"),
    (1, 0, 4, 4, P, "INVALID", b"bad sizes"),
    (1, 8, 0, 4, P, "UNSUPPORTED", b"rounds=0"),
    (1, 8, 9, 4, P, "UNSUPPORTED", b"rounds=9"),
    (1, 16385, 4, 4, P, "UNSUPPORTED", b"d=16385"),
    (1, 8, 4, 9, P, "INVALID", b"num_bits"),
    (1, 8, 4, 4, None, "INVALID", b"null pointer"),
    (0, 8, 4, 4, None, "OK", b""),
))
def test_return_codes(entry, n, d, rounds, nbits, ptr, rc, word):
    from haag_vq import _native

    lib = _native.load_library()
    if entry == "rotate":
        if word == b"num_bits":
            return
        got = lib.mivq_fht_rotate(ptr, n, d, ptr, rounds, 0, ptr, None)
    elif entry == "encode":
        got = lib.mivq_extrabitq_encode_fht(ptr, 0, n, d, ptr, ptr, rounds, ptr, nbits, ptr, None)
    else:
        got = lib.mivq_extrabitq_decode_fht(ptr, n, d, ptr, ptr, rounds, ptr, nbits, ptr, None)
    assert got == getattr(_native, "MIVQ_OK" if rc == "OK" else f"MIVQ_ERR_{rc}")
    assert word in lib.mivq_last_error() or rc == "OK"


def test_constructor_and_state():
    from haag_vq.methods.extended_rabitq import ExtendedRaBitQuantizer

    with pytest.raises(ValueError, match="rotation"):
        ExtendedRaBitQuantizer(4, rotation="hadamard")
    assert ExtendedRaBitQuantizer(4).rotation == "dense"
    X, c, signs, levels = F.case(37)
    q = ExtendedRaBitQuantizer(4, seed=3, rotation="fht")
    q.fit(X)
    assert q.P is None and np.array_equal(q.signs, signs) and np.array_equal(q.c, c)
    st = q.to_state()
    assert "P" not in st and str(st["rotation"]) == "fht" and st["signs"].dtype == np.uint8
    back = ExtendedRaBitQuantizer.from_state(st)
    assert back.rotation == "fht" and back.P is None and np.array_equal(back.signs, signs)
    with pytest.raises(ValueError, match="inconsistent"):
        ExtendedRaBitQuantizer.from_state(dict(st, signs=signs[:, :-1]))


@pytest.mark.parametrize("D", (3, 37, 1536))
def test_rule_is_orthogonal_and_inverts(D):
    x = np.random.default_rng(D).standard_normal((5, D))
    y = F.apply(x, F.draw_signs(1, D))
    assert np.allclose(np.linalg.norm(y.astype(np.float64), axis=1), np.linalg.norm(x, axis=1), rtol=1e-14)
    assert np.abs(F.apply(y, F.draw_signs(1, D), inverse=True) - x).max() < 1e-15 * np.sqrt(D) * 8


@pytest.mark.parametrize("D", (37, 1536))
def test_seed_of_the_quantizer_case_sets_no_row_aside(D):
    """GPU test 3 may set rows with a midpoint tie aside; at its seed the rule's own fp64 run
    against its longdouble run has none."""
    X, c, signs, levels = F.case(D)
    assert np.array_equal(F.encode(X, c, signs, levels)[0], F.encode(X, c, signs, levels, dtype=np.float64)[0])
