"""Buffer-contract cases of the codecs: PQ, k-means update, OPQ, SQ, LVQ, LVQ2, RaBitQ, Extended
RaBitQ, rank-aware, codebook1d.  See tests/_bounds.py for what a case is."""

from __future__ import annotations

import numpy as np

import _codebook1d_rule as CB
import _extrabitq_search_rule as ES
import _lvq2_rule as L2
import _lvq_rule as LR
import _rabitq_encode_rule as RE
import _rankaware_rule as RA
from _bounds import EDGE, EMPTY, F32, RAGGED, Buf, Call, Host, In, InOut, Out, Ws, add, int_rows, rng, rows

L2M, IPM = 1, 0  # MIVQ_METRIC_L2, MIVQ_METRIC_INNER_PRODUCT
PQ_AUTO, PQ_EXACT, PQ_LEGACY_MFMA, PQ_LEGACY_EXACT = 0, 1, 2, 4


def _lib():
    from haag_vq import _native

    return _native.load_library()


def _np(t) -> np.ndarray:
    return t.detach().cpu().numpy()


# ------------------------------------------------------------------------------ PQ
def _codebook(M, nbits, dsub, *seed):
    return rng(M, nbits, dsub, *seed).standard_normal((M, 1 << nbits, dsub)).astype(F32)


def _pq_code_size(M, nbits):
    return (M * nbits + 7) // 8


def pq_prepare(d, M, nbits):
    def build(O):
        C = _codebook(M, nbits, d // M, 1)
        nb = _lib().mivq_pq_prep_bytes(d, M, nbits)
        # no importable reference of the whole image: the wrapper's call on a fresh buffer
        return Call([In("centroids", C), d, M, nbits, Out("prep", nb), None],
                    expect=lambda c: {"prep": _np(c.N.pq_prepare(c.t(C), nbits))})
    return build


add("mivq_pq_prepare", "mfma-d32-M2-b8", RAGGED, pq_prepare(32, 2, 8))          # filter image + pair table
add("mivq_pq_prepare", "plain-d21-M3-b4", EDGE, pq_prepare(21, 3, 4))           # no image, odd dsub
add("mivq_pq_prepare", "plain-d35-M5-b3", EDGE, pq_prepare(35, 5, 3))


def _prep_buf(C, nbits, nb):
    """The prep input of mivq_pq_encode: only the library can make it, on the GPU machine."""
    return Buf("prep", "in", nbytes=nb, late=lambda c: c.N.pq_prepare(c.t(C), nbits))


def pq_encode(n, d, M, nbits, flags, skew=0):
    def build(O):
        X, C = rows(n, d, 2), _codebook(M, nbits, d // M, 2)
        nb = _lib().mivq_pq_prep_bytes(d, M, nbits)
        return Call([In("x", X, skew=skew), n, d, M, nbits, In("centroids", C),
                     _prep_buf(C, nbits, nb), Ws("mivq_pq_encode_workspace_bytes", n, d, M, nbits),
                     Out("codes", n * _pq_code_size(M, nbits)), flags, None],
                    expect=lambda c: {"codes": c.O.pq_pack(c.O.pq_encode(X, C), nbits)})
    return build


add("mivq_pq_encode", "auto-filter-n130-d32-M2-b8", RAGGED, pq_encode(130, 32, 2, 8, PQ_AUTO))
add("mivq_pq_encode", "auto-filter-n1025-d32-M2-b8", RAGGED, pq_encode(1025, 32, 2, 8, PQ_AUTO))
add("mivq_pq_encode", "auto-filter-n1", RAGGED, pq_encode(1, 32, 2, 8, PQ_AUTO))
add("mivq_pq_encode", "force-exact-tiled-n65", RAGGED, pq_encode(65, 32, 2, 8, PQ_EXACT))
add("mivq_pq_encode", "legacy-mfma-n130", RAGGED, pq_encode(130, 32, 2, 8, PQ_LEGACY_MFMA))
add("mivq_pq_encode", "legacy-exact-n130", RAGGED, pq_encode(130, 32, 2, 8, PQ_EXACT | PQ_LEGACY_EXACT))
add("mivq_pq_encode", "generic-x-skew4-n65", RAGGED, pq_encode(65, 32, 2, 8, PQ_AUTO, skew=4))
add("mivq_pq_encode", "b4-M3-d21-code-ends-mid-word", EDGE, pq_encode(65, 21, 3, 4, PQ_AUTO))
add("mivq_pq_encode", "b3-M5-d35-code-ends-mid-word", EDGE, pq_encode(130, 35, 5, 3, PQ_AUTO))
add("mivq_pq_encode", "empty", EMPTY, pq_encode(0, 32, 2, 8, PQ_AUTO))


def pq_decode(n, d, M, nbits, skew=0):
    def build(O):
        C = _codebook(M, nbits, d // M, 3)
        u8 = rng(n, M, nbits).integers(0, 1 << nbits, (n, M)).astype(np.uint8)
        return Call([In("codes", O.pq_pack(u8, nbits)), n, d, M, nbits, In("centroids", C),
                     Out("out", n * d * 4, skew=skew), None],
                    expect=lambda c: {"out": c.O.pq_decode(u8, C)})
    return build


add("mivq_pq_decode", "vec-n130-d32-M2-b8", RAGGED, pq_decode(130, 32, 2, 8))
add("mivq_pq_decode", "scalar-out-skew4-n65", RAGGED, pq_decode(65, 32, 2, 8, skew=4))
add("mivq_pq_decode", "b4-M3-d21-n65", EDGE, pq_decode(65, 21, 3, 4))
add("mivq_pq_decode", "b3-M5-d35-n1025", EDGE, pq_decode(1025, 35, 5, 3))
add("mivq_pq_decode", "empty", EMPTY, pq_decode(0, 32, 2, 8))


def pq_unpack(n, M, nbits):
    def build(O):
        u8 = rng(n, M, nbits, 1).integers(0, 1 << nbits, (n, M)).astype(np.uint8)
        return Call([In("codes", O.pq_pack(u8, nbits)), n, M, nbits, Out("out", n * M), None],
                    expect=lambda c: {"out": u8})
    return build


add("mivq_pq_unpack", "b8-copy-n130-M3", RAGGED, pq_unpack(130, 3, 8))
add("mivq_pq_unpack", "b4-M3-n1025", EDGE, pq_unpack(1025, 3, 4))
add("mivq_pq_unpack", "b3-M5-n65", EDGE, pq_unpack(65, 5, 3))
add("mivq_pq_unpack", "empty", EMPTY, pq_unpack(0, 3, 4))


def _kmeans_ref(X, assign, C0, M, ksub):
    """Integer-valued rows: every fp32 sum is exact in any order, the quotient one rounding."""
    n, d = X.shape
    dsub = d // M
    C, counts = C0.copy(), np.zeros((M, ksub), np.int32)
    for m in range(M):
        for k in range(ksub):
            sel = np.flatnonzero(assign[:, m] == k)
            counts[m, k] = sel.size
            if sel.size:
                s = X[sel, m * dsub:(m + 1) * dsub].astype(np.float64).sum(0).astype(F32)
                C[m, k] = s / F32(sel.size)
    return C, counts


def kmeans_update(n, d, M, ksub):
    def build(O):
        X = int_rows(n, d, 4)
        r = rng(n, M, ksub)
        assign = r.integers(0, max(ksub - 1, 1), (n, M)).astype(np.uint8)  # the last cluster stays empty
        C0 = r.standard_normal((M, ksub, d // M)).astype(F32)
        cnt0 = r.integers(0, 9, (M, ksub)).astype(np.int32)
        C, counts = _kmeans_ref(X, assign, C0, M, ksub)
        return Call([In("x", X), n, d, M, ksub, In("assign", assign), InOut("centroids", C0), InOut("counts", cnt0), None],
                    expect=lambda c: {"centroids": C, "counts": counts},
                    empty_expect={"counts": np.zeros((M, ksub), np.int32)})
    return build


add("mivq_kmeans_update", "n130-d21-M3-k16", RAGGED, kmeans_update(130, 21, 3, 16))
add("mivq_kmeans_update", "n1025-d32-M2-k256", EDGE, kmeans_update(1025, 32, 2, 256))
add("mivq_kmeans_update", "empty", EMPTY, kmeans_update(0, 21, 3, 16))


# ------------------------------------------------------------------------------ OPQ
def _int_matrix(d, *seed):
    return int_rows(d, d, *seed, lim=4)


def opq_rotate(n, d, transpose):
    def build(O):
        X, A = int_rows(n, d, 5), _int_matrix(d, 5)
        want = (X.astype(np.int64) @ (A if transpose else A.T).astype(np.int64)).astype(F32)
        return Call([In("x", X), n, d, In("A", A), transpose, Out("y", n * d * 4), None],
                    expect=lambda c: {"y": want})
    return build


add("mivq_opq_rotate", "n65-d37-apply", RAGGED, opq_rotate(65, 37, 0))
add("mivq_opq_rotate", "n130-d64-reverse", RAGGED, opq_rotate(130, 64, 1))
add("mivq_opq_rotate", "n1-d7", EDGE, opq_rotate(1, 7, 0))
add("mivq_opq_rotate", "n1025-d130-reverse", EDGE, opq_rotate(1025, 130, 1))
add("mivq_opq_rotate", "empty", EMPTY, opq_rotate(0, 37, 0))


def opq_prepare(d, transpose):
    def build(O):
        A = rows(d, d, 6)
        nb = _lib().mivq_opq_prep_bytes(d)
        # no importable reference of the split f16 image: the wrapper's call on a fresh buffer
        return Call([In("A", A), d, transpose, Out("prep", nb), None],
                    expect=lambda c: {"prep": _np(c.N.opq_prepare(c.t(A), bool(transpose)))})
    return build


add("mivq_opq_prepare", "d64-apply", RAGGED, opq_prepare(64, 0))
add("mivq_opq_prepare", "d104-reverse", EDGE, opq_prepare(104, 1))


def opq_rotate_prepared(n, d, transpose):
    def build(O):
        X, A = int_rows(n, d, 7), _int_matrix(d, 7)
        nb = _lib().mivq_opq_prep_bytes(d)
        want = (X.astype(np.int64) @ (A if transpose else A.T).astype(np.int64)).astype(F32)
        prep = Buf("prep", "in", nbytes=nb, late=lambda c: c.N.opq_prepare(c.t(A), bool(transpose)))
        return Call([In("x", X), n, d, prep, Ws("mivq_opq_rotate_workspace_bytes", n, d), Out("y", n * d * 4), None],
                    expect=lambda c: {"y": want})
    return build


add("mivq_opq_rotate_prepared", "n130-d64-apply", RAGGED, opq_rotate_prepared(130, 64, 0))
add("mivq_opq_rotate_prepared", "n1025-d104-reverse", RAGGED, opq_rotate_prepared(1025, 104, 1))
add("mivq_opq_rotate_prepared", "n1-d64", EDGE, opq_rotate_prepared(1, 64, 0))
add("mivq_opq_rotate_prepared", "empty", EMPTY, opq_rotate_prepared(0, 64, 0))


def opq_gram(n, d):
    def build(O):
        X, Y = int_rows(n, d, 8), int_rows(n, d, 9)
        want = (X.astype(np.int64).T @ Y.astype(np.int64)).astype(np.float64)
        return Call([In("x", X), In("y", Y), n, d, Ws("mivq_opq_gram_workspace_bytes", n, d), Out("G", d * d * 8), None],
                    expect=lambda c: {"G": want}, empty_expect={"G": np.zeros((d, d))})
    return build


add("mivq_opq_gram", "splits3-n130-d37", RAGGED, opq_gram(130, 37))
add("mivq_opq_gram", "splits17-n1025-d64", RAGGED, opq_gram(1025, 64))
add("mivq_opq_gram", "one-split-n1-d7", EDGE, opq_gram(1, 7))
add("mivq_opq_gram", "empty", EMPTY, opq_gram(0, 37))


# ------------------------------------------------------------------------------ SQ
def _sq_fit(X):
    lo = X.min(axis=0)
    den = (X.max(axis=0) - lo) + X.dtype.type(1e-8)
    assert lo.dtype == den.dtype == X.dtype
    return lo, den


def _sq_code_bytes(n, d, nbits):
    return n * {4: (d + 1) // 2, 8: d, 16: 2 * d}[nbits]


def sq_encode(dt, n, d, nbits, skew=0):
    def build(O):
        X = rng(n, d, nbits, 10).standard_normal((max(n, 2), d)).astype(dt)
        lo, den = _sq_fit(X)
        X = X[:n]
        return Call([In("x", X, skew=skew), n, d, In("lo", lo), In("den", den), nbits,
                     Out("codes", _sq_code_bytes(n, d, nbits)), None],
                    expect=lambda c: {"codes": c.O.sq_encode(X, lo, den, nbits)})
    return build


def sq_decode(dt, n, d, nbits, skew=0):
    def build(O):
        X = rng(n, d, nbits, 11).standard_normal((max(n, 2), d)).astype(dt)
        lo, den = _sq_fit(X)
        L = (1 << nbits) - 1
        width = (d + 1) // 2 if nbits == 4 else d
        codes = rng(n, d, nbits, 12).integers(0, (256 if nbits == 4 else L + 1), (n, width))
        codes = codes.astype(np.uint16 if nbits == 16 else np.uint8)
        return Call([In("codes", codes), n, d, In("lo", lo), In("den", den), nbits,
                     Out("out", n * d * np.dtype(dt).itemsize, skew=skew), None],
                    expect=lambda c: {"out": c.O.sq_decode(codes, d, lo, den, nbits)})
    return build


for _dt, _sfx, _sk in ((np.float32, "f32", 4), (np.float64, "f64", 8)):
    for _fn, _mk, _op in (("encode", sq_encode, "x"), ("decode", sq_decode, "out")):
        _e = f"mivq_sq_{_fn}_{_sfx}"
        add(_e, "b8-d64-n130-aligned", RAGGED, _mk(_dt, 130, 64, 8))
        add(_e, f"b8-d64-n65-{_op}-skew{_sk}", RAGGED, _mk(_dt, 65, 64, 8, skew=_sk))
        add(_e, "b4-odd-d37-n65", EDGE, _mk(_dt, 65, 37, 4))
        add(_e, "b16-d100-n1025", EDGE, _mk(_dt, 1025, 100, 16))
        add(_e, "b4-d7-n1", EDGE, _mk(_dt, 1, 7, 4))
        add(_e, "empty", EMPTY, _mk(_dt, 0, 37, 8))


# ------------------------------------------------------------------------------ LVQ / LVQ2
def column_mean(n, d, skew=0):
    def build(O):
        X = rows(n, d, 13)
        return Call([In("x", X, skew=skew), n, d, Out("mean", d * 4), None], expect=lambda c: {"mean": LR.seq_mean(X)})
    return build


add("mivq_column_mean", "vec-n130-d64", RAGGED, column_mean(130, 64))
add("mivq_column_mean", "scalar-x-skew4-n65-d64", RAGGED, column_mean(65, 64, skew=4))
add("mivq_column_mean", "n1025-d37", RAGGED, column_mean(1025, 37))
add("mivq_column_mean", "n1-d7", EDGE, column_mean(1, 7))


def _lvq_rows(n, d, *seed):
    X = rows(max(n, 1), d, *seed) * F32(1.5) + F32(0.25)
    return X[:n], LR.seq_mean(X)


def lvq_encode(n, d, B, skew=0):
    def build(O):
        X, mu = _lvq_rows(n, d, 14)
        return Call([In("x", X, skew=skew), n, d, In("mu", mu), B, Out("codes", n * LR.code_size(d, B)), None],
                    expect=lambda c: {"codes": LR.encode(X, mu, B)})
    return build


def lvq_decode(n, d, B, skew=0):
    def build(O):
        X, mu = _lvq_rows(n, d, 15)
        codes = LR.encode(X, mu, B) if n else np.zeros((0, LR.code_size(d, B)), np.uint8)
        return Call([In("codes", codes), n, d, In("mu", mu), B, Out("out", n * d * 4, skew=skew), None],
                    expect=lambda c: {"out": LR.decode(codes, mu, B)})
    return build


for _fn, _mk, _op in (("encode", lvq_encode, "x"), ("decode", lvq_decode, "out")):
    _e = f"mivq_lvq_{_fn}"
    add(_e, "vec-b8-d64-n130", RAGGED, _mk(130, 64, 8))
    add(_e, f"scalar-{_op}-skew4-b8-d64-n65", RAGGED, _mk(65, 64, 8, skew=4))
    add(_e, "b3-d37-n65-code-size-22", EDGE, _mk(65, 37, 3))       # 14 index bytes + 8: not a multiple of 4
    add(_e, "b1-d7-n1", EDGE, _mk(1, 7, 1))
    add(_e, "b5-d130-n1025", EDGE, _mk(1025, 130, 5))
    add(_e, "empty", EMPTY, _mk(0, 37, 3))


def lvq2_encode(n, d, B1, B2, skew=0):
    def build(O):
        X, mu = _lvq_rows(n, d, 16)
        s1, s2 = L2.code_sizes(d, B1, B2)

        def want(c):
            c1, c2 = L2.encode2(X, mu, B1, B2)
            return {"codes1": c1, "codes2": c2}
        return Call([In("x", X, skew=skew), n, d, In("mu", mu), B1, B2, Out("codes1", n * s1), Out("codes2", n * s2), None],
                    expect=want)
    return build


def lvq2_decode(n, d, B1, B2, skew=0):
    def build(O):
        X, mu = _lvq_rows(n, d, 17)
        s1, s2 = L2.code_sizes(d, B1, B2)
        c1, c2 = L2.encode2(X, mu, B1, B2) if n else (np.zeros((0, s1), np.uint8), np.zeros((0, s2), np.uint8))
        return Call([In("codes1", c1), In("codes2", c2), n, d, In("mu", mu), B1, B2, Out("out", n * d * 4, skew=skew), None],
                    expect=lambda c: {"out": L2.decode2(c1, c2, mu, B1, B2)})
    return build


for _fn, _mk, _op in (("encode", lvq2_encode, "x"), ("decode", lvq2_decode, "out")):
    _e = f"mivq_lvq2_{_fn}"
    add(_e, "b8x8-d64-n130", RAGGED, _mk(130, 64, 8, 8))
    add(_e, f"{_op}-skew4-b4x4-d64-n65", RAGGED, _mk(65, 64, 4, 4, skew=4))
    add(_e, "b3x4-d37-n65-odd-code-sizes", EDGE, _mk(65, 37, 3, 4))   # 22 and 19 bytes
    add(_e, "b1x8-d7-n1", EDGE, _mk(1, 7, 1, 8))
    add(_e, "b5x4-d130-n1025", EDGE, _mk(1025, 130, 5, 4))
    add(_e, "empty", EMPTY, _mk(0, 37, 3, 4))


# ------------------------------------------------------------------------------ RaBitQ-1
def rabitq_code_check(d):
    """The comparison of test_rabitq_parity: sign bytes equal, the two factors within 1e-5."""
    nb = (d + 7) // 8

    def check(got, ref, what):
        got = got.reshape(-1, nb + 8)
        np.testing.assert_array_equal(got[:, :nb], ref[:, :nb], err_msg=what)
        fr, fg = ref[:, nb:].copy().view(F32), got[:, nb:].copy().view(F32)
        np.testing.assert_allclose(fg, fr, rtol=1e-5, atol=1e-5 * np.abs(fr).max(), err_msg=what)
    return check


def rabitq_encode(n, d, metric, centroid=True, skew=0):
    def build(O):
        X = rows(n, d, 18)
        c = rows(1, d, 19)[0] * F32(0.1) if centroid else None
        return Call([In("x", X, skew=skew), n, d, In("centroid", c) if centroid else None, metric,
                     Out("codes", n * ((d + 7) // 8 + 8)), None],
                    expect=lambda cx: {"codes": cx.O.rabitq_encode(X, c, metric)}, check={"codes": rabitq_code_check(d)})
    return build


add("mivq_rabitq_encode", "d64-n130-l2", RAGGED, rabitq_encode(130, 64, L2M))
add("mivq_rabitq_encode", "d37-n65-ip-code-size-13", EDGE, rabitq_encode(65, 37, IPM))
add("mivq_rabitq_encode", "d100-n1025-no-centroid", RAGGED, rabitq_encode(1025, 100, L2M, centroid=False))
add("mivq_rabitq_encode", "x-skew4-d64-n65", RAGGED, rabitq_encode(65, 64, L2M, skew=4))
add("mivq_rabitq_encode", "d7-n1", EDGE, rabitq_encode(1, 7, L2M))
add("mivq_rabitq_encode", "empty", EMPTY, rabitq_encode(0, 37, L2M))


def rabitq_decode(n, d, centroid=True, skew=0):
    def build(O):
        X = rows(n, d, 20)
        c = rows(1, d, 21)[0] * F32(0.1) if centroid else None
        codes = O.rabitq_encode(X, c, L2M)
        return Call([In("codes", codes), n, d, In("centroid", c) if centroid else None, Out("out", n * d * 4, skew=skew), None],
                    expect=lambda cx: {"out": cx.O.rabitq_decode(codes, d, c)})
    return build


add("mivq_rabitq_decode", "d64-n130", RAGGED, rabitq_decode(130, 64))
add("mivq_rabitq_decode", "d37-n65-code-size-13", EDGE, rabitq_decode(65, 37))
add("mivq_rabitq_decode", "d100-n1025-no-centroid", RAGGED, rabitq_decode(1025, 100, centroid=False))
add("mivq_rabitq_decode", "out-skew4-d64-n65", RAGGED, rabitq_decode(65, 64, skew=4))
add("mivq_rabitq_decode", "empty", EMPTY, rabitq_decode(0, 37))


# ------------------------------------------------------------------------------ Extended RaBitQ
# normalize / quantize: the rule module states them with error bounds on the norms and on t, which
# the device sums in another order; the byte-level reference here is the wrapper's call on the same
# inputs (listed in the test module's docstring).  dequantize / finish have bit-exact rules.
def erq_normalize(n, d, f64):
    def build(O):
        X = rows(n, d, 22).astype(np.float64 if f64 else F32)
        cen = rows(1, d, 23)[0].astype(np.float64) * 0.1

        def want(c):
            o, nrm = c.N.extrabitq_normalize(c.t(X), c.t(cen))
            return {"o": _np(o), "nrm": _np(nrm)}
        return Call([In("x", X), int(f64), n, d, In("centroid", cen), Out("o", n * d * 8), Out("nrm", n * 8), None],
                    expect=want)
    return build


add("mivq_extrabitq_normalize", "f32-n130-d37", RAGGED, erq_normalize(130, 37, False))
add("mivq_extrabitq_normalize", "f64-n65-d100", RAGGED, erq_normalize(65, 100, True))
add("mivq_extrabitq_normalize", "f32-n1025-d64", EDGE, erq_normalize(1025, 64, False))
add("mivq_extrabitq_normalize", "f32-n1-d7", EDGE, erq_normalize(1, 7, False))
add("mivq_extrabitq_normalize", "empty", EMPTY, erq_normalize(0, 37, False))


def _erq_codes(n, d, B, *seed):
    r = rng(n, d, B, *seed)
    idx = r.integers(0, 1 << B, (n, d))
    return ES.pack(idx, r.uniform(0.5, 2.0, n).astype(F32), r.uniform(0.5, 1.5, n).astype(F32), B)


def erq_quantize(n, d, B):
    def build(O):
        lv = RE.synthetic_levels(B)
        s = rng(n, d, B, 24).standard_normal((n, d)) / np.sqrt(d)
        nrm = rng(n, d, B, 25).uniform(0.5, 2.0, n)

        def want(c):
            return {"codes": _np(c.N.extrabitq_quantize(c.t(s), c.t(lv), B, c.t(nrm)))}
        return Call([In("s_raw", s), n, d, In("levels", lv), B, In("nrm", nrm), Out("codes", n * ES.code_size(d, B)), None],
                    expect=want)
    return build


add("mivq_extrabitq_quantize", "b4-n130-d64", RAGGED, erq_quantize(130, 64, 4))
add("mivq_extrabitq_quantize", "b3-n65-d37-code-size-22", EDGE, erq_quantize(65, 37, 3))
add("mivq_extrabitq_quantize", "b8-n1025-d100", RAGGED, erq_quantize(1025, 100, 8))
add("mivq_extrabitq_quantize", "b1-n1-d7", EDGE, erq_quantize(1, 7, 1))
add("mivq_extrabitq_quantize", "empty", EMPTY, erq_quantize(0, 37, 3))


def erq_dequantize(n, d, B):
    def build(O):
        lv = RE.synthetic_levels(B)
        codes = _erq_codes(n, d, B, 26)
        return Call([In("codes", codes), n, d, In("levels", lv), B, Out("o_hat", n * d * 8), None],
                    expect=lambda c: {"o_hat": RE.dequantize_ref(codes, lv, d, B)})
    return build


add("mivq_extrabitq_dequantize", "b4-n130-d64", RAGGED, erq_dequantize(130, 64, 4))
add("mivq_extrabitq_dequantize", "b3-n65-d37-code-size-22", EDGE, erq_dequantize(65, 37, 3))
add("mivq_extrabitq_dequantize", "b8-n1025-d100", RAGGED, erq_dequantize(1025, 100, 8))
add("mivq_extrabitq_dequantize", "empty", EMPTY, erq_dequantize(0, 37, 3))


def erq_finish(n, d, B):
    def build(O):
        y = rng(n, d, B, 27).standard_normal((n, d))
        cen = rows(1, d, 28)[0].astype(np.float64) * 0.1
        codes = _erq_codes(n, d, B, 29)
        return Call([In("y", y), n, d, In("codes", codes), B, In("centroid", cen), Out("out", n * d * 4), None],
                    expect=lambda c: {"out": RE.finish_ref(y, codes, cen, B)})
    return build


add("mivq_extrabitq_finish", "b4-n130-d64", RAGGED, erq_finish(130, 64, 4))
add("mivq_extrabitq_finish", "b3-n65-d37-code-size-22", EDGE, erq_finish(65, 37, 3))
add("mivq_extrabitq_finish", "b8-n1025-d100", RAGGED, erq_finish(1025, 100, 8))
add("mivq_extrabitq_finish", "empty", EMPTY, erq_finish(0, 37, 3))


def erq_rotate(n, d, transpose):
    def build(O):
        o = int_rows(n, d, 30, lim=1024, dtype=np.float64)
        P = int_rows(d, d, 31, lim=1024, dtype=np.float64)
        want = (o.astype(np.int64) @ (P.T if transpose else P).astype(np.int64)).astype(np.float64)
        return Call([In("o", o), n, d, In("P", P), transpose, Out("s", n * d * 8), None], expect=lambda c: {"s": want})
    return build


add("mivq_extrabitq_rotate", "generic-n130-d100", RAGGED, erq_rotate(130, 100, 0))
add("mivq_extrabitq_rotate", "generic-n65-d37-transpose", RAGGED, erq_rotate(65, 37, 1))
add("mivq_extrabitq_rotate", "fast-n129-d160", RAGGED, erq_rotate(129, 160, 0))
add("mivq_extrabitq_rotate", "fast-n5-d32-transpose", EDGE, erq_rotate(5, 32, 1))
add("mivq_extrabitq_rotate", "generic-n1-d7", EDGE, erq_rotate(1, 7, 0))
add("mivq_extrabitq_rotate", "empty", EMPTY, erq_rotate(0, 37, 0))


# ------------------------------------------------------------------------------ rank-aware
def ra_state(d, seed, packing="dense"):
    """Widths 0..8 cycling over the dimensions, the two widest first."""
    bits = np.array([(8, 5, 3, 0, 1, 4, 2, 7, 6)[j % 9] for j in range(d)], np.int64)
    return RA.synthetic_state(bits, packing, seed)


def ra_tables(st):
    from haag_vq import _native

    return _native.rankaware_tables(st.cb, st.bits, st.pos, st.code_size)


def ra_center(n, d, f64):
    def build(O):
        X = rows(n, d, 32).astype(np.float64 if f64 else F32)
        mu = rows(1, d, 33)[0].astype(np.float64)
        return Call([In("x", X), int(f64), n, d, In("mu", mu), Out("xc", n * d * 8), None],
                    expect=lambda c: {"xc": X.astype(np.float64) - mu})
    return build


add("mivq_rankaware_center", "f32-n130-d37", RAGGED, ra_center(130, 37, False))
add("mivq_rankaware_center", "f64-n1025-d100", RAGGED, ra_center(1025, 100, True))
add("mivq_rankaware_center", "f32-n1-d7", EDGE, ra_center(1, 7, False))
add("mivq_rankaware_center", "empty", EMPTY, ra_center(0, 37, False))


def ra_quantize(n, d, packing):
    def build(O):
        st = ra_state(d, 34, packing)
        lv, lv_off, pos, width = ra_tables(st)
        Y = rng(n, d, 35).standard_normal((n, d)) * 2.0
        return Call([In("y", Y), n, d, In("lv", lv), In("lv_off", lv_off), In("pos", pos), In("width", width),
                     st.code_size, Out("codes", n * st.code_size), None],
                    expect=lambda c: {"codes": RA.pack(RA.indices(Y, st), st)})
    return build


def ra_dequantize(n, d, packing):
    def build(O):
        st = ra_state(d, 36, packing)
        lv, lv_off, pos, width = ra_tables(st)
        codes = rng(n, d, 37).integers(0, 256, (n, st.code_size)).astype(np.uint8)  # any bytes decode
        return Call([In("codes", codes), n, d, In("lv", lv), In("lv_off", lv_off), In("pos", pos), In("width", width),
                     st.code_size, Out("y_hat", n * d * 8), None],
                    expect=lambda c: {"y_hat": RA.lookup(RA.unpack(codes, st), st)})
    return build


for _fn, _mk in (("quantize", ra_quantize), ("dequantize", ra_dequantize)):
    _e = f"mivq_rankaware_{_fn}"
    add(_e, "dense-n130-d37-code-size-19", EDGE, _mk(130, 37, "dense"))   # 148 bits: the row ends mid-word
    add(_e, "byte-n65-d100", RAGGED, _mk(65, 100, "byte"))
    add(_e, "dense-n1025-d64", RAGGED, _mk(1025, 64, "dense"))
    add(_e, "dense-n1-d7", EDGE, _mk(1, 7, "dense"))
    add(_e, "empty", EMPTY, _mk(0, 37, "dense"))


def ra_finish(n, d):
    def build(O):
        z = rng(n, d, 38).standard_normal((n, d))
        mu = rows(1, d, 39)[0].astype(np.float64)
        return Call([In("z", z), n, d, In("mu", mu), Out("out", n * d * 4), None],
                    expect=lambda c: {"out": (z + mu).astype(F32)})
    return build


add("mivq_rankaware_finish", "n130-d37", RAGGED, ra_finish(130, 37))
add("mivq_rankaware_finish", "n1025-d100", RAGGED, ra_finish(1025, 100))
add("mivq_rankaware_finish", "n1-d7", EDGE, ra_finish(1, 7))
add("mivq_rankaware_finish", "empty", EMPTY, ra_finish(0, 37))


# ------------------------------------------------------------------------------ codebook1d
CB_EXACT, CB_LLOYD = 0, 1
CB_DRAWS = 320


def codebook1d(n, widths, method, dims_at_once):
    """Every width > 0: a width-0 dimension's level and sse entries are documented as not written,
    so they cannot be part of an all-bytes-written check."""
    def build(O):
        from haag_vq import _native

        d = len(widths)
        width, lv_off = _native.codebook1d_tables(widths)
        cols = np.sort(rng(n, d, method).standard_normal((d, n)).astype(F32) * F32(1.7), axis=1)
        draws = np.array(_native.mt19937_64(0, CB_DRAWS), dtype=np.uint64)
        lloyd = method == CB_LLOYD

        def want(c):
            levels, sse = np.zeros(int(lv_off[-1]), F32), np.zeros(d, np.float64)
            for j in range(d):
                lv, s = CB.fit(cols[j], int(width[j]), "lloyd" if lloyd else "exact")
                levels[lv_off[j]:lv_off[j + 1]], sse[j] = lv, s
            return {"levels": levels, "sse": sse}
        return Call([In("cols", cols), n, d, Host("width", width), Host("lv_off", lv_off), method,
                     In("draws", draws) if lloyd else None, CB_DRAWS if lloyd else 0,
                     Ws("mivq_codebook1d_workspace_bytes", n, max(widths), method, dims_at_once),
                     Out("levels", int(lv_off[-1]) * 4), Out("sse", d * 8), None], expect=want)
    return build


add("mivq_codebook1d_fit", "exact-n65-one-slot", RAGGED, codebook1d(65, [3, 2, 1], CB_EXACT, 1))
add("mivq_codebook1d_fit", "exact-n130-all-slots", RAGGED, codebook1d(130, [2, 4, 1], CB_EXACT, 3))
add("mivq_codebook1d_fit", "lloyd-n65-one-slot", RAGGED, codebook1d(65, [3, 2, 1], CB_LLOYD, 1))
add("mivq_codebook1d_fit", "lloyd-n130-all-slots", RAGGED, codebook1d(130, [2, 4, 1], CB_LLOYD, 3))
add("mivq_codebook1d_fit", "exact-n5-fewer-rows-than-levels", EDGE, codebook1d(5, [3, 1], CB_EXACT, 2))
add("mivq_codebook1d_fit", "empty", EMPTY, codebook1d(0, [3, 2, 1], CB_EXACT, 1))
