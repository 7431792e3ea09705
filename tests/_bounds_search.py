"""Buffer-contract cases of the searches, the re-ranking entries, the top-k / IVF building blocks
and the IVF searches.  See tests/_bounds.py for what a case is."""

from __future__ import annotations

import numpy as np

import _extrabitq_search_rule as ES
import _ivf_listpq_rule as LP
import _ivf_quantized_rule as IQ
import _ivf_rabitq_rule as IR
import _lvq2_rule as L2
import _lvq_rule as LR
import _rabitq_encode_rule as RE
import _rankaware_rule as RA
import _rerank_rule as RR
from _bounds import EDGE, EMPTY, F32, NO_ID, RAGGED, Call, In, InOut, Out, Ws, add, pad_topk, rng, rows, sentinel
from _bounds_codec import _codebook, _sq_fit, ra_state, ra_tables

L2M, IPM = 1, 0
ADC_AUTO, ADC_EXACT, ADC_SMALL_RERUN_GRID = 0, 1, 4
OFF = 1000  # id_offset of the cases that use one


def topk(nq, k):
    return [Out("dists", nq * k * 4), Out("ids", nq * k * 4)]


def flat_ref(O, Q, X, k, metric, off=0):
    """oracle.flat_search padded to k > n."""
    nq = Q.shape[0]
    if X.shape[0] == 0:
        return sentinel(nq, k)
    dd, ii = O.flat_search(Q, X, min(k, X.shape[0]), metric, off)
    dd, ii = pad_topk(dd, ii, k)
    return {"dists": dd, "ids": ii}


# ------------------------------------------------------------------------------ ADC
def adc_lut(nq, d, M, nbits, metric, skew=0):
    def build(O):
        Q, C = rows(nq, d, 40), _codebook(M, nbits, d // M, 40)
        return Call([In("q", Q), nq, d, M, nbits, In("centroids", C, skew=skew), metric,
                     Out("lut", nq * M * (1 << nbits) * 4), None],
                    expect=lambda c: {"lut": c.O.adc_lut(Q, C, metric)})
    return build


add("mivq_adc_lut", "vec-nq3-d32-M2-b8-l2", RAGGED, adc_lut(3, 32, 2, 8, L2M))
add("mivq_adc_lut", "generic-centroids-skew4-nq17", RAGGED, adc_lut(17, 32, 2, 8, IPM, skew=4))
add("mivq_adc_lut", "nq1-d21-M3-b4", EDGE, adc_lut(1, 21, 3, 4, L2M))
add("mivq_adc_lut", "nq17-d35-M5-b3-ip", EDGE, adc_lut(17, 35, 5, 3, IPM))
add("mivq_adc_lut", "empty", EMPTY, adc_lut(0, 32, 2, 8, L2M))


def adc_search(nq, n, M, nbits, k, flags, off=0):
    def build(O):
        r = rng(nq, n, M, nbits, k)
        lut = r.standard_normal((nq, M, 1 << nbits)).astype(F32)
        codes = r.integers(0, 1 << nbits, (n, M)).astype(np.uint8)

        def want(c):
            if n == 0:
                return sentinel(nq, k)
            dd, ii = pad_topk(*c.O.adc_search(lut, codes, min(k, n), off), k)
            return {"dists": dd, "ids": ii}
        return Call([In("lut", lut), nq, In("codes", codes), n, M, nbits, k, off,
                     Ws("mivq_adc_search_workspace_bytes", nq, n, M, nbits, k), *topk(nq, k), flags, None], expect=want)
    return build


add("mivq_adc_search", "auto-filtered-nq3-n1025-M16-k10", RAGGED, adc_search(3, 1025, 16, 8, 10, ADC_AUTO))
add("mivq_adc_search", "force-exact-nq3-n1025-M16-k10", RAGGED, adc_search(3, 1025, 16, 8, 10, ADC_EXACT))
add("mivq_adc_search", "filtered-small-rerun-grid-nq3-n1025-M16-k10", RAGGED,
    adc_search(3, 1025, 16, 8, 10, ADC_SMALL_RERUN_GRID))
add("mivq_adc_search", "auto-filtered-nq17-n130-M32-k1", EDGE, adc_search(17, 130, 32, 8, 1, ADC_AUTO, OFF))
add("mivq_adc_search", "scan-nq17-n130-M3-b4-k65", EDGE, adc_search(17, 130, 3, 4, 65, ADC_AUTO))
add("mivq_adc_search", "scan-nq1-n65-M5-b3-k256-above-n", EDGE, adc_search(1, 65, 5, 3, 256, ADC_AUTO, OFF))
add("mivq_adc_search", "empty", EMPTY, adc_search(0, 0, 16, 8, 10, ADC_AUTO))


# ------------------------------------------------------------------------------ the exact searches
def flat_search(nq, n, d, k, metric, off=0, skew=0):
    def build(O):
        Q, X = rows(nq, d, 41), rows(n, d, 42)
        return Call([In("q", Q), nq, In("x", X, skew=skew), n, d, metric, k, off,
                     Ws("mivq_flat_search_workspace_bytes", nq, n, d, k), *topk(nq, k), None],
                    expect=lambda c: flat_ref(c.O, Q, X, k, metric, off))
    return build


add("mivq_flat_search", "scan-nq3-n130-d37-k10", RAGGED, flat_search(3, 130, 37, 10, L2M))
add("mivq_flat_search", "scan-x-skew4-nq3-n130-d64-k10", RAGGED, flat_search(3, 130, 64, 10, L2M, skew=4))
add("mivq_flat_search", "scan-nq1-n1025-d64-k65-ip", EDGE, flat_search(1, 1025, 64, 65, IPM, OFF))
add("mivq_flat_search", "scan-nq17-n65-d7-k256-above-n", EDGE, flat_search(17, 65, 7, 256, L2M))
add("mivq_flat_search", "tiled-nq17-n4100-d100-k10", RAGGED, flat_search(17, 4100, 100, 10, L2M))
add("mivq_flat_search", "tiled-nq16-n4096-d64-k256", EDGE, flat_search(16, 4096, 64, 256, IPM, OFF))
add("mivq_flat_search", "scan-k1-nq3-n130-d130", EDGE, flat_search(3, 130, 130, 1, L2M))
add("mivq_flat_search", "empty", EMPTY, flat_search(0, 0, 37, 10, L2M))


def _sq_store(n, d, nbits, *seed):
    X = rows(max(n, 2), d, *seed)
    lo, den = _sq_fit(X)
    return _sq_rows(X[:n], lo, den, nbits), lo, den


def _sq_rows(X, lo, den, nbits):
    if X.shape[0] == 0:
        w, dt = IQ.code_shape("sq", nbits, X.shape[1])
        return np.zeros((0, w), dt)
    return IQ.sq_rows(X, lo, den, nbits)


def sq_flat_search(nq, n, d, nbits, k, metric, off=0, skew=0):
    def build(O):
        Q = rows(nq, d, 43)
        codes, lo, den = _sq_store(n, d, nbits, 44)
        return Call([In("q", Q), nq, In("codes", codes, skew=skew), n, d, In("lo", lo), In("den", den), nbits, metric, k,
                     off, Ws("mivq_sq_flat_search_workspace_bytes", nq, n, d, k), *topk(nq, k), None],
                    expect=lambda c: flat_ref(c.O, Q, RR.dequant("sq", nbits, codes, (lo, den), d), k, metric, off))
    return build


add("mivq_sq_flat_search", "scan-b8-nq3-n130-d64-k10", RAGGED, sq_flat_search(3, 130, 64, 8, 10, L2M))
add("mivq_sq_flat_search", "scan-b4-odd-d37-nq3-n65-k65", EDGE, sq_flat_search(3, 65, 37, 4, 65, IPM, OFF))
add("mivq_sq_flat_search", "scan-b16-nq1-n1025-d100-k1", EDGE, sq_flat_search(1, 1025, 100, 16, 1, L2M))
add("mivq_sq_flat_search", "scan-codes-skew4-b8-nq17-n130-d64-k256-above-n", EDGE,
    sq_flat_search(17, 130, 64, 8, 256, L2M, skew=4))
add("mivq_sq_flat_search", "tiled-b8-nq17-n4100-d37-k10", RAGGED, sq_flat_search(17, 4100, 37, 8, 10, L2M))
add("mivq_sq_flat_search", "empty", EMPTY, sq_flat_search(0, 0, 37, 8, 10, L2M))


def rabitq_flat_search(nq, n, d, k, metric, centroid=True, off=0):
    def build(O):
        Q, X = rows(nq, d, 45), rows(n, d, 46)
        cen = rows(1, d, 47)[0] * F32(0.1) if centroid else None
        codes = O.rabitq_encode(X, cen, metric)
        return Call([In("q", Q), nq, In("codes", codes), n, d, In("centroid", cen) if centroid else None, metric, k, off,
                     Ws("mivq_rabitq_flat_search_workspace_bytes", nq, n, d, k), *topk(nq, k), None],
                    expect=lambda c: flat_ref(c.O, Q, c.O.rabitq_decode(codes, d, cen), k, metric, off))
    return build


add("mivq_rabitq_flat_search", "scan-nq3-n130-d64-k10", RAGGED, rabitq_flat_search(3, 130, 64, 10, L2M))
add("mivq_rabitq_flat_search", "scan-nq3-n65-d37-k65-code-size-13", EDGE, rabitq_flat_search(3, 65, 37, 65, IPM, off=OFF))
add("mivq_rabitq_flat_search", "scan-nq1-n130-d100-k256-above-n-no-centroid", EDGE,
    rabitq_flat_search(1, 130, 100, 256, L2M, centroid=False))
add("mivq_rabitq_flat_search", "tiled-nq17-n4100-d37-k10", RAGGED, rabitq_flat_search(17, 4100, 37, 10, L2M))
add("mivq_rabitq_flat_search", "empty", EMPTY, rabitq_flat_search(0, 0, 37, 10, L2M))


def _lvq_store(n, d, B, *seed):
    X = rows(max(n, 1), d, *seed) * F32(1.5) + F32(0.25)
    mu = LR.seq_mean(X)
    codes = LR.encode(X[:n], mu, B) if n else np.zeros((0, LR.code_size(d, B)), np.uint8)
    return codes, mu


def lvq_flat_search(nq, n, d, B, k, metric, off=0, skew=0):
    def build(O):
        Q = rows(nq, d, 48)
        codes, mu = _lvq_store(n, d, B, 49)
        return Call([In("q", Q), nq, In("codes", codes, skew=skew), n, d, In("mu", mu), B, metric, k, off,
                     Ws("mivq_lvq_flat_search_workspace_bytes", nq, n, d, k), *topk(nq, k), None],
                    expect=lambda c: flat_ref(c.O, Q, LR.decode(codes, mu, B) if n else np.zeros((0, d), F32), k, metric,
                                              off))
    return build


add("mivq_lvq_flat_search", "scan-8B-loads-b8-nq3-n130-d64-k10", RAGGED, lvq_flat_search(3, 130, 64, 8, 10, L2M))
add("mivq_lvq_flat_search", "scan-4B-loads-b4-nq3-n130-d40-k10", RAGGED, lvq_flat_search(3, 130, 40, 4, 10, L2M))
add("mivq_lvq_flat_search", "scan-bytes-b3-d37-nq3-n65-k65-code-size-22", EDGE,
    lvq_flat_search(3, 65, 37, 3, 65, IPM, OFF))
add("mivq_lvq_flat_search", "scan-codes-skew1-b8-nq1-n130-d64-k256-above-n", EDGE,
    lvq_flat_search(1, 130, 64, 8, 256, L2M, skew=1))
add("mivq_lvq_flat_search", "tiled-b5-nq17-n4100-d37-k10", RAGGED, lvq_flat_search(17, 4100, 37, 5, 10, L2M))
add("mivq_lvq_flat_search", "empty", EMPTY, lvq_flat_search(0, 0, 37, 3, 10, L2M))


def _erq_store(n, d, B, *seed):
    r = rng(n, d, B, *seed)
    return ES.pack(r.integers(0, 1 << B, (n, d)), r.uniform(0.5, 2.0, n).astype(F32),
                   r.uniform(0.5, 1.5, n).astype(F32), B)


def erq_flat_search(nq, n, d, B, k, metric, off=0):
    def build(O):
        Q = rows(nq, d, 50)
        lv = RE.synthetic_levels(B)
        codes = _erq_store(n, d, B, 51)
        return Call([In("qy", Q), nq, In("codes", codes), n, d, In("levels", lv), B, metric, k, off,
                     Ws("mivq_extrabitq_flat_search_workspace_bytes", nq, n, d, k), *topk(nq, k), None],
                    expect=lambda c: flat_ref(c.O, Q, ES.y_hat(codes, lv, d, B), k, metric, off))
    return build


add("mivq_extrabitq_flat_search", "scan-b4-nq3-n130-d64-k10", RAGGED, erq_flat_search(3, 130, 64, 4, 10, L2M))
add("mivq_extrabitq_flat_search", "scan-b3-d37-nq3-n65-k65-code-size-22", EDGE, erq_flat_search(3, 65, 37, 3, 65, IPM, OFF))
add("mivq_extrabitq_flat_search", "scan-b8-nq1-n130-d100-k256-above-n", EDGE, erq_flat_search(1, 130, 100, 8, 256, L2M))
add("mivq_extrabitq_flat_search", "tiled-b2-nq17-n4100-d37-k10", RAGGED, erq_flat_search(17, 4100, 37, 2, 10, L2M))
add("mivq_extrabitq_flat_search", "empty", EMPTY, erq_flat_search(0, 0, 37, 3, 10, L2M))


def ra_flat_search(nq, n, d, k, metric, packing="dense", off=0):
    def build(O):
        st = ra_state(d, 52, packing)
        lv, lv_off, pos, width = ra_tables(st)
        lv32 = lv.astype(F32)
        Q = rows(nq, d, 53)
        codes = rng(n, d, 54).integers(0, 256, (n, st.code_size)).astype(np.uint8)

        def want(c):
            Y = RA.lookup(RA.unpack(codes, st), st).astype(F32) if n else np.zeros((0, d), F32)
            return flat_ref(c.O, Q, Y, k, metric, off)
        return Call([In("qy", Q), nq, In("codes", codes), n, d, In("lv32", lv32), In("lv_off", lv_off), In("pos", pos),
                     In("width", width), st.code_size, metric, k, off,
                     Ws("mivq_rankaware_flat_search_workspace_bytes", nq, n, d, st.code_size, k), *topk(nq, k), None],
                    expect=want)
    return build


add("mivq_rankaware_flat_search", "scan-dense-nq3-n130-d37-k10-code-size-19", RAGGED, ra_flat_search(3, 130, 37, 10, L2M))
add("mivq_rankaware_flat_search", "scan-byte-nq3-n65-d100-k65", EDGE, ra_flat_search(3, 65, 100, 65, IPM, "byte", OFF))
add("mivq_rankaware_flat_search", "scan-nq1-n130-d7-k256-above-n", EDGE, ra_flat_search(1, 130, 7, 256, L2M))
add("mivq_rankaware_flat_search", "tiled-nq17-n4100-d37-k10", RAGGED, ra_flat_search(17, 4100, 37, 10, L2M))
add("mivq_rankaware_flat_search", "empty", EMPTY, ra_flat_search(0, 0, 37, 10, L2M))


# ------------------------------------------------------------------------------ RaBitQ estimator search
def rabitq_search(nq, n, d, qb, k, metric, off=0):
    def build(O):
        Q, X = rows(nq, d, 55), rows(n, d, 56)
        cen = rows(1, d, 57)[0] * F32(0.1)
        codes = O.rabitq_encode(X, cen, metric)

        def want(c):
            if n == 0:
                return sentinel(nq, k)
            dd, ii = c.O.topk_rows(c.O.rabitq_est(codes, d, Q, cen, qb, metric), k)
            live = ii != NO_ID
            return {"dists": dd, "ids": np.where(live, ii + np.uint32(off), ii).astype(np.uint32)}
        return Call([In("codes", codes), n, d, In("centroid", cen), In("q", Q), nq, qb, metric, k, off,
                     Ws("mivq_rabitq_search_workspace_bytes", nq, n, d, k), *topk(nq, k), None], expect=want)
    return build


add("mivq_rabitq_search", "mfma-qb4-nq3-n130-d64-k10", RAGGED, rabitq_search(3, 130, 64, 4, 10, L2M))
add("mivq_rabitq_search", "generic-qb4-nq3-n65-d37-k65", EDGE, rabitq_search(3, 65, 37, 4, 65, IPM, OFF))
add("mivq_rabitq_search", "generic-qb0-nq17-n130-d64-k1", EDGE, rabitq_search(17, 130, 64, 0, 1, L2M))
add("mivq_rabitq_search", "mfma-qb8-nq17-n1025-d32-k256", EDGE, rabitq_search(17, 1025, 32, 8, 256, L2M))
add("mivq_rabitq_search", "mfma-qb4-nq1-n65-d64-k256-above-n", EDGE, rabitq_search(1, 65, 64, 4, 256, L2M))
# d % 512 == 0: the multi-query kernel; past 8192 rows its screened blocks, whose per-query counters
# live in the workspace
add("mivq_rabitq_search", "multi-query-dense-qb4-nq3-n1025-d512-k10", RAGGED, rabitq_search(3, 1025, 512, 4, 10, L2M))
add("mivq_rabitq_search", "multi-query-screened-qb4-nq3-n9000-d512-k10", RAGGED, rabitq_search(3, 9000, 512, 4, 10, L2M))
add("mivq_rabitq_search", "multi-query-screened-qb4-nq33-n10000-d512-k65", EDGE,
    rabitq_search(33, 10000, 512, 4, 65, IPM, OFF))
# more than 64 queries: 128 queries per workgroup, its own LDS size and grid
add("mivq_rabitq_search", "multi-query-128-dense-qb4-nq65-n1025-d512-k10", RAGGED, rabitq_search(65, 1025, 512, 4, 10, L2M))
add("mivq_rabitq_search", "multi-query-128-screened-qb4-nq65-n9000-d512-k10", RAGGED,
    rabitq_search(65, 9000, 512, 4, 10, L2M, OFF))
add("mivq_rabitq_search", "empty", EMPTY, rabitq_search(0, 0, 37, 4, 10, L2M))


# ------------------------------------------------------------------------------ re-ranking
def _cand(nq, r, n, off, *seed):
    """Distinct live ids where n >= r, else with repeats; three dead slots per query."""
    g = rng(nq, r, n, *seed)
    out = np.empty((nq, r), np.uint32)
    for a in range(nq):
        row = (g.permutation(n)[:r] if n >= r else g.integers(0, max(n, 1), r)).astype(np.int64) + off
        if r > 3:
            row[g.permutation(r)[:3]] = [NO_ID, off + n, max(off - 1, 0) if off else NO_ID]
        out[a] = row.astype(np.uint32)
    return out


def _rr_want(Q, cand, xh, off, metric, k):
    dd, ii = RR.rerank(Q, cand, xh, off, metric, k)
    return {"dists": dd, "ids": ii}


def rerank(kind, nq, r, n, d, bits, k, metric, off=0):
    """kind f32 / sq / lvq; r <= 256 is one slice of the candidate list, r > 256 several."""
    def build(O):
        Q, X = rows(nq, d, 58), rows(max(n, 2), d, 59) * F32(1.5)
        if kind == "f32":
            store, params = X[:n], ()
        elif kind == "sq":
            lo, den = _sq_fit(X)
            store, params = _sq_rows(X[:n], lo, den, bits), (lo, den)
        else:
            mu = LR.seq_mean(X)
            store = LR.encode(X[:n], mu, bits) if n else np.zeros((0, LR.code_size(d, bits)), np.uint8)
            params = (mu,)
        cand = _cand(nq, r, n, off, 60)
        mid = [In("store", store), n, d] + [In(nm, p) for nm, p in zip(("lo", "den") if kind == "sq" else ("mu",), params)]
        if kind != "f32":
            mid.append(bits)

        def want(c):
            xh = RR.dequant(kind, bits, store, params, d) if n else np.zeros((0, d), F32)
            return _rr_want(Q, cand, xh, off, metric, k)
        return Call([In("q", Q), nq, In("cand", cand), r, *mid, metric, k, off,
                     Ws(f"mivq_rerank_{kind}_workspace_bytes", nq, r, k), *topk(nq, k), None], expect=want)
    return build


for _kind, _bits, _odd in (("f32", 0, 0), ("sq", 8, 4), ("lvq", 8, 3)):
    _e = f"mivq_rerank_{_kind}"
    add(_e, "one-slice-nq3-r40-n300-d64-k10", RAGGED, rerank(_kind, 3, 40, 300, 64, _bits, 10, L2M))
    add(_e, "slices-nq3-r300-n1025-d37-k65", RAGGED, rerank(_kind, 3, 300, 1025, 37, _odd or _bits, 65, IPM, OFF))
    add(_e, "one-slice-nq17-r10-n65-d7-k256-above-r", EDGE, rerank(_kind, 17, 10, 65, 7, _odd or _bits, 256, L2M))
    add(_e, "one-slice-nq1-r1-n130-d100-k1", EDGE, rerank(_kind, 1, 1, 130, 100, _bits, 1, L2M, OFF))
    add(_e, "empty", EMPTY, rerank(_kind, 0, 40, 0, 37, _odd or _bits, 10, L2M))
add("mivq_rerank_sq", "one-slice-b16-nq3-r40-n130-d37-k10", EDGE, rerank("sq", 3, 40, 130, 37, 16, 10, L2M))


def rerank_lvq2(nq, r, n, d, B1, B2, k, metric, off=0):
    def build(O):
        Q, X = rows(nq, d, 61), rows(max(n, 2), d, 62) * F32(1.5)
        mu = LR.seq_mean(X)
        s1, s2 = L2.code_sizes(d, B1, B2)
        c1, c2 = L2.encode2(X[:n], mu, B1, B2) if n else (np.zeros((0, s1), np.uint8), np.zeros((0, s2), np.uint8))
        cand = _cand(nq, r, n, off, 63)

        def want(c):
            xh = L2.decode2(c1, c2, mu, B1, B2) if n else np.zeros((0, d), F32)
            return _rr_want(Q, cand, xh, off, metric, k)
        return Call([In("q", Q), nq, In("cand", cand), r, In("codes1", c1), In("codes2", c2), n, d, In("mu", mu), B1, B2,
                     metric, k, off, Ws("mivq_rerank_lvq2_workspace_bytes", nq, r, k), *topk(nq, k), None], expect=want)
    return build


add("mivq_rerank_lvq2", "one-slice-b8x8-nq3-r40-n300-d64-k10", RAGGED, rerank_lvq2(3, 40, 300, 64, 8, 8, 10, L2M))
add("mivq_rerank_lvq2", "slices-b3x4-nq3-r300-n1025-d37-k65-odd-code-sizes", RAGGED,
    rerank_lvq2(3, 300, 1025, 37, 3, 4, 65, IPM, OFF))
add("mivq_rerank_lvq2", "one-slice-b1x8-nq17-r10-n65-d7-k256-above-r", EDGE, rerank_lvq2(17, 10, 65, 7, 1, 8, 256, L2M))
add("mivq_rerank_lvq2", "empty", EMPTY, rerank_lvq2(0, 40, 0, 37, 3, 4, 10, L2M))


# ------------------------------------------------------------------------------ top-k, pairwise
def _sorted_lists(parts, nq, k, *seed):
    """Finite sorted (parts, nq, k) lists with distinct ids, some ending in padding, values that
    recur across parts."""
    g = rng(parts, nq, k, *seed)
    dd = np.full((parts, nq, k), np.inf, F32)
    ii = np.full((parts, nq, k), NO_ID, np.uint32)
    for a in range(nq):
        pool = g.permutation(max(parts * k, 1) * 2)[:parts * k].reshape(parts, k)
        for p in range(parts):
            r = k if (p + a) % 3 else int(g.integers(0, k + 1))
            d = (g.integers(0, 40, r) / 4.0).astype(F32)
            i = pool[p, :r].astype(np.int64) + (1 << 31) * int(p % 2)
            o = np.lexsort((i, d))
            dd[p, a, :r], ii[p, a, :r] = d[o], i[o].astype(np.uint32)
    return dd, ii


def topk_merge(parts, nq, k):
    def build(O):
        import _ivfpq_rule as PR

        dd, ii = _sorted_lists(parts, nq, k, 64)

        def want(c):
            if parts == 0:
                return sentinel(nq, k)
            d, i = PR.merge_rule(dd, ii, k)
            return {"dists": d, "ids": i}
        return Call([In("dists_in", dd) if parts else None, In("ids_in", ii) if parts else None, parts, nq, k,
                     Out("dists", nq * k * 4), Out("ids", nq * k * 4), None], expect=want)
    return build


add("mivq_topk_merge", "parts3-nq3-k10", RAGGED, topk_merge(3, 3, 10))
add("mivq_topk_merge", "parts7-nq17-k65", EDGE, topk_merge(7, 17, 65))
add("mivq_topk_merge", "parts2-nq1-k256", EDGE, topk_merge(2, 1, 256))
add("mivq_topk_merge", "parts1-nq3-k1", EDGE, topk_merge(1, 3, 1))
add("mivq_topk_merge", "parts0-writes-the-sentinel", EDGE, topk_merge(0, 3, 10))
add("mivq_topk_merge", "empty", EMPTY, topk_merge(3, 0, 10))


def pairwise(n, m, d, metric, skew=0):
    def build(O):
        X, Y = rows(n, d, 65), rows(m, d, 66)
        return Call([In("x", X), n, In("y", Y, skew=skew), m, d, metric, Out("out", n * m * 4), None],
                    expect=lambda c: {"out": c.O.pairwise(X, Y, metric)})
    return build


add("mivq_pairwise_distances", "n130-m65-d37-l2", RAGGED, pairwise(130, 65, 37, L2M))
add("mivq_pairwise_distances", "y-skew4-n65-m17-d64", RAGGED, pairwise(65, 17, 64, L2M, skew=4))
add("mivq_pairwise_distances", "n1025-m130-d64-ip", RAGGED, pairwise(1025, 130, 64, IPM))
add("mivq_pairwise_distances", "n1-m1-d7", EDGE, pairwise(1, 1, 7, L2M))
add("mivq_pairwise_distances", "empty", EMPTY, pairwise(0, 0, 37, L2M))


def topk_rows(n, m, k):
    def build(O):
        D = (rng(n, m, k).integers(0, 64, (n, m)) / 4.0).astype(F32)  # many ties

        def want(c):
            dd, ii = c.O.topk_rows(D, k)
            return {"out_d": dd, "out_i": ii}
        return Call([In("dist", D), n, m, k, Out("out_d", n * k * 4), Out("out_i", n * k * 4), None], expect=want)
    return build


add("mivq_topk_rows", "n130-m65-k10", RAGGED, topk_rows(130, 65, 10))
add("mivq_topk_rows", "n17-m1025-k65", EDGE, topk_rows(17, 1025, 65))
add("mivq_topk_rows", "n3-m130-k256-above-m", EDGE, topk_rows(3, 130, 256))
add("mivq_topk_rows", "n1025-m7-k1", EDGE, topk_rows(1025, 7, 1))
add("mivq_topk_rows", "empty", EMPTY, topk_rows(0, 65, 10))


# ------------------------------------------------------------------------------ IVF building blocks
def bucket_sort(n, K):
    def build(O):
        assign = rng(n, K).integers(0, K, n).astype(np.uint32)

        def want(c):
            off, order = c.O.bucket_sort(assign, K)
            return {"offsets": off, "order": order}
        return Call([In("assign", assign), n, K, Out("offsets", (K + 1) * 8), Out("order", n * 4),
                     Ws("mivq_bucket_sort_workspace_bytes", n, K), None], expect=want,
                    empty_expect={"offsets": np.zeros(K + 1, np.int64)})
    return build


add("mivq_bucket_sort", "n130-K7", RAGGED, bucket_sort(130, 7))
add("mivq_bucket_sort", "n1025-K65-one-row-past-the-block", RAGGED, bucket_sort(1025, 65))
add("mivq_bucket_sort", "n3000-K300-three-blocks", EDGE, bucket_sort(3000, 300))
add("mivq_bucket_sort", "n1-K1", EDGE, bucket_sort(1, 1))
add("mivq_bucket_sort", "empty", EMPTY, bucket_sort(0, 7))


def centroid_update(n, d, K):
    def build(O):
        X = rows(n, d, 67)
        assign = rng(n, K, 1).integers(0, max(K - 1, 1), n).astype(np.uint32)  # the last bucket stays empty
        off, order = O.bucket_sort(assign, K)
        C0 = rows(K, d, 68)
        cnt0 = rng(K, 2).integers(0, 9, K).astype(np.int32)

        def want(c):
            C, counts = c.O.centroid_update(X, assign, C0)
            return {"centroids": C, "counts": counts}
        return Call([In("x", X), n, d, K, In("offsets", off), In("order", order), InOut("centroids", C0),
                     InOut("counts", cnt0), None], expect=want, empty_expect={"counts": np.zeros(K, np.int32)})
    return build


add("mivq_centroid_update", "n130-d37-K7", RAGGED, centroid_update(130, 37, 7))
add("mivq_centroid_update", "n1025-d64-K65", RAGGED, centroid_update(1025, 64, 65))
add("mivq_centroid_update", "n1-d7-K2", EDGE, centroid_update(1, 7, 2))
add("mivq_centroid_update", "empty", EMPTY, centroid_update(0, 37, 7))


def ivf_residuals(n, d, K):
    def build(O):
        X, C = rows(n, d, 69), rows(K, d, 70)
        assign = rng(n, K, 3).integers(0, K, n).astype(np.uint32)
        return Call([In("x", X), n, d, In("coarse", C), In("assign", assign), Out("r", n * d * 4), None],
                    expect=lambda c: {"r": X - C[assign.astype(np.int64)]})
    return build


add("mivq_ivf_residuals", "n130-d37-K7", RAGGED, ivf_residuals(130, 37, 7))
add("mivq_ivf_residuals", "n1025-d64-K65", RAGGED, ivf_residuals(1025, 64, 65))
add("mivq_ivf_residuals", "n1-d7-K1", EDGE, ivf_residuals(1, 7, 1))
add("mivq_ivf_residuals", "empty", EMPTY, ivf_residuals(0, 37, 7))


def gather_rows(n, nsrc, row_bytes):
    def build(O):
        src = rng(n, nsrc, row_bytes).integers(0, 256, (nsrc, row_bytes)).astype(np.uint8)
        order = rng(n, nsrc, 4).integers(0, max(nsrc, 1), n).astype(np.uint32)
        return Call([In("src", src), row_bytes, In("order", order), n, Out("dst", n * row_bytes), None],
                    expect=lambda c: {"dst": src[order.astype(np.int64)]})
    return build


add("mivq_gather_rows", "row-bytes-4-n130", EDGE, gather_rows(130, 65, 4))
add("mivq_gather_rows", "row-bytes-148-n1025", RAGGED, gather_rows(1025, 130, 148))
add("mivq_gather_rows", "row-bytes-12288-n17", EDGE, gather_rows(17, 5, 12288))   # the longest row of the tables
add("mivq_gather_rows", "empty", EMPTY, gather_rows(0, 65, 4))


def ivfpq_terms(n, d, M, nbits, K):
    def build(O):
        C = _codebook(M, nbits, d // M, 71)
        coarse = rows(K, d, 72)
        g = rng(n, M, nbits, K)
        codes = g.integers(0, 1 << nbits, (n, M)).astype(np.uint8)
        assign = g.integers(0, K, n).astype(np.uint32)
        return Call([In("codes", codes), n, d, M, nbits, In("pq_centroids", C), In("cn", O.pq_norms(C)),
                     In("coarse", coarse), In("assign", assign), Out("tau", n * 4), None],
                    expect=lambda c: {"tau": c.O.ivfpq_terms(codes, C, coarse, assign)})
    return build


add("mivq_ivfpq_terms", "n130-d32-M2-b8", RAGGED, ivfpq_terms(130, 32, 2, 8, 7))
add("mivq_ivfpq_terms", "n1025-d21-M3-b4", EDGE, ivfpq_terms(1025, 21, 3, 4, 65))
add("mivq_ivfpq_terms", "n1-d35-M5-b3", EDGE, ivfpq_terms(1, 35, 5, 3, 1))
add("mivq_ivfpq_terms", "empty", EMPTY, ivfpq_terms(0, 32, 2, 8, 7))


# ------------------------------------------------------------------------------ IVF searches
def _lists(n, d, nlist, *seed, big_ids=False):
    """(X, coarse, assign, offsets, order, list_ids): list 1 empty where nlist > 2, ids in bucket
    order, the last few above 2^31 when big_ids."""
    g = rng(n, d, nlist, *seed)
    X = rows(n, d, *seed)
    coarse = rows(nlist, d, *seed, 1)
    assign = g.integers(0, nlist, n).astype(np.int64)
    if nlist > 2:
        assign[assign == 1] = 0
    off, order = _bucket(assign, nlist)
    ids = order.astype(np.int64)
    if big_ids and n > 4:
        ids[-3:] += 1 << 31
    return X, coarse, assign, off, order, ids.astype(np.uint32)


def _bucket(assign, K):
    order = np.argsort(assign, kind="stable").astype(np.uint32)
    off = np.zeros(K + 1, np.int64)
    off[1:] = np.cumsum(np.bincount(assign, minlength=K))
    return off, order


def _probes(nq, nlist, nprobe, *seed):
    """Distinct lists per query in its own order, one skipped slot in query 0."""
    g = rng(nq, nlist, nprobe, *seed)
    P = np.stack([g.permutation(nlist)[:nprobe] for _ in range(max(nq, 1))])[:nq].astype(np.uint32)
    if nq and nprobe > 1:
        P[0, -1] = NO_ID
    return P.reshape(nq, nprobe)


def ivfpq_search(nq, n, d, M, nbits, nlist, nprobe, k, metric):
    def build(O):
        X, coarse, assign, off, order, ids = _lists(n, d, nlist, 73, big_ids=True)
        C = _codebook(M, nbits, d // M, 74) * F32(0.5)
        Q = rows(nq, d, 75)
        g = rng(nq, n, 76)
        codes = g.integers(0, 1 << nbits, (n, M)).astype(np.uint8)[order]
        tau = g.standard_normal(n).astype(F32)
        P = _probes(nq, nlist, nprobe, 77)
        pd = g.standard_normal((nq, nprobe)).astype(F32)
        lut = O.adc_lut(Q, C, IPM) if nq else np.zeros((0, M, 1 << nbits), F32)

        def want(c):
            dd, ii = c.O.ivfpq_search(lut, pd, P, off, codes, ids, tau, metric, k)
            return {"dists": dd, "ids": ii}
        return Call([In("lut", lut), nq, M, nbits, In("probe_d", pd), In("probe_l", P), nprobe, nlist, In("offsets", off),
                     In("list_codes", codes), In("list_ids", ids), In("tau", tau), metric, k,
                     Ws("mivq_ivfpq_search_workspace_bytes", nq, nprobe, k), *topk(nq, k), None], expect=want)
    return build


add("mivq_ivfpq_search", "nq3-n130-M2-b8-nprobe2-k10-l2", RAGGED, ivfpq_search(3, 130, 32, 2, 8, 4, 2, 10, L2M))
add("mivq_ivfpq_search", "nq17-n1025-M3-b4-nprobe7-k65-ip", EDGE, ivfpq_search(17, 1025, 21, 3, 4, 7, 7, 65, IPM))
add("mivq_ivfpq_search", "nq1-n65-M5-b3-nprobe1-k256-above-n", EDGE, ivfpq_search(1, 65, 35, 5, 3, 4, 1, 256, L2M))
add("mivq_ivfpq_search", "empty", EMPTY, ivfpq_search(0, 0, 32, 2, 8, 4, 2, 10, L2M))


def _rabitq_rows(O, X, coarse, assign, metric):
    d = X.shape[1]
    codes = np.zeros((X.shape[0], (d + 7) // 8 + 8), np.uint8)
    for l in range(coarse.shape[0]):
        sel = np.flatnonzero(assign == l)
        if sel.size:
            codes[sel] = O.rabitq_encode(X[sel], coarse[l], metric)
    return codes


def ivf_rabitq_encode(n, d, nlist, metric, skew=0):
    def build(O):
        from _bounds_codec import rabitq_code_check

        X, coarse, assign, *_ = _lists(n, d, nlist, 78)
        return Call([In("x", X, skew=skew), n, d, In("coarse", coarse), nlist, In("assign", assign.astype(np.uint32)), metric,
                     Out("codes", n * ((d + 7) // 8 + 8)), None],
                    expect=lambda c: {"codes": _rabitq_rows(c.O, X, coarse, assign, metric)},
                    check={"codes": rabitq_code_check(d)})
    return build


add("mivq_ivf_rabitq_encode", "vec-n130-d64-l2", RAGGED, ivf_rabitq_encode(130, 64, 4, L2M))
add("mivq_ivf_rabitq_encode", "scalar-x-skew4-n65-d64", RAGGED, ivf_rabitq_encode(65, 64, 4, L2M, skew=4))
add("mivq_ivf_rabitq_encode", "n65-d37-ip-code-size-13", EDGE, ivf_rabitq_encode(65, 37, 7, IPM))
add("mivq_ivf_rabitq_encode", "wide-n1025-d512", RAGGED, ivf_rabitq_encode(1025, 512, 7, L2M))
add("mivq_ivf_rabitq_encode", "empty", EMPTY, ivf_rabitq_encode(0, 37, 4, L2M))


def ivf_rabitq_search(nq, n, d, nlist, nprobe, qb, k, metric):
    def build(O):
        X, coarse, assign, off, order, ids = _lists(n, d, nlist, 79, big_ids=True)
        codes = _rabitq_rows(O, X, coarse, assign, metric)[order]
        Q = rows(nq, d, 80)
        P = _probes(nq, nlist, nprobe, 81)

        def want(c):
            dd, ii = IR.expected(c.O, codes, ids, off, coarse, Q, P, qb, metric, k)
            return {"dists": dd, "ids": ii}
        return Call([In("q", Q), nq, d, In("coarse", coarse), nlist, In("probe_l", P), nprobe, In("offsets", off),
                     In("list_codes", codes), In("list_ids", ids), qb, metric, k,
                     Ws("mivq_ivf_rabitq_search_workspace_bytes", nq, n, nlist, nprobe, d, k), *topk(nq, k), None],
                    expect=want)
    return build


add("mivq_ivf_rabitq_search", "mfma-qb4-nq3-n130-d64-nprobe2-k10", RAGGED, ivf_rabitq_search(3, 130, 64, 4, 2, 4, 10, L2M))
add("mivq_ivf_rabitq_search", "generic-qb4-nq17-n1025-d37-nprobe7-k65", EDGE,
    ivf_rabitq_search(17, 1025, 37, 7, 7, 4, 65, IPM))
add("mivq_ivf_rabitq_search", "generic-qb0-nq1-n65-d64-nprobe1-k256-above-n", EDGE,
    ivf_rabitq_search(1, 65, 64, 4, 1, 0, 256, L2M))
add("mivq_ivf_rabitq_search", "two-chunks-nq1040-n512-d32-nprobe256-k256", EDGE,
    ivf_rabitq_search(1040, 512, 32, 256, 256, 4, 256, L2M))
add("mivq_ivf_rabitq_search", "empty", EMPTY, ivf_rabitq_search(0, 0, 37, 4, 2, 4, 10, L2M))


def ivf_sq_fit(n, d, nlist):
    def build(O):
        X, coarse, assign, off, order, _ = _lists(n, d, nlist, 82)

        def want(c):
            lo, den = IQ.fit(X, coarse, assign, "sq")
            return {"lo": lo, "den": den}
        return Call([In("x", X), n, d, In("coarse", coarse), nlist, In("offsets", off), In("order", order),
                     Out("lo", nlist * d * 4), Out("den", nlist * d * 4), None], expect=want,
                    empty_expect={"lo": np.zeros((nlist, d), F32), "den": np.full((nlist, d), F32(1e-8), F32)})
    return build


add("mivq_ivf_sq_fit", "n130-d37-nlist4-one-empty", RAGGED, ivf_sq_fit(130, 37, 4))
add("mivq_ivf_sq_fit", "n1025-d64-nlist65", RAGGED, ivf_sq_fit(1025, 64, 65))
add("mivq_ivf_sq_fit", "n1-d7-nlist1", EDGE, ivf_sq_fit(1, 7, 1))
add("mivq_ivf_sq_fit", "empty", EMPTY, ivf_sq_fit(0, 37, 4))


def _code_bytes(kind, bits, d):
    w, dt = IQ.code_shape(kind, bits, d)
    return w * np.dtype(dt).itemsize


def ivf_code_encode(kind, n, d, nlist, bits, skew=0):
    def build(O):
        X, coarse, assign, *_ = _lists(n, d, nlist, 83)
        params = IQ.fit(X, coarse, assign, kind)
        names = ("lo", "den") if kind == "sq" else ("mu",)
        return Call([In("x", X, skew=skew), n, d, In("coarse", coarse), nlist, In("assign", assign.astype(np.uint32)),
                     *[In(nm, p) for nm, p in zip(names, params)], bits, Out("codes", n * _code_bytes(kind, bits, d)), None],
                    expect=lambda c: {"codes": IQ.encode(X, coarse, assign, params, kind, bits)})
    return build


def ivf_code_decode(kind, n, d, nlist, bits, skew=0):
    def build(O):
        X, coarse, assign, *_ = _lists(n, d, nlist, 84)
        params = IQ.fit(X, coarse, assign, kind)
        codes = IQ.encode(X, coarse, assign, params, kind, bits)
        names = ("lo", "den") if kind == "sq" else ("mu",)
        return Call([In("codes", codes), n, d, In("coarse", coarse), nlist, In("assign", assign.astype(np.uint32)),
                     *[In(nm, p) for nm, p in zip(names, params)], bits, Out("out", n * d * 4, skew=skew), None],
                    expect=lambda c: {"out": IQ.decode(c.O, codes, coarse, assign, params, kind, bits)})
    return build


for _kind, _b, _bo in (("sq", 8, 4), ("lvq", 8, 3)):
    for _fn, _mk, _op in (("encode", ivf_code_encode, "x"), ("decode", ivf_code_decode, "out")):
        _e = f"mivq_ivf_{_kind}_{_fn}"
        add(_e, f"b{_b}-n130-d64-nlist4", RAGGED, _mk(_kind, 130, 64, 4, _b))
        add(_e, f"{_op}-skew4-b{_b}-n65-d64", RAGGED, _mk(_kind, 65, 64, 4, _b, skew=4))
        add(_e, f"b{_bo}-odd-d37-n65-nlist7", EDGE, _mk(_kind, 65, 37, 7, _bo))
        add(_e, f"b{_b}-n1025-d100-nlist65", RAGGED, _mk(_kind, 1025, 100, 65, _b))
        add(_e, "empty", EMPTY, _mk(_kind, 0, 37, 4, _bo))
add("mivq_ivf_sq_encode", "b16-n130-d37", EDGE, ivf_code_encode("sq", 130, 37, 4, 16))
add("mivq_ivf_sq_decode", "b16-n130-d37", EDGE, ivf_code_decode("sq", 130, 37, 4, 16))


def ivf_code_search(kind, nq, n, d, nlist, nprobe, bits, k, metric):
    def build(O):
        X, coarse, assign, off, order, ids = _lists(n, d, nlist, 85, big_ids=True)
        params = IQ.fit(X, coarse, assign, kind)
        codes = np.ascontiguousarray(IQ.encode(X, coarse, assign, params, kind, bits)[order])
        Q = rows(nq, d, 86)
        P = _probes(nq, nlist, nprobe, 87)
        names = ("lo", "den") if kind == "sq" else ("mu",)

        def want(c):
            dd, ii = IQ.expected(c.O, codes, ids, off, coarse, params, kind, bits, Q, P, metric, k)
            return {"dists": dd, "ids": ii}
        return Call([In("q", Q), nq, d, In("coarse", coarse), nlist, In("probe_l", P), nprobe, In("offsets", off),
                     In("list_codes", codes), In("list_ids", ids), *[In(nm, p) for nm, p in zip(names, params)], bits,
                     metric, k, Ws(f"mivq_ivf_{kind}_search_workspace_bytes", nq, n, nlist, nprobe, d, bits, k),
                     *topk(nq, k), None], expect=want)
    return build


for _kind, _b, _bo in (("sq", 8, 4), ("lvq", 8, 3)):
    _e = f"mivq_ivf_{_kind}_search"
    add(_e, f"b{_b}-nq3-n130-d64-nprobe2-k10", RAGGED, ivf_code_search(_kind, 3, 130, 64, 4, 2, _b, 10, L2M))
    add(_e, f"b{_bo}-odd-d37-nq17-n1025-nprobe7-k65", EDGE, ivf_code_search(_kind, 17, 1025, 37, 7, 7, _bo, 65, IPM))
    add(_e, f"b{_b}-nq1-n65-d7-nprobe1-k256-above-n", EDGE, ivf_code_search(_kind, 1, 65, 7, 4, 1, _b, 256, L2M))
    add(_e, f"two-chunks-b{_b}-nq1040-n512-d8-nprobe256-k256", EDGE,
        ivf_code_search(_kind, 1040, 512, 8, 256, 256, _b, 256, L2M))
    add(_e, "empty", EMPTY, ivf_code_search(_kind, 0, 0, 37, 4, 2, _bo, 10, L2M))
add("mivq_ivf_sq_search", "b16-nq3-n130-d37-nprobe2-k10", EDGE, ivf_code_search("sq", 3, 130, 37, 4, 2, 16, 10, L2M))


def _listpq(n, d, M, B, nlist, *seed):
    X, coarse, assign, off, order, ids = _lists(n, d, nlist, *seed, big_ids=True)
    cb = (rng(nlist, M, B, *seed).standard_normal((nlist, M, 1 << B, d // M)) * 0.5).astype(F32)
    codes = rng(n, M, B, *seed).integers(0, 1 << B, (n, M)).astype(np.uint8)
    return X, coarse, assign, off, order, ids, cb, codes


def ivf_listpq_decode(n, d, M, B, nlist, skew=0):
    def build(O):
        _, coarse, assign, _, _, _, cb, codes = _listpq(n, d, M, B, nlist, 88)
        return Call([In("codes", codes), n, d, M, B, In("codebooks", cb), In("coarse", coarse), nlist,
                     In("assign", assign.astype(np.uint32)), Out("out", n * d * 4, skew=skew), None],
                    expect=lambda c: {"out": LP.decode(c.O, codes, coarse, assign, cb)})
    return build


add("mivq_ivf_listpq_decode", "n130-d32-M2-b8-nlist4", RAGGED, ivf_listpq_decode(130, 32, 2, 8, 4))
add("mivq_ivf_listpq_decode", "out-skew4-n65-d32-M2-b8", RAGGED, ivf_listpq_decode(65, 32, 2, 8, 4, skew=4))
add("mivq_ivf_listpq_decode", "n1025-d21-M3-b4-nlist7", EDGE, ivf_listpq_decode(1025, 21, 3, 4, 7))
add("mivq_ivf_listpq_decode", "n65-d35-M35-b3-dsub1", EDGE, ivf_listpq_decode(65, 35, 35, 3, 4))
add("mivq_ivf_listpq_decode", "empty", EMPTY, ivf_listpq_decode(0, 32, 2, 8, 4))


def ivf_listpq_search(nq, n, d, M, B, nlist, nprobe, k, metric):
    def build(O):
        _, coarse, assign, off, order, ids, cb, codes = _listpq(n, d, M, B, nlist, 89)
        codes = np.ascontiguousarray(codes[order])
        Q = rows(nq, d, 90)
        P = _probes(nq, nlist, nprobe, 91)

        def want(c):
            dd, ii = LP.expected(c.O, codes, ids, off, coarse, cb, Q, P, metric, k)
            return {"dists": dd, "ids": ii}
        return Call([In("q", Q), nq, d, M, B, In("codebooks", cb), In("coarse", coarse), nlist, In("probe_l", P), nprobe,
                     In("offsets", off), In("list_codes", codes), In("list_ids", ids), metric, k,
                     Ws("mivq_ivf_listpq_search_workspace_bytes", nq, n, nlist, nprobe, d, M, B, k), *topk(nq, k), None],
                    expect=want)
    return build


add("mivq_ivf_listpq_search", "nq3-n130-d32-M2-b8-nprobe2-k10", RAGGED, ivf_listpq_search(3, 130, 32, 2, 8, 4, 2, 10, L2M))
add("mivq_ivf_listpq_search", "nq17-n1025-d21-M3-b4-nprobe7-k65-ip", EDGE,
    ivf_listpq_search(17, 1025, 21, 3, 4, 7, 7, 65, IPM))
add("mivq_ivf_listpq_search", "nq1-n65-d35-M35-b3-dsub1-nprobe1-k256-above-n", EDGE,
    ivf_listpq_search(1, 65, 35, 35, 3, 4, 1, 256, L2M))
add("mivq_ivf_listpq_search", "empty", EMPTY, ivf_listpq_search(0, 0, 32, 2, 8, 4, 2, 10, L2M))
