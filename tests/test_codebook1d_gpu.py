"""GPU: mivq_codebook1d_fit bit for bit against the reference's builders
(tests/golden/codebook1d_golden.npz) and the rule (tests/_codebook1d_rule.py), and
RankAwareQuantizer(codebook="lloyd" | "exact", codebook_engine="device") from the sample to the
index."""

import numpy as np
import pytest
import torch

import _codebook1d_rule as CR
import _rankaware_rule as RR

pytestmark = pytest.mark.gpu

LEFT_OUT_CAP = 0.02   # share of a case's dimensions whose own f32 sample column may differ from numpy's


@pytest.fixture(scope="module")
def z(golden_dir):
    with np.load(golden_dir / CR.GOLDEN, allow_pickle=False) as f:
        return {k: f[k] for k in f.files}


@pytest.fixture(scope="module")
def g(golden_dir):
    return RR.load_golden(golden_dir)


@pytest.fixture(scope="module")
def rule_sse():
    """The rule's fp64 sse of every column case and method, computed once (the fixture holds the
    reference's f32 cost, which the CPU tests tie to these)."""
    return {(name, m): CR.fit(CR.column(name), CR.COLUMN_CASES[name][1], m)[1]
            for name in CR.COLUMN_CASES for m in CR.METHODS}


def _same_bits(a, b) -> bool:
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _preload_normal_tables(g):
    """The N(0,1) Lloyd tables of seed 0 (b = 0..8) from rankaware_golden.npz into the quantizer
    module's per-process cache: fit() then spends its time on the device, not on the CPU tables."""
    import haag_vq.methods.rank_aware_quantization as ram

    for b in range(9):
        key = (b, 2 ** b, 200_000, 100, 1e-7)
        ram._LLOYD_CACHE.setdefault(key, (np.array(g["levels"][2 ** b - 1:2 ** (b + 1) - 1]), float(g["Dg"][b])))


# ------------------------------------------------------------------ the library, column cases
def _groups():
    """The column cases as calls: one per sample size, its columns as the call's dimensions; the
    n = 1000 call also carries a width-0 dimension, so that one call holds every width 0..8."""
    by_n = {}
    for name, (n, w, _, _) in CR.COLUMN_CASES.items():
        by_n.setdefault(n, []).append(name)
    return by_n


@pytest.mark.parametrize("method", CR.METHODS)
def test_columns_against_the_fixture(dev, z, rule_sse, method):
    from haag_vq import _native

    m = _native.CB1D_METHODS[method]
    lib = _native.load_library()
    for n, names in _groups().items():
        widths = [CR.COLUMN_CASES[nm][1] for nm in names]
        cols = [CR.column(nm) for nm in names]
        if n == 1000:
            names, widths, cols = names + [None], widths + [0], cols + [CR.column("g1000_w3")]
            assert set(widths) == set(range(9))
        cd = torch.from_numpy(np.stack(cols)).to(dev)
        one = lib.mivq_codebook1d_workspace_bytes(n, max(widths), m, 1)
        runs = [_native.codebook1d_fit(cd, widths, method, workspace_bytes=one),       # one dimension at a time
                _native.codebook1d_fit(cd, widths, method, workspace_bytes=one * len(widths)),
                _native.codebook1d_fit(cd, widths, method)]
        lv0, off0, sse0 = (runs[0][0].cpu().numpy(), runs[0][1], runs[0][2].cpu().numpy())
        for lv, off, sse in runs[1:]:
            assert np.array_equal(off, off0) and _same_bits(lv.cpu().numpy(), lv0) and _same_bits(sse.cpu().numpy(), sse0)
        for j, nm in enumerate(names):
            got = lv0[off0[j]:off0[j + 1]]
            if nm is None:
                assert got.tolist() == [0.0] and sse0[j] == 0.0    # width 0: the caller's level, untouched
                continue
            assert _same_bits(got, z[f"col_{nm}_{method}"]), (nm, method)
            assert sse0[j] == rule_sse[nm, method], (nm, method, sse0[j], rule_sse[nm, method])
            assert np.float32(sse0[j] / n) == z[f"col_{nm}_{method}_cost"]


def test_width_order_does_not_matter(dev, z):
    """The library starts the widest dimensions first whatever their order in the call."""
    from haag_vq import _native

    names = [f"g1000_w{w}" for w in (2, 8, 1, 5, 8, 3)]
    widths = [CR.COLUMN_CASES[nm][1] for nm in names]
    cd = torch.from_numpy(np.stack([CR.column(nm) for nm in names])).to(dev)
    for method in CR.METHODS:
        one = _native.load_library().mivq_codebook1d_workspace_bytes(1000, 8, _native.CB1D_METHODS[method], 1)
        lv, off, _ = _native.codebook1d_fit(cd, widths, method, workspace_bytes=2 * one)
        lv = lv.cpu().numpy()
        for j, nm in enumerate(names):
            assert _same_bits(lv[off[j]:off[j + 1]], z[f"col_{nm}_{method}"]), (nm, method)


@pytest.mark.parametrize("method", CR.METHODS)
def test_more_dimensions_than_one_table_launch(dev, method):
    """600 dimensions in flight at once: the batch's table reaches the slots 256 entries to a launch,
    the fit itself is one launch over all of them; also with room for 257 slots of the widest."""
    from haag_vq import _native

    base = [np.sort(np.random.default_rng([7, j]).standard_normal(200).astype(np.float32)) for j in range(5)]
    widths = [1 + (j * 7) % 4 for j in range(600)]
    cols = np.stack([base[j % 5] for j in range(600)])
    want = {(c, w): CR.fit(base[c], w, method) for c in range(5) for w in range(1, 5)}
    cd = torch.from_numpy(cols).to(dev)
    one = _native.load_library().mivq_codebook1d_workspace_bytes(200, 4, _native.CB1D_METHODS[method], 1)
    assert _native.codebook1d_workspace(200, widths, method, dev) == (600 * one, 600)
    for ws in (None, 257 * one):
        lv, off, sse = _native.codebook1d_fit(cd, widths, method, workspace_bytes=ws)
        lv, sse = lv.cpu().numpy(), sse.cpu().numpy()
        for j, w in enumerate(widths):
            levels, s = want[j % 5, w]
            assert _same_bits(lv[off[j]:off[j + 1]], levels) and sse[j] == s, (method, j, w, ws)


# ------------------------------------------------------------------ _fit_codebooks on the fixture states
@pytest.mark.parametrize("method", CR.METHODS)
@pytest.mark.parametrize("name", list(RR.CASES))
def test_fit_codebooks_on_fixture_states(dev, z, g, name, method):
    X = RR.inputs(name)
    q = RR.fixture_quantizer(g, name, "dense")
    q.codebook, q.codebook_engine = method, "device"
    cb = q._fit_codebooks(X)
    assert len(cb) == q.D and all(t.dtype == np.float64 and t.shape == (2 ** int(b),) for t, b in zip(cb, q.bits))
    want = RR.split_cb(z[f"{name}_cb_{method}"], q.bits)
    cols = q.sample_columns(X).cpu().numpy()
    Y = np.sort(((np.asarray(X, dtype=np.float64) - q.mu) @ q.V).astype(np.float32), axis=0).T
    assert cols.shape == Y.shape == (q.D, X.shape[0])
    left_out = [d for d in range(q.D) if not _same_bits(cols[d], Y[d])]
    print(f"{name} {method}: {len(left_out)} of {q.D} dimensions left out")
    assert len(left_out) <= LEFT_OUT_CAP * q.D
    for d in range(q.D):
        if d not in left_out:
            assert _same_bits(cb[d], want[d]), (name, method, d, int(q.bits[d]))


# ------------------------------------------------------------------ a full fit
@pytest.fixture(scope="module")
def fitted(dev, g):
    """RankAwareQuantizer.fit of w08's rows with both fitted codebooks, the fit's own sorted
    columns and the library's sse on them."""
    from haag_vq import _native
    from haag_vq.methods.rank_aware_quantization import RankAwareQuantizer

    _preload_normal_tables(g)
    c, X = RR.CASES["w08"], RR.inputs("w08")
    out = {}
    for method in CR.METHODS:
        q = RankAwareQuantizer(c["avg_bits"], alpha=c["alpha"], max_bits=c["max_bits"], codebook=method,
                               codebook_engine="device")
        q.fit(X)
        cols = q.sample_columns(X)
        _, _, sse = _native.codebook1d_fit(cols, q.bits, method)
        out[method] = (q, cols.cpu().numpy(), sse.cpu().numpy())
    return out


@pytest.mark.parametrize("method", CR.METHODS)
def test_full_fit_equals_the_rule_on_its_own_columns(fitted, method):
    q, cols, sse = fitted[method]
    assert set(q.bits.tolist()) == set(range(9)) and q.codebook_engine == "device"
    assert np.all(cols[:, 1:] >= cols[:, :-1])
    wide = [d for d in range(q.D) if q.bits[d] >= 6][:16]
    for d in range(q.D):
        b = int(q.bits[d])
        if b == 0:
            assert q.cb[d].tolist() == [0.0]
        elif b < 6 or d in wide:
            levels, want_sse = CR.fit(cols[d], b, method)
            assert _same_bits(q.cb[d], levels.astype(np.float64)), (method, d, b)
            assert sse[d] == want_sse, (method, d, b)
    assert q.code_size == (int(q.bits.sum()) + 7) // 8


def test_exact_is_optimal_on_the_fit(fitted):
    qe, cols, sse_e = fitted["exact"]
    ql, cols_l, sse_l = fitted["lloyd"]
    assert np.array_equal(qe.bits, ql.bits) and _same_bits(cols, cols_l)
    scale = np.sqrt(qe.var)
    for d in np.flatnonzero(qe.bits):
        b = int(qe.bits[d])
        assert sse_e[d] <= sse_l[d] * (1 + 1e-12), (d, b, sse_e[d], sse_l[d])
        gauss = CR.table_sse(cols[d], qe._levels[b] * scale[d])
        assert sse_e[d] <= gauss * (1 + 1e-6), (d, b, sse_e[d], gauss)


# ------------------------------------------------------------------ through the codec and the index
@pytest.mark.parametrize("method", CR.METHODS)
@pytest.mark.parametrize("packing", RR.PACKINGS)
def test_codec_and_index_with_fitted_tables(dev, g, packing, method):
    from haag_vq.methods.rank_aware_quantization import RankAwareQuantizer
    from haag_vq.methods.search.flat_quantized_index import FlatQuantizedIndex, RankAwareFlatIndex

    _preload_normal_tables(g)
    c, X = RR.CASES["w08"], RR.inputs("w08")
    assert X.shape == (512, 64)
    Q = RR.gaussian_rows(20, 64, c["decay"], 9)
    idx = RankAwareFlatIndex(RankAwareQuantizer(c["avg_bits"], alpha=c["alpha"], max_bits=c["max_bits"], packing=packing,
                                                codebook=method, codebook_engine="device"))
    idx.fit(X)
    q = idx.quantizer
    st = RR.make_state(q.mu, q.V, q.bits, q.cb, q.field_positions(), q.code_size, packing)
    codes = idx._codes.cpu().numpy()
    Y = RR.project(X, st)
    assert not RR.tie_problems(RR.unpack(codes, st), RR.indices(Y, st), Y, X, st)
    rec = q.decompress(idx._codes).cpu().numpy()
    slack = RR.decode_slack(rec, RR.lookup(RR.unpack(codes, st), st), q.D)
    assert np.all(np.abs(rec.astype(np.float64) - RR.decompress(codes, st)) <= slack)
    gauss = RankAwareQuantizer(c["avg_bits"], alpha=c["alpha"], max_bits=c["max_bits"], packing=packing)
    gauss.fit(X)
    mse, mse_g = float(np.mean((rec - X) ** 2)), float(np.mean((gauss.decompress(gauss.compress(X)) - X) ** 2))
    print(f"{method} {packing}: mse {mse:.4e}, gaussian tables {mse_g:.4e}")
    if method == "exact":   # per dimension the optimal table for these very rows; V is orthogonal
        assert mse < mse_g

    plain = FlatQuantizedIndex(q)
    plain._codes, plain._metric, plain._N, plain._D = idx._codes, idx._metric, idx._N, idx._D
    assert np.array_equal(idx.search(Q, 10), plain.search(Q, 10))
