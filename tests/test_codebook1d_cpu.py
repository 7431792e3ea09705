"""CPU: the data-fitted codebook rule (tests/_codebook1d_rule.py) against the reference's builders
(tests/golden/codebook1d_golden.npz), the host-side generator, the codebook_engine keyword, the
library's size query and error paths, and save / load of a quantizer with fitted tables."""

import ctypes

import numpy as np
import pytest

import _codebook1d_rule as CR
import _rankaware_rule as RR


@pytest.fixture(scope="module")
def z(golden_dir):
    with np.load(golden_dir / CR.GOLDEN, allow_pickle=False) as f:
        return {k: f[k] for k in f.files}


def _same_bits(a, b) -> bool:
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------ the rule
def test_fixture_lists_the_cases(z):
    assert list(z["column_cases"]) == list(CR.COLUMN_CASES) and list(z["fit_cases"]) == list(RR.CASES)
    for name, (n, w, kind, draw) in CR.COLUMN_CASES.items():   # the fixture's own record of each column's seed
        assert z[f"col_{name}_seed"].tolist() == [n, w, draw] and str(z[f"col_{name}_kind"]) == kind


@pytest.mark.parametrize("method", CR.METHODS)
@pytest.mark.parametrize("name", list(CR.COLUMN_CASES))
def test_rule_reproduces_the_reference_columns(z, name, method):
    n, w, _, _ = CR.COLUMN_CASES[name]
    s = CR.column(name)
    assert CR.sha(s) == str(z[f"col_{name}_sha"])
    levels, sse = CR.fit(s, w, method)
    assert _same_bits(levels, z[f"col_{name}_{method}"])
    assert np.float32(sse / n) == z[f"col_{name}_{method}_cost"]
    assert levels.shape == (1 << w,) and np.all(levels[1:] >= levels[:-1])


@pytest.mark.parametrize("name", list(CR.COLUMN_CASES))
def test_rule_reproduces_the_reference_seeding(z, name):
    n, w, _, _ = CR.COLUMN_CASES[name]
    s = CR.column(name)
    key = f"col_{name}_lloyd_seed"
    assert (key in z) == ((1 << w) < len(CR.distinct(s)))
    if key in z:
        seeds = CR.seed_centres(s, 1 << w)
        assert _same_bits(CR._pad(np.unique(seeds.astype(np.float32)), 1 << w), z[key])


def test_lloyd_cases_cover_repair_cap_and_convergence():
    seen = set()
    for name, (n, w, _, _) in CR.COLUMN_CASES.items():
        s = CR.column(name)
        if (1 << w) >= len(CR.distinct(s)):
            continue
        info = {}
        CR.lloyd(s, w, info=info)
        seen |= {"repair"} if info["repairs"] else set()
        seen |= {"cap"} if info["passes"] == CR.MAX_PASSES and not info["converged"] else set()
        seen |= {"early"} if info["converged"] and info["passes"] < CR.MAX_PASSES else set()
    assert seen == {"repair", "cap", "early"}


def test_degenerate_tables_are_the_distinct_values_padded():
    for name in ("one", "n_eq_k", "const", "few_under"):
        n, w, _, _ = CR.COLUMN_CASES[name]
        s = CR.column(name)
        ds = CR.distinct(s)
        assert len(ds) <= 1 << w
        for method in CR.METHODS:
            levels, sse = CR.fit(s, w, method)
            assert sse == 0.0 and _same_bits(levels[:len(ds)], ds) and np.all(levels[len(ds):] == ds[-1])


def test_exact_is_no_worse_than_lloyd_on_every_column():
    for name, (n, w, _, _) in CR.COLUMN_CASES.items():
        s = CR.column(name)
        assert CR.exact(s, w)[1] <= CR.lloyd(s, w)[1] * (1 + 1e-12), name


@pytest.mark.parametrize("method", CR.METHODS)
@pytest.mark.parametrize("name", ["odd37", "cap3"])
def test_rule_reproduces_the_reference_fit(z, golden_dir, name, method):
    """Two of the fit cases on the CPU (the GPU test covers all): the fixture's state projected by
    numpy, every dimension through the rule."""
    g = RR.load_golden(golden_dir)
    st = RR.fixture_state(g, name, "dense")
    Y = ((np.asarray(RR.inputs(name), dtype=np.float64) - st.mu) @ st.V).astype(np.float32)
    got = [CR.fit(np.sort(Y[:, d]), int(b), method)[0].astype(np.float64) if b else np.array([0.0])
           for d, b in enumerate(st.bits)]
    assert _same_bits(np.concatenate(got), z[f"{name}_cb_{method}"])


# ------------------------------------------------------------------ the generator
PUBLISHED_5489 = (14514284786278117030, 4620546740167642908, 13109570281517897720)
PUBLISHED_10000TH = 9981545732273789042   # ISO C++ [rand.predef]: the 10000th output of mt19937_64


def test_mt19937_64_published_outputs():
    from haag_vq import _native

    out = _native.mt19937_64(5489, 10000)
    assert tuple(out[:3]) == PUBLISHED_5489 and out[9999] == PUBLISHED_10000TH
    g = CR.MT19937_64(5489)
    mine = [g() for _ in range(10000)]
    assert mine == out
    g0 = CR.MT19937_64(0)
    assert [g0() for _ in range(_native.CB1D_DRAWS)] == _native.mt19937_64(0, _native.CB1D_DRAWS)


def test_index_draw_rejects_and_stays_in_range():
    draws = iter([5])                  # n = 10, 2^64 mod 10 = 6: the low half 50 is accepted, high half 0
    assert CR.draw_index(lambda: next(draws), 10) == 0
    draws = iter([0, (1 << 63) + 1])   # low half 0 < 6: rejected; then 5 * 2^64 + 10: accepted, high half 5
    assert CR.draw_index(lambda: next(draws), 10) == 5
    assert CR.draw_unit(lambda: (1 << 64) - 1) == np.nextafter(1.0, 0.0)
    assert CR.draw_unit(lambda: 1 << 63) == 0.5


# ------------------------------------------------------------------ the keyword
def test_codebook_engine_keyword():
    from haag_vq.methods.rank_aware_quantization import RankAwareQuantizer

    assert RankAwareQuantizer(4.0).codebook_engine == "saq"
    for cb in ("gaussian", "lloyd", "exact"):
        assert RankAwareQuantizer(4.0, codebook=cb, codebook_engine="device").codebook_engine == "device"
    for bad in ("gpu", "", None, "SAQ"):
        with pytest.raises(ValueError, match="codebook_engine"):
            RankAwareQuantizer(4.0, codebook="lloyd", codebook_engine=bad)
    q = RankAwareQuantizer(4.0, codebook="exact")
    with pytest.raises(ValueError, match="out of scope"):
        q.fit(np.zeros((4, 4), dtype=np.float32))


# ------------------------------------------------------------------ the library without a GPU
def test_size_query_needs_no_gpu():
    from haag_vq import _native

    lib = _native.load_library()
    q = lib.mivq_codebook1d_workspace_bytes
    n = 200_000
    exact8, lloyd8 = q(n, 8, _native.CB1D_EXACT, 1), q(n, 8, _native.CB1D_LLOYD, 1)
    assert exact8 >= 4 * 8 * (n + 1) + 4 * 255 * (n + 1) and exact8 < 4 * 8 * (n + 1) + 4 * 256 * (n + 1) + 2 ** 16
    assert 4 * 8 * (n + 1) <= lloyd8 < 4 * 8 * (n + 1) + 2 ** 16
    assert q(n, 8, _native.CB1D_EXACT, 7) == 7 * exact8
    assert q(n, 1, _native.CB1D_EXACT, 1) < q(n, 4, _native.CB1D_EXACT, 1) < exact8
    assert q(n, 4, _native.CB1D_LLOYD, 1) == lloyd8   # Lloyd keeps no argmins
    for bad in ((-1, 8, 0, 1), (n, 9, 0, 1), (n, -1, 0, 1), (n, 8, 2, 1), (n, 8, 0, 0), ((1 << 26) + 1, 8, 0, 1)):
        assert q(*bad) == 0, bad


def _fit_rc(n, width, lv_off, method, ws_bytes, ndraws=320, fake=0x1000):
    """mivq_codebook1d_fit with pointers that are never followed: every call here has to return
    before its first launch."""
    from haag_vq import _native

    lib = _native.load_library()
    w = np.asarray(width, dtype=np.int32)
    off = np.asarray(lv_off, dtype=np.int32)
    p = ctypes.c_void_p(fake)
    return lib.mivq_codebook1d_fit(p, n, len(w), w.ctypes.data_as(ctypes.c_void_p), off.ctypes.data_as(ctypes.c_void_p),
                                   method, p, ndraws, p, ws_bytes, p, p, None)


def test_error_paths_need_no_gpu():
    from haag_vq import _native

    lib = _native.load_library()
    E, L = _native.CB1D_EXACT, _native.CB1D_LLOYD
    assert _fit_rc(0, [3], [0, 8], E, 0) == _native.MIVQ_OK            # n == 0: nothing to do
    assert _fit_rc(100, [], [0], E, 0) == _native.MIVQ_OK              # d == 0
    assert _fit_rc(100, [0, 0], [0, 1, 2], L, 0) == _native.MIVQ_OK    # only width-0 dimensions
    assert _fit_rc(100, [9], [0, 512], E, 1 << 30) == _native.MIVQ_ERR_INVALID
    assert b"outside 0..8" in lib.mivq_last_error()
    assert _fit_rc(100, [-1], [0, 1], E, 1 << 30) == _native.MIVQ_ERR_INVALID
    assert _fit_rc(100, [3], [0, 4], E, 1 << 30) == _native.MIVQ_ERR_INVALID      # lv_off holds 4, not 8
    assert _fit_rc(100, [3], [0, 8], 2, 1 << 30) == _native.MIVQ_ERR_INVALID      # unknown method
    assert _fit_rc(-1, [3], [0, 8], E, 1 << 30) == _native.MIVQ_ERR_INVALID
    assert _fit_rc(100, [8], [0, 256], L, 1 << 30, ndraws=255) == _native.MIVQ_ERR_INVALID
    assert _fit_rc((1 << 26) + 1, [3], [0, 8], E, 1 << 40) == _native.MIVQ_ERR_UNSUPPORTED
    for m in (E, L):
        need = lib.mivq_codebook1d_workspace_bytes(100, 5, m, 1)
        assert _fit_rc(100, [5, 2], [0, 32, 36], m, need - 1) == _native.MIVQ_ERR_WORKSPACE
        with pytest.raises(RuntimeError, match="workspace"):
            _native._raise(_native.MIVQ_ERR_WORKSPACE)


# ------------------------------------------------------------------ save / load
def _fixture_quantizer(z, g, name, packing, codebook, engine="saq"):
    q = RR.fixture_quantizer(g, name, packing)
    q.codebook, q.codebook_engine = codebook, engine
    if codebook != "gaussian":
        q.cb = RR.split_cb(z[f"{name}_cb_{codebook}"], q.bits)
    return q


@pytest.mark.parametrize("packing", RR.PACKINGS)
def test_save_load_round_trip_keeps_fitted_tables(z, golden_dir, tmp_path, packing):
    from haag_vq.methods.search.flat_quantized_index import quantizer_from_state, quantizer_state

    g = RR.load_golden(golden_dir)
    q = _fixture_quantizer(z, g, "w08", packing, "exact", "device")
    path = tmp_path / "exact.npz"
    np.savez(path, **quantizer_state(q))
    with np.load(path, allow_pickle=False) as f:
        assert str(f["codebook"]) == "exact" and str(f["codebook_engine"]) == "device"
        got = quantizer_from_state(f)
    assert got.codebook == "exact" and got.codebook_engine == "device" and got.packing == packing
    assert _same_bits(np.concatenate(got.cb), z["w08_cb_exact"]) and np.array_equal(got.bits, q.bits)
    assert got.code_size == q.code_size and np.array_equal(got.field_positions(), q.field_positions())


OLD_MEMBERS = ["qtype", "avg_bits", "alpha", "max_bits", "seed", "packing", "mu", "V", "var", "bits", "cb", "levels", "Dg"]


def test_gaussian_quantizer_file_is_unchanged(z, golden_dir, tmp_path):
    """The new members are written only when they differ from the defaults: the state of a
    gaussian quantizer has the members it had, in their order, and a file without the new ones
    loads as gaussian / saq and saves to the same members again."""
    from haag_vq.methods.search.flat_quantized_index import quantizer_from_state, quantizer_state

    g = RR.load_golden(golden_dir)
    st = quantizer_state(_fixture_quantizer(z, g, "w08", "dense", "gaussian"))
    assert list(st) == OLD_MEMBERS
    path = tmp_path / "gaussian.npz"
    np.savez(path, **st)
    with np.load(path, allow_pickle=False) as f:
        assert list(f.files) == OLD_MEMBERS
        back = quantizer_from_state(f)
    assert back.codebook == "gaussian" and back.codebook_engine == "saq"
    again = quantizer_state(back)
    assert list(again) == OLD_MEMBERS and all(_same_bits(again[m], st[m]) for m in OLD_MEMBERS)
    lloyd = quantizer_state(_fixture_quantizer(z, g, "w08", "dense", "lloyd"))
    assert list(lloyd) == OLD_MEMBERS + ["codebook"] and str(lloyd["codebook"]) == "lloyd"
