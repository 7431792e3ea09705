"""CPU: the IvfQuantizedIndex rule against the reference's fixture, and the ABI and host logic of
the per-list SQ / LVQ entry points (no GPU).

The device side (fit, encode, decode, the search over probed lists, the index end to end) is
held to the rule in tests/test_ivf_quantized_gpu.py.
"""

import re
from pathlib import Path

import numpy as np
import pytest

import _ivf_quantized_rule as IR

ROOT = Path(__file__).resolve().parents[1]
GOLDEN = ROOT / "tests" / "golden"
SYMBOLS = ("mivq_ivf_sq_fit", "mivq_ivf_sq_encode", "mivq_ivf_sq_decode", "mivq_ivf_lvq_encode", "mivq_ivf_lvq_decode",
           "mivq_ivf_sq_search_workspace_bytes", "mivq_ivf_sq_search", "mivq_ivf_lvq_search_workspace_bytes",
           "mivq_ivf_lvq_search")
GIB = 1 << 30
CASE_IDS = [(n, m) for n in IR.CASES for m in IR.METRICS]


@pytest.fixture(scope="module")
def cases(oracle):
    fx = IR.load_fixture(GOLDEN)
    assert list(fx["cases"]) == list(IR.CASES)
    return {(n, m): IR.Case(oracle, n, m, fx) for n, m in CASE_IDS}


# ------------------------------------------------------------------------------ rule vs fixture
@pytest.mark.parametrize("name,metric", CASE_IDS)
def test_rule_reproduces_the_reference_parameters_and_codes(cases, name, metric):
    c = cases[(name, metric)]
    key = f"{name}_{metric}"
    counts = np.bincount(c.assign, minlength=IR.K)
    assert (counts == 0).sum() == 1, counts  # one empty list
    np.testing.assert_array_equal(IR.assign64(c.X, c.coarse, metric), c.assign)
    np.testing.assert_array_equal(IR.probes64(c.Q, c.coarse, metric, IR.NPROBE), c.probe_l)
    names = ("lo", "den") if c.kind == "sq" else ("mu",)
    for pname, p in zip(names, c.params):
        ref = c.fx[f"{key}_{pname}"]
        assert p.dtype == ref.dtype == np.float32
        np.testing.assert_array_equal(p.view(np.uint32), ref.view(np.uint32), err_msg=f"{key} {pname}")
    ref_head = c.fx[f"{key}_codes_head"]
    assert c.codes.dtype == ref_head.dtype
    np.testing.assert_array_equal(c.codes[:8], ref_head)
    assert IR.sha(c.codes) == str(c.fx[f"{key}_codes_sha"]), f"{key}: codes differ from the reference's"


@pytest.mark.parametrize("name,metric", CASE_IDS)
def test_reference_result_passes_the_judge_on_the_rule_reconstruction(cases, name, metric):
    c = cases[(name, metric)]
    share = IR.open_share(c.judges)
    print(f"\n[ivf-quantized] {name} {metric}: open share {share:.4f}")
    from _search_rule import OPEN_CAP

    assert share <= OPEN_CAP
    np.testing.assert_array_equal(np.stack([j.open[0] for j, _ in c.judges]), c.fx[f"{name}_{metric}_open"])
    ids, dists = c.ref()
    assert ids.shape == dists.shape == (IR.NQ, IR.TOPK) and ids.dtype == np.uint32 and dists.dtype == np.float32
    # the reference sums in numpy's pairwise order and breaks ties by argpartition: no tie order
    bad = IR.problems(c.judges, ids, dists, metric, tie_order=False)
    assert not bad, bad[:3]


@pytest.mark.parametrize("name,metric", CASE_IDS)
def test_rule_expected_passes_the_judge(cases, oracle, name, metric):
    c = cases[(name, metric)]
    dd, ii = c.expected(oracle)
    assert (ii != IR.NO_ID).all() and np.isfinite(dd).all()
    bad = IR.problems(c.judges, ii, dd, metric, tie_order=True)
    assert not bad, bad[:3]


def test_expected_pads_skips_and_ignores_slot_order(cases, oracle):
    c = cases[("sq8_d37", "l2")]
    args = (oracle, c.list_codes, c.list_ids, c.offsets, c.coarse, c.params, c.kind, c.bits, c.Q)
    probes = c.probe_l.copy()
    d0, i0 = IR.expected(*args, probes, IR.L2, IR.TOPK)
    d1, i1 = IR.expected(*args, probes[:, ::-1], IR.L2, IR.TOPK)
    np.testing.assert_array_equal(i0, i1)
    np.testing.assert_array_equal(d0.view(np.uint32), d1.view(np.uint32))
    probes[0, :] = IR.NO_ID      # every slot skipped
    probes[1, 1:] = IR.K + 5     # ids >= nlist are skipped too
    d2, i2 = IR.expected(*args, probes, IR.L2, 256)
    assert (i2[0] == IR.NO_ID).all() and np.isinf(d2[0]).all()
    n1 = int(c.offsets[c.probe_l[1, 0] + 1] - c.offsets[c.probe_l[1, 0]])
    assert n1 < 256 and (i2[1, :n1] != IR.NO_ID).all() and (i2[1, n1:] == IR.NO_ID).all() and np.isinf(d2[1, n1:]).all()
    assert (np.diff(d2[1, :n1]) >= 0).all()


def test_single_row_list_and_empty_list_parameters():
    """hi == lo: den = 1e-8 and every level 0; an empty list keeps lo = 0, den = 1e-8, mu = 0."""
    rng = np.random.default_rng(3)
    X = rng.standard_normal((5, 7)).astype(np.float32)
    coarse = rng.standard_normal((3, 7)).astype(np.float32)
    assign = np.array([0, 0, 2, 0, 0])
    lo, den = IR.fit(X, coarse, assign, "sq")
    np.testing.assert_array_equal(lo[2], X[2] - coarse[2])
    assert (den[2] == np.float32(1e-8)).all() and (den[1] == np.float32(1e-8)).all() and (lo[1] == 0).all()
    for bits in (4, 8, 16):
        assert not IR.encode(X, coarse, assign, (lo, den), "sq", bits)[2].any()
    (mu,) = IR.fit(X, coarse, assign, "lvq")
    np.testing.assert_array_equal(mu[2], X[2] - coarse[2])
    assert (mu[1] == 0).all()


# ------------------------------------------------------------------------------ ABI
def test_header_declares_the_symbols():
    txt = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "mivq.h").read_text(), flags=re.S)
    names = set(re.findall(r"\b(mivq_[a-z0-9_]+)\s*\(", txt))
    from haag_vq import _native

    for s in SYMBOLS:
        assert s in names, s
        assert s in _native.SIGNATURES, s
        assert hasattr(_native.load_library(), s), s
    assert "#define MIVQ_ABI_VERSION 2" in txt  # symbols were only added
    # the ctypes table carries as many arguments as the header declares
    for s in SYMBOLS:
        decl = re.search(rf"\b{s}\s*\(([^)]*)\)", txt).group(1)
        assert len(decl.split(",")) == len(_native.SIGNATURES[s][1]), s


def test_exports():
    import haag_vq.methods as M
    from haag_vq.methods.base_search_index import BaseSearchIndex
    from haag_vq.methods.search import IvfQuantizedIndex
    from haag_vq.methods.search.ivf_quantized_index import IvfQuantizedIndex as Direct

    assert M.IvfQuantizedIndex is IvfQuantizedIndex is Direct and "IvfQuantizedIndex" in M.__all__
    assert issubclass(IvfQuantizedIndex, BaseSearchIndex)
    with pytest.raises(AttributeError):
        M.NoSuchIndex


@pytest.mark.parametrize("kind", ["sq", "lvq"])
def test_workspace_query_needs_no_gpu(kind):
    from haag_vq import _native

    fn = getattr(_native.load_library(), f"mivq_ivf_{kind}_search_workspace_bytes")
    bits = 8
    # (nq, n, nlist, nprobe, d, nbits, k)
    assert fn(100, 10_000, 16, 4, 64, bits, 10) > 0
    for nq in (1000, 100_000):
        nb = fn(nq, 1_000_000, 1024, 256, 1024, bits, 10)
        print(f"\n[ivf-{kind}] workspace at nq {nq}, n 1M, nlist 1024, nprobe 256, d 1024, k 10: {nb / 2**20:.1f} MiB")
        assert 0 < nb <= GIB  # queries are processed in chunks
    assert fn(100, 10_000, 16, 4, 64, bits, 257) == 0 and fn(100, 10_000, 16, 4, 64, bits, 0) == 0
    assert fn(100, 10_000, 16, 4, 0, bits, 10) == 0 and fn(100, 10_000, 0, 4, 64, bits, 10) == 0
    assert fn(100, 10_000, 16, 0, 64, bits, 10) == 0 and fn(-1, 10_000, 16, 4, 64, bits, 10) == 0
    assert fn(100, 10_000, 16384, 4, 64, bits, 10) == 0
    assert fn(100, 10_000, 16, 4, 64, 5 if kind == "sq" else 9, 10) == 0
    # one query row plus the list's rows (SQ: den, lo, centroid; LVQ: mu, centroid) within 160 KiB
    rows = 4 if kind == "sq" else 3
    fits = 160 * 1024 // (4 * rows) // 4 * 4
    assert fn(100, 10_000, 16, 4, fits, bits, 10) > 0
    assert fn(100, 10_000, 16, 4, fits + 4, bits, 10) == 0
    # sized on shape alone: the number of stored rows does not enter
    assert fn(100, 10, 16, 4, 64, bits, 10) == fn(100, 10_000_000, 16, 4, 64, bits, 10)


def test_bad_arguments_are_rejected_before_any_hip_call():
    """Null pointers, no GPU: validation comes first."""
    from haag_vq import _native

    lib = _native.load_library()
    INV, UNS, OK = _native.MIVQ_ERR_INVALID, _native.MIVQ_ERR_UNSUPPORTED, _native.MIVQ_OK

    def sq_search(nq=4, d=64, nlist=16, nprobe=4, nbits=8, metric=1, k=10):
        return lib.mivq_ivf_sq_search(None, nq, d, None, nlist, None, nprobe, None, None, None, None, None, nbits, metric,
                                      k, None, 0, None, None, None)

    def lvq_search(nq=4, d=64, nlist=16, nprobe=4, nbits=8, metric=1, k=10):
        return lib.mivq_ivf_lvq_search(None, nq, d, None, nlist, None, nprobe, None, None, None, None, nbits, metric, k,
                                       None, 0, None, None, None)

    for search, badbits, too_wide in ((sq_search, 5, 10244), (lvq_search, 9, 13656)):
        assert search(k=300) == UNS and b"k=300" in lib.mivq_last_error()
        assert search(k=0) == UNS
        assert search(nlist=16384) == UNS
        assert search(metric=7) == UNS
        assert search(d=too_wide) == UNS and b"LDS" in lib.mivq_last_error()
        assert search(nbits=badbits) == INV and b"num_bits" in lib.mivq_last_error()
        assert search(nlist=0) == INV and search(d=0) == INV and search(nprobe=0) == INV and search(nq=-1) == INV
        assert search() == INV and b"null pointer" in lib.mivq_last_error()
        assert search(nq=0) == OK  # nothing to do
    with pytest.raises(ValueError, match="null pointer"):
        _native._raise(INV)

    def sq_codec(fn, n=4, d=64, nlist=16, nbits=8):
        return fn(None, n, d, None, nlist, None, None, None, nbits, None, None)

    def lvq_codec(fn, n=4, d=64, nlist=16, nbits=8):
        return fn(None, n, d, None, nlist, None, None, nbits, None, None)

    for call, fns, badbits in ((sq_codec, (lib.mivq_ivf_sq_encode, lib.mivq_ivf_sq_decode), 12),
                               (lvq_codec, (lib.mivq_ivf_lvq_encode, lib.mivq_ivf_lvq_decode), 0)):
        for fn in fns:
            assert call(fn, d=0) == INV and call(fn, n=-1) == INV and call(fn, nlist=0) == INV
            assert call(fn, nbits=badbits) == INV and b"num_bits" in lib.mivq_last_error()
            assert call(fn) == INV and b"null pointer" in lib.mivq_last_error()
            assert call(fn, n=0) == OK
    fit = lib.mivq_ivf_sq_fit
    assert fit(None, 4, 0, None, 16, None, None, None, None, None) == INV
    assert fit(None, 4, 64, None, 0, None, None, None, None, None) == INV
    assert fit(None, 4, 64, None, 16, None, None, None, None, None) == INV and b"null pointer" in lib.mivq_last_error()


# ------------------------------------------------------------------------------ index host logic
def test_index_host_logic(tmp_path):
    from haag_vq.methods.lvq_quantization import LVQQuantizer
    from haag_vq.methods.product_quantization import ProductQuantizer
    from haag_vq.methods.scalar_quantization import ScalarQuantizer
    from haag_vq.methods.search import IvfQuantizedIndex

    calls = []

    def factory():
        calls.append(1)
        return ScalarQuantizer(num_bits=4)

    idx = IvfQuantizedIndex(factory)
    assert len(calls) == 1 and (idx._kind, idx._bits, idx._K, idx.nprobe) == ("sq", 4, 4096, 200)
    lv = IvfQuantizedIndex(lambda: LVQQuantizer(num_bits=3), K=16, nprobe=4)
    assert (lv._kind, lv._bits, lv._K, lv.nprobe) == ("lvq", 3, 16, 4)
    lv.nprobe = 7
    assert lv.nprobe == 7
    with pytest.raises(NotImplementedError, match="ScalarQuantizer.*LVQQuantizer"):
        IvfQuantizedIndex(lambda: ProductQuantizer(M=4, B=8))
    Q = np.zeros((2, 8), np.float32)
    for call in (lambda: idx.search(Q, 3), lambda: idx.search_with_scores(Q, 3), lambda: idx.search_device(Q, 3),
                 lambda: idx.save(tmp_path / "unfit.npz")):
        with pytest.raises(RuntimeError, match="fit"):
            call()
    assert not (tmp_path / "unfit.npz").exists()
    assert idx.memory_footprint() == 0 and idx.ntotal == 0 and idx.reconstruction_mse(Q) is None
