"""CPU: the IvfListPqIndex rule against the fp64 Judge, and the ABI and host logic of the per-list
PQ entry points (no GPU).

The device side (decode, the search over probed lists, the index end to end) is held to the rule
in tests/test_ivf_listpq_gpu.py.
"""

import re
from pathlib import Path

import numpy as np
import pytest

import _ivf_listpq_rule as PR
from _search_rule import OPEN_CAP

ROOT = Path(__file__).resolve().parents[1]
SYMBOLS = ("mivq_ivf_listpq_decode", "mivq_ivf_listpq_search_workspace_bytes", "mivq_ivf_listpq_search")
GIB = 1 << 30
CASE_IDS = [(n, m) for n in PR.CASES for m in PR.METRICS]


@pytest.fixture(scope="module")
def cases(oracle):
    return {(n, m): PR.Case(oracle, n, m) for n, m in CASE_IDS}


# ------------------------------------------------------------------------------ the rule
@pytest.mark.parametrize("name,metric", CASE_IDS)
def test_rule_expected_passes_the_judge(cases, oracle, name, metric):
    c = cases[(name, metric)]
    counts = np.bincount(c.assign, minlength=PR.K)
    assert (counts == 0).sum() == 1 and (counts[counts > 0] >= 1 << c.B).all(), counts  # one empty list
    assert counts.max() - counts[counts > 0].min() <= 1, counts  # rows dealt evenly
    share = PR.open_share(c.judges)
    print(f"\n[ivf-listpq] {name} {metric}: open share {share:.4f}")
    assert share <= OPEN_CAP
    dd, ii = c.expected(oracle)
    assert dd.dtype == np.float32 and ii.dtype == np.uint32 and dd.shape == ii.shape == (PR.NQ, PR.TOPK)
    assert (ii != PR.NO_ID).all() and np.isfinite(dd).all()
    bad = PR.problems(c.judges, ii, dd, metric, tie_order=True)
    assert not bad, bad[:3]


def test_decode_is_the_gather_of_the_shifted_codebook(cases, oracle):
    c = cases[("m8_b4_d40", "l2")]
    dsub = c.D // c.M
    for i in (0, 1, 2, 699):
        l = c.assign[i]
        e = PR.shifted(c.cb[l], c.coarse[l])
        want = np.concatenate([e[m, c.codes[i, m]] for m in range(c.M)])
        assert want.shape == (c.M * dsub,)
        np.testing.assert_array_equal(c.rec[i].view(np.uint32), want.view(np.uint32))


def test_tied_keys_come_in_id_order(cases, oracle):
    """m2_b8_d200: distinct rows share a code, so their keys tie exactly; the smaller uint32 id first."""
    c = cases[("m2_b8_d200", "l2")]
    ids = c.list_ids.copy()
    ids[::3] |= np.uint32(1 << 31)  # uint32 order, not int32
    nrows = int(c.offsets[-1])
    dd, ii = c.expected(oracle, k=256, list_ids=ids)
    ties = 0
    for a in range(PR.NQ):
        same = dd[a, 1:] == dd[a, :-1]
        real = ii[a, 1:] != PR.NO_ID
        ties += int((same & real).sum())
        assert (ii[a, 1:][same & real] > ii[a, :-1][same & real]).all()
    assert ties > 0 and nrows == c.N


def test_expected_pads_skips_and_ignores_slot_order(cases, oracle):
    c = cases[("m8_b4_d40", "l2")]
    probes = c.probe_l.copy()
    d0, i0 = c.expected(oracle, probes)
    d1, i1 = c.expected(oracle, probes[:, ::-1])
    np.testing.assert_array_equal(i0, i1)
    np.testing.assert_array_equal(d0.view(np.uint32), d1.view(np.uint32))
    probes[0, :] = PR.NO_ID      # every slot skipped
    probes[1, 1:] = PR.K + 5     # ids >= nlist are skipped too
    empty = int(np.flatnonzero(np.diff(c.offsets) == 0)[0])
    probes[2, :] = empty         # the empty list
    d2, i2 = c.expected(oracle, probes, k=256)
    for a in (0, 2):
        assert (i2[a] == PR.NO_ID).all() and np.isinf(d2[a]).all()
    n1 = int(c.offsets[c.probe_l[1, 0] + 1] - c.offsets[c.probe_l[1, 0]])
    assert n1 < 256 and (i2[1, :n1] != PR.NO_ID).all() and (i2[1, n1:] == PR.NO_ID).all() and np.isinf(d2[1, n1:]).all()
    assert (np.diff(d2[1, :n1]) >= 0).all()


# ------------------------------------------------------------------------------ ABI
def test_header_declares_the_symbols():
    txt = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "mivq.h").read_text(), flags=re.S)
    names = set(re.findall(r"\b(mivq_[a-z0-9_]+)\s*\(", txt))
    from haag_vq import _native

    for s in SYMBOLS:
        assert s in names, s
        assert s in _native.SIGNATURES, s
        assert hasattr(_native.load_library(), s), s
        decl = re.search(rf"\b{s}\s*\(([^)]*)\)", txt).group(1)
        assert len(decl.split(",")) == len(_native.SIGNATURES[s][1]), s
    assert "#define MIVQ_ABI_VERSION 2" in txt  # symbols were only added


def test_header_documents_the_arithmetic():
    txt = (ROOT / "include" / "mivq.h").read_text()
    for line in ("e[m][j][t] = cb[l][m][j][t] + c[m*dsub + t]",
                 "T[m][j] = fmaf chain over t ascending of (q_{m*dsub+t} - e[m][j][t])^2",
                 "T[m][j] = -(fmaf chain over t ascending of q_{m*dsub+t} * e[m][j][t])",
                 "((T[0][code_0] + T[1][code_1]) + ...) + T[M-1][code_{M-1}]"):
        assert line in txt, line


def test_exports():
    from haag_vq.methods.base_search_index import BaseSearchIndex
    from haag_vq.methods.search import IvfListPqIndex, __all__ as names
    from haag_vq.methods.search.ivf_listpq_index import IvfListPqIndex as Direct

    assert IvfListPqIndex is Direct and "IvfListPqIndex" in names and issubclass(IvfListPqIndex, BaseSearchIndex)


def test_workspace_query_needs_no_gpu():
    from haag_vq import _native

    fn = _native.load_library().mivq_ivf_listpq_search_workspace_bytes
    # (nq, n, nlist, nprobe, d, M, nbits, k)
    assert fn(100, 10_000, 16, 4, 64, 8, 8, 10) > 0
    assert fn(100, 10_000, 16, 4, 64, 64, 8, 10) > 0      # dsub = 1
    assert fn(100, 10_000, 16, 4, 1024, 1024, 8, 10) > 0  # 1 MB of table per pair: no LDS limit
    for nq in (1000, 10_000):
        nb = fn(nq, 1_000_000, 1024, 64, 1024, 128, 8, 10)
        print(f"\n[ivf-listpq] workspace at nq {nq}, n 1M, nlist 1024, nprobe 64, d 1024, M 128, k 10: {nb / 2**20:.1f} MiB")
        # the per-pair regions are chunked under 1 GiB; the fixed ones (list offsets, work items,
        # sort histogram) do not grow with the queries
        assert 0 < nb <= GIB
    assert fn(10_000, 1_000_000, 1024, 64, 1024, 128, 8, 10) == fn(100_000, 1_000_000, 1024, 64, 1024, 128, 8, 10)
    assert fn(100, 10_000, 16, 4, 64, 8, 8, 257) == 0 and fn(100, 10_000, 16, 4, 64, 8, 8, 0) == 0
    assert fn(100, 10_000, 16, 4, 0, 8, 8, 10) == 0 and fn(100, 10_000, 0, 4, 64, 8, 8, 10) == 0
    assert fn(100, 10_000, 16, 0, 64, 8, 8, 10) == 0 and fn(-1, 10_000, 16, 4, 64, 8, 8, 10) == 0
    assert fn(100, -1, 16, 4, 64, 8, 8, 10) == 0
    assert fn(100, 10_000, 16384, 4, 64, 8, 8, 10) == 0
    assert fn(100, 10_000, 16, 4, 64, 7, 8, 10) == 0 and fn(100, 10_000, 16, 4, 64, 0, 8, 10) == 0
    assert fn(100, 10_000, 16, 4, 64, 8, 9, 10) == 0 and fn(100, 10_000, 16, 4, 64, 8, 0, 10) == 0
    # sized on shape alone: the number of stored rows does not enter
    assert fn(100, 10, 16, 4, 64, 8, 8, 10) == fn(100, 10_000_000, 16, 4, 64, 8, 8, 10)


def test_bad_arguments_are_rejected_before_any_hip_call():
    """Null pointers, no GPU: validation comes first."""
    from haag_vq import _native

    lib = _native.load_library()
    INV, UNS, OK = _native.MIVQ_ERR_INVALID, _native.MIVQ_ERR_UNSUPPORTED, _native.MIVQ_OK

    def search(nq=4, d=64, M=8, nbits=8, nlist=16, nprobe=4, metric=1, k=10):
        return lib.mivq_ivf_listpq_search(None, nq, d, M, nbits, None, None, nlist, None, nprobe, None, None, None,
                                          metric, k, None, 0, None, None, None)

    assert search(k=300) == UNS and b"k=300" in lib.mivq_last_error()
    assert search(k=0) == UNS and b"k=0" in lib.mivq_last_error()
    assert search(nlist=16384) == UNS and b"nlist=16384" in lib.mivq_last_error()
    assert search(metric=7) == UNS
    assert search(M=7) == INV and b"M=7" in lib.mivq_last_error()
    with pytest.raises(AssertionError, match="divisible"):  # the error of ProductQuantizer.fit
        _native._raise(INV)
    assert search(M=0) == INV
    for bad in (0, 9):
        assert search(nbits=bad) == INV and b"nbits=%d" % bad in lib.mivq_last_error()
    assert search(nlist=0) == INV and b"nlist=0" in lib.mivq_last_error()
    assert search(d=0) == INV and search(nprobe=0) == INV and search(nq=-1) == INV
    assert search() == INV and b"null pointer" in lib.mivq_last_error()
    assert search(nq=0) == OK  # nothing to do
    assert search(nq=0, k=300) == UNS  # the limits come before the early return

    def decode(n=4, d=64, M=8, nbits=8, nlist=16):
        return lib.mivq_ivf_listpq_decode(None, n, d, M, nbits, None, None, nlist, None, None, None)

    assert decode(d=0) == INV and decode(n=-1) == INV and decode(nlist=0) == INV and decode(M=0) == INV
    assert decode(M=7) == INV and b"M=7" in lib.mivq_last_error()
    assert decode(nbits=9) == INV and b"nbits=9" in lib.mivq_last_error()
    assert decode() == INV and b"null pointer" in lib.mivq_last_error()
    assert decode(n=0) == OK


# ------------------------------------------------------------------------------ index host logic
def test_short_list_message():
    from haag_vq.methods._ivf import short_list_error

    assert short_list_error(np.array([0, 256, 300, 0]), 8) is None
    msg = short_list_error(np.array([300, 0, 255, 1]), 8)
    assert "Number of training points (255) should be at least as large as number of clusters (256)" in msg
    assert "list 2" in msg and "2 non-empty lists" in msg and "smaller K or B" in msg
    assert short_list_error(np.array([300, 0, 255, 16]), 4) is None
    assert "list 1 of 2 (1 non-empty list holds" in short_list_error(np.array([16, 15]), 4)


def test_index_host_logic(tmp_path):
    from haag_vq.methods.product_quantization import ProductQuantizer
    from haag_vq.methods.scalar_quantization import ScalarQuantizer
    from haag_vq.methods.search import IvfListPqIndex

    calls = []

    def factory():
        calls.append(1)
        q = ProductQuantizer(M=4, B=6)
        q.niter, q.seed = 3, 77
        return q

    idx = IvfListPqIndex(factory)
    assert len(calls) == 1 and (idx._M, idx._B, idx._niter, idx._seed, idx._K, idx.nprobe) == (4, 6, 3, 77, 4096, 200)
    idx.nprobe = 7
    assert idx.nprobe == 7
    with pytest.raises(ValueError, match="ProductQuantizer.*ScalarQuantizer"):
        IvfListPqIndex(lambda: ScalarQuantizer(num_bits=8))
    for K, nprobe in ((0, 4), (-1, 4), (4, 0), (4, -2)):
        with pytest.raises(ValueError, match="positive"):
            IvfListPqIndex(factory, K=K, nprobe=nprobe)
    Q = np.zeros((2, 8), np.float32)
    for call in (lambda: idx.search(Q, 3), lambda: idx.search_with_scores(Q, 3), lambda: idx.search_device(Q, 3),
                 lambda: idx.save(tmp_path / "unfit.npz")):
        with pytest.raises(RuntimeError, match="fit"):
            call()
    assert not (tmp_path / "unfit.npz").exists()
    assert idx.memory_footprint() == 0 and idx.ntotal == 0 and idx.reconstruction_mse(Q) is None
