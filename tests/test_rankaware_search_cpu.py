"""CPU: the rank-aware code search's C ABI (symbols, size query, argument checks), the index
class's constructor, and the bound its GPU tests use, evaluated in numpy on the reference's
fixture (tests/golden/rankaware_golden.npz)."""

import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

import _rankaware_rule as RR
import _rankaware_search_rule as RS

ROOT = Path(__file__).resolve().parents[1]
NAMES = ("mivq_rankaware_flat_search_workspace_bytes", "mivq_rankaware_flat_search")


@pytest.fixture(scope="module")
def z(golden_dir):
    return RR.load_golden(golden_dir)


def test_symbols_declared_exported_and_bound():
    from haag_vq import _native

    txt = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "mivq.h").read_text(), flags=re.S)
    lib = _native.load_library()
    for name in NAMES:
        assert re.search(rf"\b{name}\s*\(", txt), name
        assert name in _native.SIGNATURES and hasattr(lib, name), name
    assert len(_native.SIGNATURES["mivq_rankaware_flat_search"][1]) == 18
    assert lib.mivq_abi_version() == 2


def test_size_query_needs_no_gpu():
    from haag_vq import _native

    fn = _native.load_library().mivq_rankaware_flat_search_workspace_bytes
    for shape in ((1, 1_000_000, 1024, 512, 10), (15, 4095, 1536, 1536, 256), (16, 4096, 37, 14, 10),
                  (1000, 1_000_000, 1024, 512, 10), (3, 1, 5, 1, 1)):
        assert fn(*shape) > 0, shape
    for shape in ((0, 10, 8, 4, 1), (1, 0, 8, 4, 1), (1, 10, 0, 4, 1), (1, 10, 8, 0, 1), (1, 10, 8, 4, 0)):
        assert fn(*shape) == 0, shape
    # top-k lists or a block of keys, never decoded rows: far below the 4 GB of 1M x 1024 floats
    assert fn(1, 1_000_000, 1024, 512, 10) < 2 ** 20 and fn(1000, 1_000_000, 1024, 512, 10) < 2 ** 30


def test_invalid_arguments_need_no_gpu():
    """Every refusal comes before any launch, so it needs no device; the pointers are host
    buffers that are never read."""
    from haag_vq import _native

    lib = _native.load_library()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)

    def call(nq=2, n=5, d=8, cs=4, metric=_native.METRIC_L2, k=3, id_offset=0, null=()):
        ptr = {nm: (None if nm in null else p) for nm in ("qy", "codes", "lv32", "lv_off", "pos", "width", "ws", "dists",
                                                          "ids")}
        return lib.mivq_rankaware_flat_search(ptr["qy"], nq, ptr["codes"], n, d, ptr["lv32"], ptr["lv_off"], ptr["pos"],
                                              ptr["width"], cs, metric, k, id_offset, ptr["ws"], 64, ptr["dists"],
                                              ptr["ids"], None)

    for bad in (dict(n=-1), dict(nq=-1), dict(d=0), dict(d=-3), dict(cs=0), dict(cs=-1), dict(k=0), dict(k=-1),
                dict(metric=2), dict(metric=-1), dict(id_offset=-1), dict(id_offset=2 ** 32 - 5)):
        assert call(**bad) == _native.MIVQ_ERR_INVALID, bad
        assert b"rankaware_flat_search" in lib.mivq_last_error()
    for nm in ("qy", "codes", "lv32", "lv_off", "pos", "width", "dists", "ids"):
        assert call(null=(nm,)) == _native.MIVQ_ERR_INVALID, nm
    assert call(n=0, null=("dists",)) == _native.MIVQ_ERR_INVALID
    assert call(k=257) == _native.MIVQ_ERR_UNSUPPORTED
    assert call(cs=48001) == _native.MIVQ_ERR_UNSUPPORTED
    assert call(nq=0, null=("qy", "codes", "dists", "ids")) == _native.MIVQ_OK
    with pytest.raises(ValueError):
        _native._raise(call(d=0))


def test_index_refuses_other_quantizers():
    from haag_vq.methods.rank_aware_quantization import RankAwareQuantizer
    from haag_vq.methods.scalar_quantization import ScalarQuantizer
    from haag_vq.methods.search import FlatQuantizedIndex, RankAwareFlatIndex

    with pytest.raises(ValueError, match="RankAwareQuantizer"):
        RankAwareFlatIndex(ScalarQuantizer(8))
    idx = RankAwareFlatIndex(RankAwareQuantizer(avg_bits=2))
    assert isinstance(idx, FlatQuantizedIndex) and idx.memory_footprint() == 0


def test_state_keeps_its_positional_fields():
    from haag_vq import _native

    assert _native.RankAwareState._fields[:7] == ("mu", "V", "lv", "lv_off", "pos", "width", "code_size")
    assert _native.RankAwareState(1, 2, 3, 4, 5, 6, 7).lv32 is None


@pytest.mark.parametrize("name", list(RR.CASES))
def test_rotated_chain_within_the_bound(z, name):
    """The f32 chain in the rotated domain and the f32 chain over the reference's reconstruction
    both lie within l2_slack of the fp64 value ||(q - mu) V - y_hat||^2, and rank the same ten
    rows first; likewise the IP chain under ip_slack."""
    st = RR.fixture_state(z, name, "dense")
    D = st.D
    Q = RS.queries(name)
    assert Q.shape == (RS.NQ, D) and Q.dtype == np.float32
    rec = z[f"{name}_rec"]
    Yh = RS.levels(z[f"{name}_dense_codes"], st)
    assert np.array_equal(Yh, RS.levels(z[f"{name}_ffd_codes"], RR.fixture_state(z, name, "ffd")))
    A, Aip = RS.rotate(Q, st, "l2"), RS.rotate(Q, st, "ip")
    a32, b32 = A.astype(np.float32), Yh.astype(np.float32)
    worst = 0.0
    for i in range(RS.NQ):
        truth = ((A[i] - Yh) ** 2).sum(axis=1)
        rot = RS.chain_l2(a32[i], b32)
        org = RS.chain_l2(Q[i], rec)
        s_rot, s_org = RS.l2_slack(a32[i], b32, D), RS.l2_slack(Q[i], rec, D)
        worst = max(worst, float(np.max(np.abs(rot - truth) / s_rot)), float(np.max(np.abs(org - truth) / s_org)))
        assert np.all(np.abs(rot - truth) <= s_rot) and np.all(np.abs(org - truth) <= s_org), i
        assert set(RS.top_ids(rot)) == set(RS.top_ids(org)), i
        ip_truth = Aip[i] @ Yh.T + float(Q[i].astype(np.float64) @ st.mu)
        mu_norm = float(np.linalg.norm(st.mu))
        key = RS.chain_ip(Aip[i].astype(np.float32), b32)
        score = (key + np.float32(Q[i].astype(np.float64) @ st.mu)).astype(np.float32)
        assert np.all(np.abs(score - ip_truth) <= RS.ip_slack(Aip[i], Yh, D, mu_norm)), i
        assert np.all(np.abs(RS.chain_ip(Q[i], rec) - ip_truth) <= RS.ip_slack(Q[i], rec, D, mu_norm)), i
    print(f"{name}: worst L2 error / slack {worst:.4f} (slack = (D + 8) 2^-23 (|a| + |b|)^2, D + 8 = {D + 8})")
