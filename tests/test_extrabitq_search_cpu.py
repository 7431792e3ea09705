"""CPU: the Extended RaBitQ code search's C ABI (symbols, size query, argument checks), the index
class's constructor and state round trip, and the definition of the rotated-domain search
(_extrabitq_search_rule) on the reference-generated cases erq1 / erq4 of
tests/golden/search_golden.npz, whose state and codes are those of extrabitq_golden.npz."""

import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

import _extrabitq_search_rule as ES
import _rankaware_search_rule as RS
import _search_rule as R

ROOT = Path(__file__).resolve().parents[1]
NAMES = ("mivq_extrabitq_flat_search_workspace_bytes", "mivq_extrabitq_flat_search")
ERQ_CASES = ("erq1", "erq4")


@pytest.fixture(scope="module")
def sg(golden_dir):
    with np.load(golden_dir / "search_golden.npz") as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def erq(golden_dir):
    with np.load(golden_dir / "extrabitq_golden.npz") as z:
        return {k: z[k] for k in z.files}


def test_symbols_declared_exported_and_bound():
    from haag_vq import _native

    txt = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "mivq.h").read_text(), flags=re.S)
    lib = _native.load_library()
    for name in NAMES:
        assert re.search(rf"\b{name}\s*\(", txt), name
        assert name in _native.SIGNATURES and hasattr(lib, name), name
    assert len(_native.SIGNATURES["mivq_extrabitq_flat_search"][1]) == 15
    assert callable(_native.extrabitq_flat_search) and callable(_native.extrabitq_dequantize)
    assert lib.mivq_abi_version() == 2


def test_size_query_needs_no_gpu():
    from haag_vq import _native

    fn = _native.load_library().mivq_extrabitq_flat_search_workspace_bytes
    for shape in ((1, 1_000_000, 1024, 10), (15, 4095, 1536, 256), (16, 4096, 37, 10), (1000, 1_000_000, 1024, 10),
                  (3, 1, 5, 1)):
        assert fn(*shape) > 0, shape
    for shape in ((0, 10, 8, 1), (1, 0, 8, 1), (1, 10, 0, 1), (1, 10, 8, 0)):
        assert fn(*shape) == 0, shape
    # top-k lists or a block of keys, never decoded rows: far below the 4 GB of 1M x 1024 floats
    assert fn(1, 1_000_000, 1024, 10) < 2 ** 20 and fn(1000, 1_000_000, 1024, 10) < 2 ** 30


def test_invalid_arguments_need_no_gpu():
    """Every refusal comes before any launch, so it needs no device; the pointers are host
    buffers that are never read."""
    from haag_vq import _native

    lib = _native.load_library()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)

    def call(nq=2, n=5, d=8, nbits=4, metric=_native.METRIC_L2, k=3, id_offset=0, null=(), ws_bytes=64):
        ptr = {nm: (None if nm in null else p) for nm in ("qy", "codes", "levels", "ws", "dists", "ids")}
        return lib.mivq_extrabitq_flat_search(ptr["qy"], nq, ptr["codes"], n, d, ptr["levels"], nbits, metric, k,
                                              id_offset, ptr["ws"], ws_bytes, ptr["dists"], ptr["ids"], None)

    for bad in (dict(n=-1), dict(nq=-1), dict(d=0), dict(d=-3), dict(k=0), dict(k=-1), dict(id_offset=-1),
                dict(id_offset=2 ** 32 - 5)):
        assert call(**bad) == _native.MIVQ_ERR_INVALID, bad
        assert b"extrabitq_flat_search" in lib.mivq_last_error()
    for nbits in (0, 9, -1):
        assert call(nbits=nbits) == _native.MIVQ_ERR_INVALID
        assert lib.mivq_last_error() == f"num_bits must be in [1, 8], got {nbits}".encode()
    for nm in ("qy", "codes", "levels", "dists", "ids"):
        assert call(null=(nm,)) == _native.MIVQ_ERR_INVALID, nm
        assert b"null pointer" in lib.mivq_last_error()
    assert call(n=0, null=("dists",)) == _native.MIVQ_ERR_INVALID
    assert call(id_offset=2 ** 32 - 1 - 5 + 1) == _native.MIVQ_ERR_INVALID and b"ids overflow" in lib.mivq_last_error()
    assert call(k=257) == _native.MIVQ_ERR_UNSUPPORTED
    assert call(metric=2) == _native.MIVQ_ERR_UNSUPPORTED
    assert call(d=50_000) == _native.MIVQ_ERR_UNSUPPORTED          # 200 KB of one query: no LDS holds it
    assert b"too large for LDS" in lib.mivq_last_error()
    # 160 KiB of LDS less the level table: the widest single query of the scan
    assert call(d=40_448) == _native.MIVQ_ERR_WORKSPACE and call(d=40_452) == _native.MIVQ_ERR_UNSUPPORTED
    assert call(ws_bytes=0) == _native.MIVQ_ERR_WORKSPACE and call(null=("ws",)) == _native.MIVQ_ERR_WORKSPACE
    assert call(nq=0, null=("qy", "codes", "levels", "dists", "ids")) == _native.MIVQ_OK
    with pytest.raises(ValueError):
        _native._raise(call(d=0))


def test_index_refuses_other_quantizers_and_unfitted_use(tmp_path):
    from haag_vq.methods.extended_rabitq import ExtendedRaBitQuantizer
    from haag_vq.methods.scalar_quantization import ScalarQuantizer
    from haag_vq.methods.search import ExtendedRaBitQFlatIndex, FlatQuantizedIndex
    from haag_vq.methods.search.flat_quantized_index import quantizer_state

    with pytest.raises(ValueError, match="ExtendedRaBitQuantizer"):
        ExtendedRaBitQFlatIndex(ScalarQuantizer(8))
    idx = ExtendedRaBitQFlatIndex(ExtendedRaBitQuantizer(num_bits=4))
    assert isinstance(idx, FlatQuantizedIndex) and idx.memory_footprint() == 0
    with pytest.raises(RuntimeError, match="fit"):
        idx.search_with_scores(np.zeros((2, 8), np.float32), 3)
    with pytest.raises(RuntimeError, match="fit"):
        idx.quantizer.rotate_queries(np.zeros((2, 8), np.float32))
    with pytest.raises(RuntimeError, match="fit"):
        idx.save(tmp_path / "unfitted.npz")
    assert not (tmp_path / "unfitted.npz").exists()
    with pytest.raises(ValueError, match="not fitted"):
        quantizer_state(idx.quantizer)


def test_state_round_trip(erq):
    from haag_vq.methods.extended_rabitq import ExtendedRaBitQuantizer
    from haag_vq.methods.search.flat_quantized_index import quantizer_from_state, quantizer_state

    q = ExtendedRaBitQuantizer(num_bits=4, seed=3)
    q.c, q.P, q.levels, q.D = erq["b4_c"], erq["b4_P"], erq["b4_levels"], 64
    st = quantizer_state(q)
    assert str(st["qtype"]) == "extrabitq"
    assert all(st[nm].dtype == np.float64 for nm in ("c", "P", "levels"))
    back = quantizer_from_state(st)
    assert type(back) is ExtendedRaBitQuantizer
    assert (back.num_bits, back.seed, back.D) == (4, 3, 64)
    for nm in ("c", "P", "levels"):
        assert getattr(back, nm).dtype == np.float64 and np.array_equal(getattr(back, nm), getattr(q, nm)), nm
    bad = dict(st, levels=st["levels"][:-1])
    with pytest.raises(ValueError, match="inconsistent"):
        quantizer_from_state(bad)


def test_pack_and_unpack_are_inverse():
    rng = np.random.default_rng(3)
    for B, D in ((3, 37), (5, 70), (8, 5), (1, 9)):
        idx = rng.integers(0, 1 << B, size=(7, D))
        nrm, t = rng.standard_normal(7).astype(np.float32), rng.standard_normal(7).astype(np.float32)
        for pad_ones in (False, True):
            codes = ES.pack(idx, nrm, t, B, pad_ones)
            assert codes.shape == (7, ES.code_size(D, B))
            i2, n2, t2 = ES.unpack(codes, D, B)
            assert np.array_equal(i2, idx) and np.array_equal(n2, nrm) and np.array_equal(t2, t)


@pytest.mark.parametrize("metric", R.METRICS)
@pytest.mark.parametrize("name", ERQ_CASES)
def test_rotated_search_returns_the_reference_ids(oracle, sg, erq, name, metric):
    """The definition alone (numpy chains in the rotated domain) returns the ids the reference's
    FlatQuantizedIndex stored, and passes the rule of _search_rule against the oracle's decode."""
    c = R.CASES[name]
    B, D, k = c["bits"], c["D"], c["k"]
    t = f"b{B}"
    X, Q = R.inputs(name, erq["X"])
    assert R.sha(Q) == str(sg[f"{name}_Q_sha"])
    codes = erq[f"{t}_codes"]
    assert R.sha(codes) == str(sg[f"{name}_codes_sha"])
    state = (erq[f"{t}_c"], erq[f"{t}_P"], erq[f"{t}_levels"])
    xh = oracle.extrabitq_decode(codes, *state, B)
    judge = R.Judge(Q, xh, metric, k)
    assert judge.open_share == 0.0
    ids, dists = ES.search(Q, codes, *state, B, k, metric)
    assert np.array_equal(ids, sg[f"{name}_{metric}_ids"])
    judge.check(ids, dists, f"{name} {metric} rotated rule")
    print(f"{name} {metric}: max |dist - key| / e {judge.ratio(ids, dists):.4f}")
    # and the chain lies within the derived slack of the fp64 value in the rotated domain
    A = ES.rotate(Q, state[0], state[1], metric)
    Yh = ES.y_hat(codes, state[2], D, B).astype(np.float64)
    for j in range(len(Q)):
        r = ids[j].astype(np.int64)
        if metric == "l2":
            truth = ((A[j] - Yh) ** 2).sum(axis=1)
            assert np.all(np.abs(dists[j] - truth[r]) <= RS.l2_slack(A[j], Yh, D)[r]), j
        else:
            truth = A[j] @ Yh.T + float(Q[j].astype(np.float64) @ state[0])
            assert np.all(np.abs(dists[j] - truth[r]) <= RS.ip_slack(A[j], Yh, D, float(np.linalg.norm(state[0])))[r]), j
