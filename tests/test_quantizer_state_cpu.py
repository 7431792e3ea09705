"""CPU: the saved state of every quantizer that can be built without a device.

``FORMAT`` is the output of ``quantizer_state`` before the state rules moved onto the quantizer
classes (member names in order, numpy dtypes, shapes): index files and the sharded broadcast
written before and after hold the same members.  PQ and OPQ need device codebooks; their rows are
in test_quantizer_dispatch_gpu.py.
"""

import numpy as np
import pytest

D = 6
RA_BITS = np.array([3, 2, 1, 1, 0, 0], dtype=np.int64)  # 18 levels in all
RA_MAX_BITS = 3                                         # 1 + 2 + 4 + 8 = 15 N(0,1) levels, 4 Dg


def _rank_aware(**kw):
    from haag_vq.methods.rank_aware_quantization import RankAwareQuantizer

    rng = np.random.default_rng(11)
    q = RankAwareQuantizer(2.0, alpha=0.5, max_bits=RA_MAX_BITS, seed=7, **kw)
    q.mu = rng.standard_normal(D)
    q.V = np.linalg.qr(rng.standard_normal((D, D)))[0]
    q.var = np.sort(rng.random(D))[::-1].copy()
    q.bits, q.D = RA_BITS.copy(), D
    q.cb = [np.sort(rng.standard_normal(2 ** b)) for b in RA_BITS]
    q._levels = [np.sort(rng.standard_normal(2 ** b)) for b in range(RA_MAX_BITS + 1)]
    q._Dg = rng.random(RA_MAX_BITS + 1)
    q._layout()
    return q


def _build(name):
    from haag_vq.methods.extended_rabitq import ExtendedRaBitQuantizer
    from haag_vq.methods.lvq_quantization import LVQQuantizer
    from haag_vq.methods.rabit_quantization import RaBitQuantizer
    from haag_vq.methods.scalar_quantization import ScalarQuantizer
    from haag_vq.utils.faiss_utils import MetricType

    rng = np.random.default_rng(5)
    if name in ("sq_f32", "sq_f64"):
        q = ScalarQuantizer(8 if name == "sq_f32" else 16)
        dt = np.float32 if name == "sq_f32" else np.float64
        q.min, q.max = rng.standard_normal(D).astype(dt) - 3, rng.standard_normal(D).astype(dt) + 3
    elif name == "lvq":
        q = LVQQuantizer(5)
        q.mu = rng.standard_normal(D).astype(np.float32)
    elif name == "rabitq":
        q = RaBitQuantizer(MetricType.INNER_PRODUCT)
        q.fit(np.empty((0, D), dtype=np.float32))
    elif name == "rankaware":
        q = _rank_aware(packing="ffd")
    elif name == "rankaware_lloyd":
        q = _rank_aware(codebook="lloyd", codebook_engine="device")
    else:
        assert name == "extrabitq"
        q = ExtendedRaBitQuantizer(num_bits=3, seed=2)
        q.D, q.c = D, rng.standard_normal(D)
        q.P = np.linalg.qr(rng.standard_normal((D, D)))[0]
        q.levels = np.sort(rng.standard_normal(8))
    return q


FORMAT = {
    "sq_f32": [("qtype", "<U2", ()), ("num_bits", "int64", ()), ("min", "float32", (6,)), ("max", "float32", (6,))],
    "sq_f64": [("qtype", "<U2", ()), ("num_bits", "int64", ()), ("min", "float64", (6,)), ("max", "float64", (6,))],
    "lvq": [("qtype", "<U3", ()), ("num_bits", "int64", ()), ("mu", "float32", (6,))],
    "rabitq": [("qtype", "<U6", ()), ("metric_type", "int64", ()), ("d", "int64", ())],
    "rankaware": [("qtype", "<U9", ()), ("avg_bits", "float64", ()), ("alpha", "float64", ()),
                  ("max_bits", "int64", ()), ("seed", "int64", ()), ("packing", "<U3", ()), ("mu", "float64", (6,)),
                  ("V", "float64", (6, 6)), ("var", "float64", (6,)), ("bits", "int64", (6,)),
                  ("cb", "float64", (18,)), ("levels", "float64", (15,)), ("Dg", "float64", (4,))],
    # codebook / codebook_engine are written only when they are not the defaults
    "rankaware_lloyd": [("qtype", "<U9", ()), ("avg_bits", "float64", ()), ("alpha", "float64", ()),
                        ("max_bits", "int64", ()), ("seed", "int64", ()), ("packing", "<U5", ()),
                        ("mu", "float64", (6,)), ("V", "float64", (6, 6)), ("var", "float64", (6,)),
                        ("bits", "int64", (6,)), ("cb", "float64", (18,)), ("levels", "float64", (15,)),
                        ("Dg", "float64", (4,)), ("codebook", "<U5", ()), ("codebook_engine", "<U6", ())],
    "extrabitq": [("qtype", "<U9", ()), ("num_bits", "int64", ()), ("seed", "int64", ()), ("D", "int64", ()),
                  ("c", "float64", (6,)), ("P", "float64", (6, 6)), ("levels", "float64", (8,))],
}


def _table(st):
    return [(nm, str(np.asarray(v).dtype), np.asarray(v).shape) for nm, v in st.items()]


@pytest.mark.parametrize("name", ["sq_f32", "sq_f64", "lvq", "rabitq", "rankaware", "rankaware_lloyd", "extrabitq"])
def test_state_keeps_its_format_and_round_trips(name):
    from haag_vq.methods.search.flat_quantized_index import quantizer_from_state, quantizer_state

    q = _build(name)
    st = quantizer_state(q)
    assert _table(st) == FORMAT[name]
    assert _table(q.to_state()) == FORMAT[name]
    back = quantizer_from_state(st)
    assert type(back) is type(q)
    again = quantizer_state(back)
    assert _table(again) == FORMAT[name]
    for nm in st:
        assert np.array_equal(np.asarray(again[nm]), np.asarray(st[nm])), nm
    assert type(q).from_state(st).to_state().keys() == st.keys()


def test_what_has_no_state_says_so():
    from haag_vq.methods.base_quantizer import BaseQuantizer
    from haag_vq.methods.lvq2_quantization import TwoLevelLVQQuantizer
    from haag_vq.methods.search.flat_quantized_index import quantizer_from_state, quantizer_state

    class Foreign(BaseQuantizer):
        def fit(self, X):
            pass

        def compress(self, X):
            return X

        def decompress(self, codes):
            return codes

    assert Foreign.qtype is None and Foreign.code_kind is None
    with pytest.raises(ValueError, match=r"save\(\): unsupported quantizer Foreign"):
        quantizer_state(Foreign())
    with pytest.raises(ValueError, match=r"save\(\): unsupported quantizer TwoLevelLVQQuantizer"):
        quantizer_state(TwoLevelLVQQuantizer(4, 4))
    with pytest.raises(ValueError, match=r"load\(\): unknown quantizer type 'leanvec'"):
        quantizer_from_state(dict(qtype=np.array("leanvec")))
