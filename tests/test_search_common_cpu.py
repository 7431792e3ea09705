"""CPU: what the search indexes share on the host (methods/search/_common.py) and the array form
of the inverted lists (_ivf.IvfLists), on hand-made inputs of a few rows (no GPU)."""

import numpy as np
import pytest
import torch

from haag_vq import _native
from haag_vq.methods._ivf import IvfLists
from haag_vq.methods.search import _common as C

NO_ID = np.uint32(0xFFFFFFFF)
FLT_MAX = np.finfo(np.float32).max


def _raw(dists, ids):
    """A kernel's (dists f32, ids int32 holding uint32 ids) as CPU tensors."""
    return (torch.tensor(dists, dtype=torch.float32),
            torch.from_numpy(np.array(ids, dtype=np.uint32).view(np.int32)))


def test_constants():
    assert C.MAX_K == 256 and C.MAX_CANDIDATES == 256 and C.DECODE_BYTES == 1 << 28
    assert C.FLT_MAX == FLT_MAX
    assert C.METRIC == {"l2": _native.METRIC_L2, "ip": _native.METRIC_INNER_PRODUCT}
    from haag_vq.methods.search import flat_quantized_index, refined_index

    assert refined_index.MAX_CANDIDATES == 256 and flat_quantized_index.MAX_KERNEL_K == 256


def test_check_metric():
    assert C.check_metric("l2") == _native.METRIC_L2 and C.check_metric("ip") == _native.METRIC_INNER_PRODUCT
    for bad in ("cosine", "L2", None, 1):
        with pytest.raises(ValueError, match=r"metric must be 'l2' or 'ip', got "):
            C.check_metric(bad)


def test_results_to_host_l2_sentinel():
    d, i = _raw([[0.5, 2.0, np.inf], [1.0, np.inf, np.inf]], [[7, 3, 0xFFFFFFFF], [0, 0xFFFFFFFF, 0xFFFFFFFF]])
    ids, dists = C.results_to_host(d, i, negate=False, sentinel=FLT_MAX)
    assert ids.dtype == np.uint32 and dists.dtype == np.float32 and ids.shape == dists.shape == (2, 3)
    assert np.array_equal(ids, np.array([[7, 3, NO_ID], [0, NO_ID, NO_ID]], dtype=np.uint32))
    assert np.array_equal(dists, np.array([[0.5, 2.0, FLT_MAX], [1.0, FLT_MAX, FLT_MAX]], dtype=np.float32))


def test_results_to_host_ip_negated():
    # kernel keys of 'ip' are negated inner products, ascending; unfilled slots +inf
    d, i = _raw([[-3.0, -1.5, np.inf]], [[4, 9, 0xFFFFFFFF]])
    ids, dists = C.results_to_host(d, i, negate=True, sentinel=-FLT_MAX)
    assert np.array_equal(ids, np.array([[4, 9, NO_ID]], dtype=np.uint32))
    assert np.array_equal(dists, np.array([[3.0, 1.5, -FLT_MAX]], dtype=np.float32)) and dists.dtype == np.float32


def test_results_to_host_no_sentinel_keeps_inf():
    d, i = _raw([[1.0, np.inf]], [[2, 0xFFFFFFFF]])
    ids, dists = C.results_to_host(d, i, negate=False, sentinel=None)
    assert ids[0, 1] == NO_ID and dists[0, 0] == 1.0 and np.isposinf(dists[0, 1])
    ids, dists = C.results_to_host(*_raw([[1.0, np.inf]], [[2, 0xFFFFFFFF]]))  # the defaults
    assert ids[0, 1] == NO_ID and dists[0, 0] == 1.0 and np.isposinf(dists[0, 1])


def test_results_to_host_large_ids_are_uint32():
    big = [2 ** 31, 2 ** 31 + 5, 2 ** 32 - 2]
    ids, dists = C.results_to_host(*_raw([[0.0, 1.0, 2.0]], [big]), negate=False, sentinel=FLT_MAX)
    assert ids.dtype == np.uint32 and ids.tolist() == [big]
    assert dists.tolist() == [[0.0, 1.0, 2.0]]  # none of them is the NO_ID sentinel


@pytest.mark.parametrize("nq,k,shape", [(3, 0, (3, 0)), (0, 5, (0, 5)), (0, 0, (0, 0)), (2, -1, (2, 0)), (4, 7, (4, 7))])
def test_empty_results(nq, k, shape):
    ids, dists = C.empty_results(nq, k)
    assert ids.shape == dists.shape == shape and ids.dtype == np.uint32 and dists.dtype == np.float32


def test_candidate_count():
    assert C.candidate_count(10, 10, 1000) == 100
    assert C.candidate_count(10, 10, 37) == 37      # clamped to N
    assert C.candidate_count(10, 10, 0) == 0        # an empty database
    assert C.candidate_count(7, 1, 1000) == 7       # factor 1
    assert C.candidate_count(256, 1, 1000) == 256 and C.candidate_count(32, 8, 1000) == 256
    with pytest.raises(ValueError, match=r"k \* refine_factor = 26 \* 10 = 260: the base searches keep at most 256 results"):
        C.candidate_count(26, 10, 1000)
    with pytest.raises(ValueError, match="at most 256 results"):
        C.candidate_count(257, 1, 3)                # checked before the clamp


def test_save_npz_creates_parent(tmp_path):
    path = tmp_path / "a" / "b" / "index.npz"
    C.save_npz(path, x=np.arange(3, dtype=np.int64), name=np.array("sq"))
    with np.load(path, allow_pickle=False) as z:
        assert sorted(z.files) == ["name", "x"] and z["x"].tolist() == [0, 1, 2] and str(z["name"]) == "sq"


def test_sampled_mse_drops_ids_out_of_range():
    X = np.arange(12, dtype=np.float32).reshape(4, 3)
    seen = []

    def reconstruct(rows):
        seen.append(rows.tolist())
        return torch.from_numpy(X[rows.numpy()] + 1.0)

    assert C.sampled_mse(reconstruct, X, 4, 3, None) == 1.0 and seen == [[0, 1, 2, 3]]
    assert C.sampled_mse(reconstruct, X, 4, 3, np.array([-1, 2, 9, 0])) == 1.0 and seen[-1] == [2, 0]
    assert C.sampled_mse(reconstruct, X, 4, 3, np.array([4, -3])) is None


def _lists(codes, tau):
    return IvfLists(offsets=torch.tensor([0, 2, 2, 5], dtype=torch.int64), codes=codes,
                    ids=torch.from_numpy(np.array([3, 0, 4, 2 ** 32 - 7, 1], dtype=np.uint32).view(np.int32)), tau=tau)


@pytest.mark.parametrize("kind", ["u8", "u8_tau", "i16"])
def test_ivf_lists_arrays_round_trip(kind, tmp_path):
    if kind == "i16":
        codes = torch.tensor([[-1, 300], [7, -32768], [0, 1], [2, 3], [32767, 5]], dtype=torch.int16)
    else:
        codes = torch.arange(15, dtype=torch.uint8).reshape(5, 3)
    tau = torch.tensor([0.5, -1.0, 2.0, 3.5, 0.0]) if kind == "u8_tau" else None
    L = _lists(codes, tau)
    arrays = L.to_arrays()
    assert sorted(arrays) == sorted(["offsets", "codes", "ids"] + (["tau"] if tau is not None else []))
    assert arrays["offsets"].dtype == np.int64 and arrays["ids"].dtype == np.int32
    assert arrays["codes"].dtype == (np.int16 if kind == "i16" else np.uint8)
    C.save_npz(tmp_path / "lists.npz", **arrays)  # through a file, as the indexes do
    with np.load(tmp_path / "lists.npz", allow_pickle=False) as z:
        back = IvfLists.from_arrays(z, torch.device("cpu"))
    for name in ("offsets", "codes", "ids"):
        a, b = getattr(L, name), getattr(back, name)
        assert a.dtype == b.dtype and torch.equal(a, b), name
    if tau is None:
        assert back.tau is None
    else:
        assert back.tau.dtype == torch.float32 and torch.equal(back.tau, tau)
    assert IvfLists.from_arrays(arrays, torch.device("cpu")).codes.dtype == codes.dtype  # a plain dict too
