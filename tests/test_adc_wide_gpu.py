"""GPU: mivq_adc_search on product quantizers whose lookup tables do not fit one workgroup's LDS
(the subspace-chunked scan of adc_wide.hip), bit for bit against the header's rule in numpy float32."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NO_ID = 0xFFFFFFFF


def rule(lut, codes, k, id_offset=0):
    """dist = ((lut[q][0][c_0] + lut[q][1][c_1]) + ...) in float32, NaN as +inf, the k smallest
    (dist, id) ascending, missing slots (+inf, 0xFFFFFFFF)."""
    nq, M, _ = lut.shape
    n = codes.shape[0]
    S = lut[:, 0, codes[:, 0]]
    for m in range(1, M):
        S = S + lut[:, m, codes[:, m]]
    assert S.dtype == np.float32
    S[np.isnan(S)] = np.inf
    ids = np.arange(n, dtype=np.int64) + id_offset
    D = np.full((nq, k), np.inf, np.float32)
    I = np.full((nq, k), NO_ID, np.uint32)
    for q in range(nq):
        o = np.lexsort((ids, S[q]))[:k]
        D[q, :len(o)], I[q, :len(o)] = S[q, o], ids[o]
    return D, I


def shifted(a, dev, elems):
    """A contiguous device copy of `a` whose base lies `elems` elements past a 16-byte boundary."""
    buf = torch.empty(a.size + 16, dtype=torch.from_numpy(a).dtype, device=dev)
    assert buf.data_ptr() % 16 == 0
    v = buf[elems:elems + a.size].view(a.shape)
    v.copy_(torch.from_numpy(a))
    return v


# (M, nbits, n, nq, k): every (M, nbits), n, nq and k of the issue's table; the last case makes one
# workgroup walk several 2048-row tiles (86 query blocks leave two row ranges for three tiles)
CASES = [
    (161, 8, 4097, 9, 10), (192, 8, 4097, 17, 10), (192, 8, 1, 1, 1), (192, 8, 63, 9, 256),
    (200, 8, 4097, 1, 256), (200, 8, 63, 17, 1), (256, 8, 4097, 9, 1), (256, 8, 63, 1, 10),
    (768, 6, 4097, 17, 10), (768, 6, 1, 9, 256), (2600, 4, 4097, 1, 10), (2600, 4, 63, 17, 1),
    (161, 8, 4097, 681, 10),
]


@pytest.mark.parametrize("case", range(len(CASES)), ids=["M%d-b%d-n%d-nq%d-k%d" % c for c in CASES])
def test_wide_scan_equals_the_rule(dev, case):
    from haag_vq import _native

    M, nbits, n, nq, k = CASES[case]
    rng = np.random.default_rng(100 + case)
    ksub = 1 << nbits
    lut = (rng.standard_normal((nq, M, ksub), dtype=np.float32) ** 2).astype(np.float32)
    codes = rng.integers(0, ksub, (n, M), dtype=np.uint8)
    if n > 5:
        # a tie: id 5 before id n - 1; certain to be in the output where k >= n (the n = 63, k = 256 case)
        codes[n - 1] = codes[5]
        for j, v in enumerate((np.inf, np.inf, np.nan)):  # on codes that occur: rows 1, 2 and 3
            lut[j % nq, 7 * j, codes[1 + j, 7 * j]] = v
    # odd cases: both bases one element (codes 1 B, LUT 4 B) past a 16-byte boundary, ids from 2^31
    off = case % 2
    id_offset = 2 ** 31 if off else 0
    cd, ld = shifted(codes, dev, off), shifted(lut, dev, off)
    assert cd.data_ptr() % 16 == off and ld.data_ptr() % 16 == 4 * off
    d, i = _native.adc_search(ld, cd, k, nbits, id_offset=id_offset)
    d2, i2 = _native.adc_search(ld, cd, k, nbits, id_offset=id_offset, flags=_native.ADC_FORCE_EXACT)
    torch.cuda.synchronize()
    D, I = rule(lut, codes, k, id_offset)
    got_d, got_i = d.cpu().numpy(), i.cpu().numpy().view(np.uint32)
    np.testing.assert_array_equal(got_i, I)
    np.testing.assert_array_equal(got_d.view(np.uint32), D.view(np.uint32))
    assert torch.equal(d, d2) and torch.equal(i, i2)


def test_flat_index_over_pq192(dev):
    """FlatQuantizedIndex(ProductQuantizer(M=192, B=8)) searches, and returns the rule applied to
    mivq_adc_lut's tables and the index's own codes."""
    from haag_vq import _native
    from haag_vq.methods.product_quantization import ProductQuantizer
    from haag_vq.methods.search.flat_quantized_index import FlatQuantizedIndex

    rng = np.random.default_rng(7)
    X = rng.standard_normal((3000, 384), dtype=np.float32)
    Q = rng.standard_normal((20, 384), dtype=np.float32)
    pq = ProductQuantizer(M=192, B=8)
    pq.niter = 2
    index = FlatQuantizedIndex(pq)
    index.fit(X)
    ids, dists = index.search_with_scores(Q, 10)
    lut = _native.adc_lut(torch.from_numpy(Q).to(dev), pq.centroids_device, 8)
    D, I = rule(lut.cpu().numpy(), index._codes.cpu().numpy(), 10)
    np.testing.assert_array_equal(np.asarray(ids).astype(np.int64), I.astype(np.int64))
    np.testing.assert_array_equal(np.asarray(dists, dtype=np.float32).view(np.uint32), D.view(np.uint32))
