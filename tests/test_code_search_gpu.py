"""GPU: the code-domain flat searches (mivq_sq_flat_search / mivq_rabitq_flat_search) against
the decode path they replace.

Unless a test says otherwise, the expected value is what ``_native.sq_decode`` /
``_native.rabitq_decode`` followed by ``_native.flat_search`` return on the same tensors, and
"equal" means ``torch.equal`` on the ids and on the bit patterns of the fp32 distances.
"""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

L2, IP = 1, 0  # mivq metric codes (include/mivq.h)
FORMATS = ("sq4", "sq8", "sq16", "rbq")


# ------------------------------------------------------------------------------ data
class Db:
    """A database of random codes of one format with its parameters, on the device."""

    def __init__(self, dev, fmt, n, d, seed=0, centroid=False, misalign=False):
        g = np.random.default_rng([seed, n, d, FORMATS.index(fmt)])
        self.fmt, self.n, self.d = fmt, n, d
        self.lo = self.den = self.centroid = None
        if fmt == "rbq":
            nb = (d + 7) // 8
            bits = g.integers(0, 256, (n, nb), dtype=np.uint8)
            tail = np.stack([np.ones(n), g.uniform(0.5, 2.0, n)], axis=1).astype(np.float32)
            codes = np.concatenate([bits, tail.view(np.uint8).reshape(n, 8)], axis=1)
            if centroid:
                self.centroid = torch.from_numpy(g.standard_normal(d).astype(np.float32)).to(dev)
        else:
            self.nbits = int(fmt[2:])
            if self.nbits == 16:
                codes = g.integers(0, 65536, (n, d), dtype=np.uint16).view(np.int16)
            elif self.nbits == 8:
                codes = g.integers(0, 256, (n, d), dtype=np.uint8)
            else:
                codes = g.integers(0, 256, (n, (d + 1) // 2), dtype=np.uint8)
                if d % 2:
                    codes[:, -1] &= 0xF0  # odd d: the last low nibble is padding
            self.lo = torch.from_numpy(g.standard_normal(d).astype(np.float32)).to(dev)
            self.den = torch.from_numpy((g.random(d) + 0.5).astype(np.float32)).to(dev)
        self.dev = dev
        self.set_codes(codes, misalign)

    def set_codes(self, codes, misalign=False):
        """codes: numpy (n, width).  misalign: the rows start one element into a buffer, so the
        base is odd for the byte formats (2 mod 4 for SQ-16) and no row start is aligned."""
        codes = np.ascontiguousarray(codes)
        self.n = codes.shape[0]
        t = torch.from_numpy(codes)
        if misalign:
            buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=self.dev)
            buf[1:] = t.reshape(-1).to(self.dev)
            self.codes = buf[1:].view(codes.shape)
            assert self.codes.is_contiguous() and self.codes.data_ptr() % 4 != 0
        else:
            self.codes = t.to(self.dev)

    def queries(self, nq, seed=1):
        g = np.random.default_rng([seed, nq, self.d])
        return torch.from_numpy(g.standard_normal((nq, self.d)).astype(np.float32)).to(self.dev)

    def decode(self):
        from haag_vq import _native

        if self.fmt == "rbq":
            return _native.rabitq_decode(self.codes, self.d, self.centroid)
        return _native.sq_decode(self.codes, self.d, self.lo, self.den, self.nbits)

    def expect(self, Q, k, metric, id_offset=0):
        from haag_vq import _native

        return _native.flat_search(Q, self.decode(), k, metric, id_offset=id_offset)

    def search(self, Q, k, metric, id_offset=0):
        from haag_vq import _native

        if self.fmt == "rbq":
            return _native.rabitq_flat_search(Q, self.codes, self.d, self.centroid, k, metric, id_offset=id_offset)
        return _native.sq_flat_search(Q, self.codes, self.d, self.lo, self.den, self.nbits, k, metric,
                                      id_offset=id_offset)


def same(got, want):
    (gd, gi), (wd, wi) = got, want
    assert gi.shape == wi.shape and gd.shape == wd.shape
    assert torch.equal(gi, wi), f"ids differ in {(gi != wi).sum().item()} of {gi.numel()} places"
    bad = gd.view(torch.int32) != wd.view(torch.int32)
    assert not bad.any(), f"distance bits differ in {bad.sum().item()} of {gd.numel()} places"


def check(db, nq, k, metric, id_offset=0):
    Q = db.queries(nq)
    same(db.search(Q, k, metric, id_offset), db.expect(Q, k, metric, id_offset))


# ------------------------------------------------------------------------------ shape grid
# (nq, n, d, k, metric): the streaming scan (nq < 16 or n < 4096) and the tiled path; every
# nq, n, d and k of the grid appears once per format.  d = 1, 7, 37 are read element by element,
# 200 with 4-B loads (SQ-4 / SQ-8; 16-B for SQ-16, elements for RaBitQ), 64 and 3072 with the
# wide loads.
GRID = [
    (1, 1, 1, 1, L2), (3, 63, 7, 10, IP), (15, 1000, 37, 100, L2), (1, 1000, 64, 256, IP), (3, 1000, 200, 10, L2),
    (15, 63, 3072, 10, IP), (2, 1000, 64, 10, L2),  # (nq = 1, 2, 3, 15: 1, 2, 4, 8 queries per scan workgroup)
    (16, 4096, 64, 10, L2), (130, 4100, 37, 100, IP), (16, 9001, 200, 256, L2), (130, 4096, 7, 1, IP),
    (16, 4100, 3072, 10, L2), (130, 9001, 1, 10, IP),
]


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("nq,n,d,k,metric", GRID)
def test_shape_grid(dev, fmt, nq, n, d, k, metric):
    check(Db(dev, fmt, n, d), nq, k, metric)


# wide loads, then 4-B loads, then single elements in one row (and the 4-B loop alone)
@pytest.mark.parametrize("fmt,d", [("sq4", 63), ("sq4", 200), ("sq8", 92), ("sq16", 72), ("rbq", 60), ("rbq", 96),
                                   ("rbq", 127)])
@pytest.mark.parametrize("nq,n", [(3, 1000), (16, 4100)])
@pytest.mark.parametrize("metric", [L2, IP])
def test_load_width_sequences(dev, fmt, d, nq, n, metric):
    check(Db(dev, fmt, n, d, seed=3), nq, 10, metric)


# ------------------------------------------------------------------------------ every level
def _all_levels(dev, fmt):
    if fmt == "sq16":  # 512 x 128: every u16 once
        i, j = np.meshgrid(np.arange(512), np.arange(128), indexing="ij")
        codes = (128 * i + j).astype(np.uint16).view(np.int16)
        d = 128
    elif fmt == "sq8":  # every byte in every column
        i, j = np.meshgrid(np.arange(256), np.arange(64), indexing="ij")
        codes = ((i + j) % 256).astype(np.uint8)
        d = 64
    else:  # every nibble pair in every byte column
        i, j = np.meshgrid(np.arange(256), np.arange(32), indexing="ij")
        codes = ((i + 7 * j) % 256).astype(np.uint8)
        d = 64
    db = Db(dev, fmt, 1, d, seed=5)
    return db, codes


@pytest.mark.parametrize("fmt", ["sq4", "sq8", "sq16"])
@pytest.mark.parametrize("metric", [L2, IP])
def test_every_level(dev, fmt, metric):
    """Codes built directly so that every level 0 .. 2^b - 1 is dequantised (the division by
    2^b - 1 is a reciprocal sequence in the kernels, an IEEE division in the decode kernels).
    256 rows at a time with k = 256, so every row's distance is compared."""
    db, codes = _all_levels(dev, fmt)
    for s in range(0, codes.shape[0], 256):
        db.set_codes(codes[s:s + 256])
        check(db, 3, 256, metric, id_offset=s)
    # the tiled path: the same rows repeated to 4096
    db.set_codes(np.tile(codes, (4096 // codes.shape[0], 1)))
    check(db, 16, 256, metric)


# ------------------------------------------------------------------------------ alignment, centroid
@pytest.mark.parametrize("fmt,d", [("sq4", 64), ("sq4", 37), ("sq8", 64), ("sq8", 200), ("sq16", 64), ("sq16", 37),
                                   ("rbq", 64), ("rbq", 200)])
@pytest.mark.parametrize("nq,n", [(3, 1000), (16, 4100)])
def test_unaligned_base(dev, fmt, d, nq, n):
    db = Db(dev, fmt, n, d, seed=7, misalign=True)
    check(db, nq, 10, L2)
    check(db, nq, 10, IP)


@pytest.mark.parametrize("d", [64, 200, 3072])
@pytest.mark.parametrize("nq,n", [(3, 1000), (16, 4100)])
@pytest.mark.parametrize("centroid", [False, True])
def test_rabitq_centroid(dev, d, nq, n, centroid):
    db = Db(dev, "rbq", n, d, seed=9, centroid=centroid)
    check(db, nq, 10, L2)
    check(db, nq, 10, IP)


# ------------------------------------------------------------------------------ ties, NaN
@pytest.mark.parametrize("fmt", ["sq8", "rbq"])
@pytest.mark.parametrize("nq,n", [(3, 1000), (16, 4100)])
def test_ties_in_id_order(dev, fmt, nq, n):
    db = Db(dev, fmt, n, 64, seed=11)
    trio = [5, 700, n - 1]
    c = db.codes.cpu().numpy().copy()
    c[trio[1]] = c[trio[0]]
    c[trio[2]] = c[trio[0]]
    db.set_codes(c)
    Q = db.queries(nq)
    Q[0] = db.decode()[trio[0]]  # L2 distance 0 to the three rows
    got = db.search(Q, 10, L2)
    same(got, db.expect(Q, 10, L2))
    assert got[1][0, :3].tolist() == trio
    assert got[0][0, :3].tolist() == [0.0, 0.0, 0.0]


@pytest.mark.parametrize("nq,n", [(3, 300), (16, 4100)])
@pytest.mark.parametrize("metric", [L2, IP])
def test_nan_ranks_as_inf(dev, nq, n, metric):
    """A RaBitQ row whose `mult` is NaN decodes to NaN in every dimension; an SQ `lo` entry of
    +inf makes every row's distance +inf / -inf / NaN.  Both rank as on the decode path."""
    db = Db(dev, "rbq", n, 64, seed=13)
    c = db.codes.cpu().numpy().copy()
    c[17, 12:16] = np.array([np.nan], dtype=np.float32).view(np.uint8)
    db.set_codes(c)
    Q = db.queries(nq)
    k = min(n, 256)
    got = db.search(Q, k, metric)
    same(got, db.expect(Q, k, metric))
    if k == n:  # the NaN row is the last of every list, at +inf
        assert (got[1][:, -1] == 17).all() and torch.isinf(got[0][:, -1]).all()
    else:
        assert not (got[1] == 17).any()
    for fmt in ("sq4", "sq8", "sq16"):
        db = Db(dev, fmt, n, 37, seed=13)
        db.lo[3] = float("inf")
        Q = db.queries(nq)
        Q[0, 3] = 0.0  # IP: 0 * inf = NaN
        got = db.search(Q, 10, metric)
        same(got, db.expect(Q, 10, metric))
        assert torch.isinf(got[0][0]).all()


# ------------------------------------------------------------------------------ edges
@pytest.mark.parametrize("fmt", FORMATS)
def test_k_larger_than_n(dev, fmt):
    db = Db(dev, fmt, 5, 37, seed=15)
    Q = db.queries(3)
    got = db.search(Q, 10, L2)
    same(got, db.expect(Q, 10, L2))
    assert torch.isinf(got[0][:, 5:]).all() and (got[0][:, 5:] > 0).all()
    assert (got[1][:, 5:] == -1).all()  # 0xFFFFFFFF
    assert sorted(got[1][0, :5].tolist()) == [0, 1, 2, 3, 4]


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("nq,n", [(3, 1000), (16, 4100)])
def test_id_offset_at_the_top(dev, fmt, nq, n):
    from haag_vq import _native

    db = Db(dev, fmt, n, 64, seed=17)
    off = 2 ** 32 - 1 - n
    Q = db.queries(nq)
    got = db.search(Q, 10, L2, id_offset=off)
    same(got, db.expect(Q, 10, L2, id_offset=off))
    base = db.search(Q, 10, L2)
    ids = got[1].to(torch.int64) & 0xFFFFFFFF
    assert torch.equal(ids, base[1].to(torch.int64) + off) and int(ids.max()) <= 2 ** 32 - 2
    with pytest.raises(ValueError, match="ids overflow"):
        db.search(Q, 10, L2, id_offset=off + 1)
    assert _native.NO_ID == 0xFFFFFFFF


@pytest.mark.parametrize("fmt", FORMATS)
def test_empty_database_and_no_queries(dev, fmt):
    db = Db(dev, fmt, 4, 37, seed=19)
    Q = db.queries(3)
    full = db.codes
    db.codes = full[:0].contiguous()
    d, i = db.search(Q, 4, L2)
    assert d.shape == (3, 4) and torch.isinf(d).all() and (d > 0).all() and (i == -1).all()
    db.codes = full
    d, i = db.search(Q[:0].contiguous(), 4, IP)
    assert d.shape == (0, 4) and i.shape == (0, 4)


# ------------------------------------------------------------------------------ public path
def _data(n, d, nq, seed=21):
    g = np.random.default_rng(seed)
    return g.standard_normal((n, d)).astype(np.float32), g.standard_normal((nq, d)).astype(np.float32)


def _decode_path(model, codes, Q, k, metric):
    """What search_codes computed before the code-domain kernels: decompress + flat_search."""
    from haag_vq import _arrays, _native

    xh = _arrays.to_device(model.decompress(codes), torch.float32)
    d, i = _native.flat_search(_arrays.to_device(Q), xh, k, L2 if metric == "l2" else IP)
    return (d if metric == "l2" else -d).cpu().numpy(), i.cpu().numpy().view(np.uint32)


def _no_decode(monkeypatch):
    from haag_vq import _native

    def boom(*a, **kw):
        raise AssertionError("the database was decoded")

    monkeypatch.setattr(_native, "sq_decode", boom)
    monkeypatch.setattr(_native, "rabitq_decode", boom)


@pytest.mark.parametrize("kind", ["sq4", "sq8", "sq16", "rabitq"])
@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("nq,n", [(5, 600), (20, 4100)])
def test_index_searches_without_decoding(dev, monkeypatch, kind, metric, nq, n):
    from haag_vq.methods.rabit_quantization import RaBitQuantizer
    from haag_vq.methods.scalar_quantization import ScalarQuantizer
    from haag_vq.methods.search.flat_quantized_index import FlatQuantizedIndex

    X, Q = _data(n, 37, nq)
    make = (lambda: RaBitQuantizer()) if kind == "rabitq" else (lambda: ScalarQuantizer(int(kind[2:])))
    ref = make()
    Xd = torch.from_numpy(X).to(dev)
    ref.fit(Xd)
    want_d, want_i = _decode_path(ref, ref.compress(Xd), Q, 10, metric)
    _no_decode(monkeypatch)
    idx = FlatQuantizedIndex(make())
    idx.fit(X, metric=metric)
    ids, dists = idx.search_with_scores(Q, 10)
    np.testing.assert_array_equal(ids, want_i)
    np.testing.assert_array_equal(dists.view(np.uint32), want_d.view(np.uint32))


def test_f64_fitted_sq_still_decodes(dev, monkeypatch):
    from haag_vq.methods.scalar_quantization import ScalarQuantizer
    from haag_vq.methods.search.flat_quantized_index import search_codes

    X, Q = _data(300, 20, 4)
    sq = ScalarQuantizer(8)
    sq.fit(X.astype(np.float64))
    assert np.asarray(sq.min).dtype == np.float64
    codes = sq.compress(torch.from_numpy(X).to(dev))
    d, i = search_codes(sq, codes, Q, 5)  # works, through the f64 decode
    assert d.shape == (4, 5)
    _no_decode(monkeypatch)
    with pytest.raises(AssertionError, match="the database was decoded"):
        search_codes(sq, codes, Q, 5)


def test_code_dtypes_callers_pass(dev):
    """SQ-16 codes as the int16 device tensor compress() returns, as a uint16 device tensor and
    as a numpy uint16 array; SQ-8 / RaBitQ as numpy uint8."""
    from haag_vq.methods.rabit_quantization import RaBitQuantizer
    from haag_vq.methods.scalar_quantization import ScalarQuantizer
    from haag_vq.methods.search.flat_quantized_index import search_codes

    X, Q = _data(500, 24, 6)
    Xd = torch.from_numpy(X).to(dev)
    sq = ScalarQuantizer(16)
    sq.fit(Xd)
    c = sq.compress(Xd)
    assert c.dtype == torch.int16
    want = search_codes(sq, c, Q, 7, "ip", id_offset=100)
    for alt in (c.view(torch.uint16), c.cpu().numpy().view(np.uint16)):
        same(search_codes(sq, alt, Q, 7, "ip", id_offset=100), want)
    wd, wi = _decode_path(sq, c, Q, 7, "ip")
    np.testing.assert_array_equal(want[0].cpu().numpy().view(np.uint32), wd.view(np.uint32))
    np.testing.assert_array_equal(want[1].cpu().numpy().view(np.uint32) - 100, wi)
    for model in (ScalarQuantizer(8), RaBitQuantizer()):
        model.fit(Xd)
        c = model.compress(Xd)
        same(search_codes(model, c.cpu().numpy(), Q, 7), search_codes(model, c, Q, 7))


# ------------------------------------------------------------------------------ memory
@pytest.mark.parametrize("nq", [4, 32])
def test_search_codes_allocates_no_decoded_copy(dev, nq):
    """SQ-8, 65536 x 256: the peak rise across search_codes stays below n * d bytes, a quarter of
    the fp32 copy the decode path allocated (4 n d)."""
    from haag_vq.methods.scalar_quantization import ScalarQuantizer
    from haag_vq.methods.search.flat_quantized_index import search_codes

    n, d = 65536, 256
    g = torch.Generator(device=dev).manual_seed(23)
    X = torch.randn((n, d), generator=g, device=dev)
    Q = torch.randn((nq, d), generator=g, device=dev)
    sq = ScalarQuantizer(8)
    sq.fit(X)
    codes = sq.compress(X)
    del X
    search_codes(sq, codes, Q, 10)  # parameters cached, library loaded
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    dd, ii = search_codes(sq, codes, Q, 10)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print(f"nq={nq}: peak rise {rise} B, n*d = {n * d} B")
    assert rise < n * d
    assert ii.shape == (nq, 10)


def test_workspace_far_below_the_database():
    from haag_vq import _native

    lib = _native.load_library()
    for fn in (lib.mivq_sq_flat_search_workspace_bytes, lib.mivq_rabitq_flat_search_workspace_bytes):
        assert 0 < fn(1000, 1_000_000, 3072, 10) < 1_000_000 * 3072
        assert 0 < fn(4, 65536, 256, 10) < 1 << 20
