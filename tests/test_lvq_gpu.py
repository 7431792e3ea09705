"""GPU: LVQ encode / decode / fit and the code-domain search on the device.

Encode, decode and fit are held to tests/golden/lvq_golden.npz (the reference's LVQQuantizer, see
tests/test_lvq_cpu.py) bit for bit.  The code-domain search (mivq_lvq_flat_search) is held to
``_native.lvq_decode`` + ``_native.flat_search`` on the same tensors: ``torch.equal`` on the ids
and on the bit patterns of the fp32 distances, as tests/test_code_search_gpu.py does for its
formats.  End to end, FlatQuantizedIndex(LVQQuantizer(B)) passes the rule of
tests/_search_rule.py against the fixture.
"""

import numpy as np
import pytest
import torch

import _lvq_rule as LR

pytestmark = pytest.mark.gpu

L2, IP = 1, 0  # mivq metric codes (include/mivq.h)
BITS = tuple(range(1, 9))


@pytest.fixture(scope="module")
def lg(golden_dir):
    return LR.load_fixture(golden_dir)


_made = {}


@pytest.fixture(scope="module")
def cases(lg):
    def get(name) -> LR.Case:
        if name not in _made:
            _made[name] = LR.Case(name, lg)
        return _made[name]

    return get


def _quantizer(cs, dev):
    from haag_vq.methods.lvq_quantization import LVQQuantizer

    q = LVQQuantizer(cs.B)
    q.mu = cs.mu.copy()
    return q


# ------------------------------------------------------------------------------ encode
@pytest.mark.parametrize("name", list(LR.CASES))
def test_compress_equals_the_reference(dev, cases, name):
    """Byte for byte, from a device tensor and from a numpy array; padding bits zero."""
    cs = cases(name)
    q = _quantizer(cs, dev)
    codes = q.compress(torch.from_numpy(cs.X).to(dev))
    assert isinstance(codes, torch.Tensor) and codes.dtype == torch.uint8
    got = codes.cpu().numpy()
    cs.codes_match(got)
    np.testing.assert_array_equal(got, cs.codes)  # where they differ, not only that they do
    assert not LR.padding_bits(got, cs.D, cs.B).any()
    host = q.compress(cs.X)
    assert isinstance(host, np.ndarray)
    np.testing.assert_array_equal(host, got)


@pytest.mark.parametrize("name", ["b3_d37", "b7_d33", "b8_d128", "b4_d100", "b2_d61", "beyond_b3_d5000"])
def test_encode_writes_only_its_rows(dev, cases, name):
    """Rows [2, 2 + n) of an over-allocated buffer: the rows before and after keep their fill.
    Odd code sizes put the window at every byte alignment; an x that is not 16-B aligned takes
    the scalar loads."""
    from haag_vq import _native

    cs = cases(name)
    n, size = cs.N, LR.code_size(cs.D, cs.B)
    mu = torch.from_numpy(cs.mu).to(dev)
    buf = torch.full((n + 5, size), 0xA5, dtype=torch.uint8, device=dev)
    _native.lvq_encode(torch.from_numpy(cs.X).to(dev), mu, cs.B, out=buf[2:2 + n])
    got = buf.cpu().numpy()
    np.testing.assert_array_equal(got[2:2 + n], cs.codes)
    assert (got[:2] == 0xA5).all() and (got[2 + n:] == 0xA5).all()
    xb = torch.empty(n * cs.D + 1, dtype=torch.float32, device=dev)
    xb[1:] = torch.from_numpy(cs.X).to(dev).reshape(-1)
    x1 = xb[1:].view(n, cs.D)
    assert x1.data_ptr() % 16 != 0
    np.testing.assert_array_equal(_native.lvq_encode(x1, mu, cs.B).cpu().numpy(), cs.codes)


@pytest.mark.parametrize("B,lead,want", LR.ROUNDING)
def test_planted_ties_round_half_to_even(dev, lg, B, lead, want):
    from haag_vq.methods.lvq_quantization import LVQQuantizer

    D = lg[f"round_b{B}_rec"].shape[1]
    row, _ = LR.rounding_row(B, D)
    q = LVQQuantizer(B)
    q.mu = np.zeros(D, np.float32)
    codes = q.compress(row[None, :])
    idx, _, _ = LR.unpack(codes, D, B)
    assert list(idx[0, :len(want)]) == want
    np.testing.assert_array_equal(codes, lg[f"round_b{B}_codes"])
    np.testing.assert_array_equal(q.decompress(codes).view(np.uint32), lg[f"round_b{B}_rec"].view(np.uint32))


def test_nan_row_stays_inside_its_row(dev):
    """What a NaN row encodes to is unspecified; its neighbours and the buffer around it are not."""
    from haag_vq import _native

    rng = np.random.default_rng(31)
    X = rng.standard_normal((6, 37)).astype(np.float32)
    mu = X.mean(axis=0)
    want = LR.encode(X, mu, 5)
    X[3, 11] = np.nan
    buf = torch.full((8, want.shape[1]), 0x5A, dtype=torch.uint8, device=dev)
    _native.lvq_encode(torch.from_numpy(X).to(dev), torch.from_numpy(mu).to(dev), 5, out=buf[1:7])
    got = buf.cpu().numpy()
    keep = [0, 1, 2, 4, 5]
    np.testing.assert_array_equal(got[1:7][keep], want[keep])
    assert (got[0] == 0x5A).all() and (got[7] == 0x5A).all()


# ------------------------------------------------------------------------------ decode
@pytest.mark.parametrize("name", list(LR.CASES))
def test_decompress_equals_the_reference(dev, cases, name):
    cs = cases(name)
    q = _quantizer(cs, dev)
    cd = torch.from_numpy(cs.codes).to(dev)
    rec = q.decompress(cd)
    assert isinstance(rec, torch.Tensor) and rec.dtype == torch.float32
    got = rec.cpu().numpy()
    cs.rec_match(got)
    np.testing.assert_array_equal(got.view(np.uint32), cs.rec.view(np.uint32))
    host = q.decompress(cs.codes)
    assert isinstance(host, np.ndarray) and host.dtype == np.float32
    np.testing.assert_array_equal(host.view(np.uint32), got.view(np.uint32))
    # row-independent: decompress(codes[ids]) == decompress(codes)[ids]
    ids = torch.from_numpy(np.random.default_rng(5).permutation(cs.N)[:min(cs.N, 50)]).to(dev)
    part = q.decompress(cd[ids].contiguous())
    assert torch.equal(part.view(torch.int32), rec[ids].view(torch.int32))


# ------------------------------------------------------------------------------ fit
@pytest.mark.parametrize("name", list(LR.CASES))
def test_fit_equals_the_reference(dev, cases, name):
    from haag_vq.methods.lvq_quantization import LVQQuantizer

    cs = cases(name)
    q = LVQQuantizer(cs.B)
    q.fit(cs.X)
    assert isinstance(q.mu, np.ndarray) and q.mu.dtype == np.float32 and q.mu.shape == (cs.D,)
    np.testing.assert_array_equal(q.mu.view(np.uint32), cs.mu.view(np.uint32))
    q.fit(torch.from_numpy(cs.X).to(dev))
    np.testing.assert_array_equal(q.mu.view(np.uint32), cs.mu.view(np.uint32))


@pytest.mark.parametrize("n,d", [(70000, 16), (1000, 37), (257, 1), (4097, 130)])
def test_column_mean_is_the_sequential_sum(dev, n, d):
    """Many rows per column; d that is no multiple of 4 or of the 16 columns of a workgroup; a
    row count one past the 256-row tile.  Equal to the sequential restatement, which for
    d >= 2 is numpy's own mean (tests/test_lvq_cpu.py)."""
    from haag_vq import _native

    rng = np.random.default_rng([n, d])
    X = (rng.standard_normal((n, d)) * 3.0 + rng.standard_normal(d)).astype(np.float32)
    want = LR.seq_mean(X)
    if d >= 2:
        np.testing.assert_array_equal(want.view(np.uint32), X.mean(axis=0).view(np.uint32))
    got = _native.column_mean(torch.from_numpy(X).to(dev)).cpu().numpy()
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))


# ------------------------------------------------------------------------------ code-domain search
class Db:
    """Random LVQ codes with random finite lo and positive delta per row, on the device."""

    def __init__(self, dev, B, n, d, seed=0, misalign=False):
        g = np.random.default_rng([seed, n, d, B])
        self.B, self.n, self.d, self.dev = B, n, d, dev
        ib = (d * B + 7) // 8
        bits = g.integers(0, 256, (n, ib), dtype=np.uint8)
        spare = ib * 8 - d * B
        bits[:, -1] &= np.uint8((0xFF << spare) & 0xFF)  # padding bits are 0
        tail = np.stack([g.standard_normal(n), g.uniform(0.5, 2.0, n) / ((1 << B) - 1)], axis=1).astype(np.float32)
        self.mu = torch.from_numpy(g.standard_normal(d).astype(np.float32)).to(dev)
        self.set_codes(np.concatenate([bits, tail.view(np.uint8).reshape(n, 8)], axis=1), misalign)

    def set_codes(self, codes, misalign=False):
        """misalign: the rows start one byte into a buffer, so no row start is 4-byte aligned
        unless the code size is odd too -- then some are, which the kernel must not assume."""
        codes = np.ascontiguousarray(codes)
        self.n = codes.shape[0]
        t = torch.from_numpy(codes)
        if misalign:
            buf = torch.empty(t.numel() + 1, dtype=torch.uint8, device=self.dev)
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

        return _native.lvq_decode(self.codes, self.mu, self.B)

    def expect(self, Q, k, metric, id_offset=0):
        from haag_vq import _native

        return _native.flat_search(Q, self.decode(), k, metric, id_offset=id_offset)

    def search(self, Q, k, metric, id_offset=0):
        from haag_vq import _native

        return _native.lvq_flat_search(Q, self.codes, self.mu, self.B, k, metric, id_offset=id_offset)


def same(got, want):
    (gd, gi), (wd, wi) = got, want
    assert gi.shape == wi.shape and gd.shape == wd.shape
    assert torch.equal(gi, wi), f"ids differ in {(gi != wi).sum().item()} of {gi.numel()} places"
    bad = gd.view(torch.int32) != wd.view(torch.int32)
    assert not bad.any(), f"distance bits differ in {bad.sum().item()} of {gd.numel()} places"


def check(db, nq, k, metric, id_offset=0):
    Q = db.queries(nq)
    same(db.search(Q, k, metric, id_offset), db.expect(Q, k, metric, id_offset))


def test_db_decode_is_the_restatement(dev):
    """The expectation's first half on random codes: lvq_decode equals the numpy restatement."""
    for B in BITS:
        db = Db(dev, B, 40, 77, seed=2)
        want = LR.decode(db.codes.cpu().numpy(), db.mu.cpu().numpy(), B)
        np.testing.assert_array_equal(db.decode().cpu().numpy().view(np.uint32), want.view(np.uint32))


# (nq, n, d, k, metric): the streaming scan (nq < 16 or n < 4096) and the tiled path.  d = 1, 7
# have no whole 32-dimension unit, 37 and 200 a unit loop and a tail, 64 and 3072 units only;
# whether a unit is read with 8-B, 4-B loads or byte-wise follows from B and the code size.
GRID = [
    (1, 1, 1, 1, L2), (3, 63, 7, 10, IP), (15, 1000, 37, 100, L2), (1, 1000, 64, 256, IP), (3, 1000, 200, 10, L2),
    (15, 63, 3072, 10, IP),
    (16, 4096, 64, 10, L2), (130, 4100, 37, 100, IP), (16, 9001, 200, 256, L2), (16, 4100, 3072, 10, L2),
]


@pytest.mark.parametrize("B", BITS)
@pytest.mark.parametrize("nq,n,d,k,metric", GRID)
def test_shape_grid(dev, B, nq, n, d, k, metric):
    check(Db(dev, B, n, d), nq, k, metric)


# code_size % 8, % 4 and the rest: d = 64 gives 8 B + 8 (8-B rows for every B), d = 32 gives
# 4 B + 8 (4-B rows for odd B), d = 96 a 4-B row for odd B with three units, d = 40 and 100 rows
# of every residue (byte-wise whenever code_size % 4 != 0)
@pytest.mark.parametrize("B", BITS)
@pytest.mark.parametrize("d", [32, 40, 64, 96, 100])
@pytest.mark.parametrize("nq,n", [(3, 1000), (16, 4100)])
def test_row_alignments(dev, B, d, nq, n):
    db = Db(dev, B, n, d, seed=3)
    check(db, nq, 10, L2)
    check(db, nq, 10, IP)


@pytest.mark.parametrize("B", BITS)
@pytest.mark.parametrize("d", [64, 37])
@pytest.mark.parametrize("nq,n", [(3, 1000), (16, 4100)])
def test_unaligned_base(dev, B, d, nq, n):
    db = Db(dev, B, n, d, seed=7, misalign=True)
    check(db, nq, 10, L2)
    check(db, nq, 10, IP)


def test_code_size_not_a_multiple_of_four(dev):
    for B, d in [(3, 37), (7, 33), (1, 200), (5, 61), (8, 3)]:
        assert LR.code_size(d, B) % 4 != 0
        for nq, n in [(3, 1000), (16, 4100)]:
            check(Db(dev, B, n, d, seed=9), nq, 10, L2)


@pytest.mark.parametrize("B", BITS)
@pytest.mark.parametrize("metric", [L2, IP])
def test_every_level(dev, B, metric):
    """Every index 0 .. 2^B - 1 at every position of a 32-dimension unit: row r holds
    (r + t) mod 2^B in dimension t.  256 rows with k = 256, so every row is compared; then the
    same rows repeated to 4096 for the tiled path."""
    d = 64
    r, t = np.meshgrid(np.arange(256), np.arange(d), indexing="ij")
    idx = ((r + t) % (1 << B)).astype(np.int32)
    g = np.random.default_rng(5)
    lo = g.standard_normal(256).astype(np.float32)
    delta = (g.uniform(0.5, 2.0, 256) / ((1 << B) - 1)).astype(np.float32)
    codes = LR.pack(idx, lo, delta, B)
    db = Db(dev, B, 1, d, seed=5)
    db.set_codes(codes)
    check(db, 3, 256, metric)
    db.set_codes(np.tile(codes, (16, 1)))
    check(db, 16, 256, metric)


@pytest.mark.parametrize("B", [1, 3, 8])
@pytest.mark.parametrize("nq,n", [(3, 1000), (16, 4100)])
def test_ties_in_id_order(dev, B, nq, n):
    db = Db(dev, B, n, 64, seed=11)
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
    """A row whose delta is NaN decodes to NaN in every dimension and ranks as +inf."""
    db = Db(dev, 5, n, 64, seed=13)
    c = db.codes.cpu().numpy().copy()
    c[17, -4:] = np.array([np.nan], dtype=np.float32).view(np.uint8)
    db.set_codes(c)
    Q = db.queries(nq)
    k = min(n, 256)
    got = db.search(Q, k, metric)
    same(got, db.expect(Q, k, metric))
    if k == n:
        assert (got[1][:, -1] == 17).all() and torch.isinf(got[0][:, -1]).all()
    else:
        assert not (got[1] == 17).any()


@pytest.mark.parametrize("B", BITS)
def test_k_larger_than_n(dev, B):
    db = Db(dev, B, 5, 37, seed=15)
    Q = db.queries(3)
    got = db.search(Q, 10, L2)
    same(got, db.expect(Q, 10, L2))
    assert torch.isinf(got[0][:, 5:]).all() and (got[0][:, 5:] > 0).all()
    assert (got[1][:, 5:] == -1).all()  # 0xFFFFFFFF
    assert sorted(got[1][0, :5].tolist()) == [0, 1, 2, 3, 4]


@pytest.mark.parametrize("B", [2, 7, 8])
@pytest.mark.parametrize("nq,n", [(3, 1000), (16, 4100)])
def test_id_offset_at_the_top(dev, B, nq, n):
    db = Db(dev, B, n, 64, seed=17)
    off = 2 ** 32 - 1 - n
    Q = db.queries(nq)
    got = db.search(Q, 10, L2, id_offset=off)
    same(got, db.expect(Q, 10, L2, id_offset=off))
    base = db.search(Q, 10, L2)
    ids = got[1].to(torch.int64) & 0xFFFFFFFF
    assert torch.equal(ids, base[1].to(torch.int64) + off) and int(ids.max()) <= 2 ** 32 - 2
    with pytest.raises(ValueError, match="ids overflow"):
        db.search(Q, 10, L2, id_offset=off + 1)


def test_empty_database_and_no_queries(dev):
    db = Db(dev, 6, 4, 37, seed=19)
    Q = db.queries(3)
    full = db.codes
    db.codes = full[:0].contiguous()
    d, i = db.search(Q, 4, L2)
    assert d.shape == (3, 4) and torch.isinf(d).all() and (d > 0).all() and (i == -1).all()
    db.codes = full
    d, i = db.search(Q[:0].contiguous(), 4, IP)
    assert d.shape == (0, 4) and i.shape == (0, 4)


def test_binding_rejects_what_does_not_fit(dev):
    from haag_vq import _native

    db = Db(dev, 4, 10, 37, seed=21)
    Q = db.queries(2)
    with pytest.raises(ValueError, match=r"num_bits must be in \[1, 8\]"):
        _native.lvq_flat_search(Q, db.codes, db.mu, 9, 3)
    with pytest.raises(ValueError, match="bytes per row"):
        _native.lvq_flat_search(Q, db.codes, db.mu, 5, 3)
    with pytest.raises(ValueError, match="bytes per row"):
        _native.lvq_decode(db.codes[:, :-1].contiguous(), db.mu, 4)
    with pytest.raises(ValueError, match="queries d="):
        _native.lvq_flat_search(Q[:, :-1].contiguous(), db.codes, db.mu, 4, 3)


# ------------------------------------------------------------------------------ end to end
def _decode_path(model, codes, Q, k, metric):
    """What search_codes computes without the code-domain kernel: decompress + flat_search."""
    from haag_vq import _arrays, _native

    xh = _arrays.to_device(model.decompress(codes), torch.float32)
    d, i = _native.flat_search(_arrays.to_device(Q), xh, k, L2 if metric == "l2" else IP)
    return (d if metric == "l2" else -d).cpu().numpy(), i.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("name", list(LR.SEARCH_CASES))
@pytest.mark.parametrize("metric", LR.METRICS)
def test_index_end_to_end(dev, cases, monkeypatch, tmp_path, name, metric):
    """fit + search_with_scores: the mean and the codes are the reference's, the result passes
    the rule against the fixture and equals decode + flat_search bit for bit without the
    database being decoded; save / load round-trips."""
    from haag_vq import _native
    from haag_vq.methods.lvq_quantization import LVQQuantizer
    from haag_vq.methods.search.flat_quantized_index import FlatQuantizedIndex

    cs = cases(name)
    k = cs.c["k"]
    idx = FlatQuantizedIndex(LVQQuantizer(cs.B))
    idx.fit(cs.X, metric)
    np.testing.assert_array_equal(idx.quantizer.mu.view(np.uint32), cs.mu.view(np.uint32))
    np.testing.assert_array_equal(idx._codes.cpu().numpy(), cs.codes)
    assert idx.memory_footprint() == cs.codes.nbytes
    want_d, want_i = _decode_path(idx.quantizer, idx._codes, cs.Q, min(k, cs.N), metric)

    def boom(*a, **kw):
        raise AssertionError("the database was decoded")

    with monkeypatch.context() as m:
        m.setattr(_native, "lvq_decode", boom)
        ids, dists = idx.search_with_scores(cs.Q, k)
    j = cs.judge(metric)
    print(f"\n[lvq-golden] device {name} {metric}: open share {j.open_share:.4f}, "
          f"max |dist - key| / e {j.ratio(ids, dists):.4f}")
    assert ids.shape == (cs.c["nq"], min(k, cs.N))
    j.check(ids, dists, f"device {name} {metric}")
    np.testing.assert_array_equal(ids, want_i)
    np.testing.assert_array_equal(dists.view(np.uint32), want_d.view(np.uint32))
    path = tmp_path / "lvq_index.npz"
    idx.save(path)
    back = FlatQuantizedIndex(LVQQuantizer(1))
    back.load(path)
    assert isinstance(back.quantizer, LVQQuantizer) and back.quantizer.num_bits == cs.B
    ids2, dists2 = back.search_with_scores(cs.Q, k)
    np.testing.assert_array_equal(ids2, ids)
    np.testing.assert_array_equal(dists2.view(np.uint32), dists.view(np.uint32))


@pytest.mark.parametrize("metric", LR.METRICS)
def test_large_k_goes_through_decompress(dev, cases, metric):
    from haag_vq.methods.lvq_quantization import LVQQuantizer
    from haag_vq.methods.search import flat_quantized_index as fqi
    from _search_rule import Judge

    cs = cases("b3_d37")
    k = 300
    assert k > fqi.MAX_KERNEL_K
    idx = fqi.FlatQuantizedIndex(LVQQuantizer(cs.B))
    idx.fit(cs.X, metric)
    ids, dists = idx.search_with_scores(cs.Q, k)
    Judge(cs.Q, cs.rec, metric, k).check(ids, dists, f"large k {metric}")


@pytest.mark.parametrize("B", [1, 4, 7])
@pytest.mark.parametrize("metric", LR.METRICS)
def test_planted_rows_come_back_adjacent(dev, B, metric):
    """Rows 5, 17 and 509 are identical and the query is that row: the three are adjacent in
    ascending id order with one distance (first, at 0 from their common reconstruction's
    point of view, under L2)."""
    from haag_vq.methods.lvq_quantization import LVQQuantizer
    from haag_vq.methods.search.flat_quantized_index import FlatQuantizedIndex

    rng = np.random.default_rng(77)
    X = rng.standard_normal((512, 32)).astype(np.float32)
    X[17] = X[5]
    X[509] = X[5]
    Q = np.concatenate([X[5:6], rng.standard_normal((3, 32)).astype(np.float32)])
    idx = FlatQuantizedIndex(LVQQuantizer(B))
    idx.fit(X, metric)
    ids, dists = idx.search_with_scores(Q, 64)
    pos = [int(np.flatnonzero(ids[0] == r)[0]) for r in (5, 17, 509)]
    assert pos[1] == pos[0] + 1 and pos[2] == pos[0] + 2
    assert dists[0, pos[0]] == dists[0, pos[1]] == dists[0, pos[2]]
    if metric == "l2" and B >= 4:
        assert pos[0] == 0


def test_study_runs_lvq(dev):
    """build_quantizer("lvq", b, D) through the adapter the study uses: fit, reconstruct by id,
    stored bytes."""
    from haag_vq.benchmarks.method_registry import build_quantizer
    from haag_vq.benchmarks.quantizer_adapters import NORM_SIDECHANNEL_BYTES

    rng = np.random.default_rng(41)
    X = rng.standard_normal((300, 48)).astype(np.float32)
    a = build_quantizer("lvq", 4, 48)
    a.fit(X)
    assert a.code_bytes() == 300 * (LR.code_size(48, 4) + NORM_SIDECHANNEL_BYTES)
    ids = np.array([7, 0, 299, 7])
    mu = X.mean(axis=0)
    want = LR.decode(LR.encode(X, mu, 4), mu, 4)[ids]
    np.testing.assert_array_equal(a.reconstruct(ids).view(np.uint32), want.view(np.uint32))


def test_run_study_arrays_lvq(dev):
    from haag_vq.benchmarks.quantizer_study import run_study_arrays

    rng = np.random.default_rng(0)
    X = rng.standard_normal((1000, 48)).astype(np.float32)
    Q = rng.standard_normal((50, 48)).astype(np.float32)
    df = run_study_arrays(X, Q, methods=["lvq"], bpd_values=[2, 4, 8], ks=(1, 10), chunk_size=256, mse_sample=1000)
    assert len(df) == 3 and (df["method"] == "lvq").all()
    assert df["recall_at_10"].between(0, 1).all() and (df["compression_factor"] > 1).all()
    sub = df.sort_values("bpd")
    assert sub["mse"].is_monotonic_decreasing and sub["recall_at_10"].iloc[2] >= sub["recall_at_10"].iloc[0]
    assert sub["compression_factor"].is_monotonic_decreasing
