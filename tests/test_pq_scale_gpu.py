"""PQ encode across codebook and row magnitudes: both regimes of the fp16 filter (sigma = 1 and
sigma = 2^(12 - e)), rows near and past the Xs < 65000 threshold, subspaces of different regimes
in one call, non-centred data that fills the pair and full lists, f16-subnormal rows.

Every case is held bit for bit to the CPU oracle at its own scale, on the default path, the
exact path and (dsub <= 128) the legacy MFMA kernel; `scaled(s)` also to the device's own codes
at s = 0 (the canonical fp32 chains do not see a common power of two).  The inputs and the rule
are tests/_pq_filter_rule.py; tests/test_pq_filter_rule_cpu.py shows on the oracle alone that
each family reaches what it is built for.

Shapes: M = 2 and n = 3001 (a ragged last block, the generic code transpose), one dsub per
filter specialisation:

    96 -> DS 96, 12 waves     48 -> DS 48, 16 waves     64 -> DS 64, per-block sigma test
    128, 160, 192 -> K-halves, 8 waves      140 -> wide generic, 4 waves
    8, 24, 20 -> generic loop, load layouts 1, 3, 0

With two subspaces the launcher gives every workgroup one 32-row block per wave, so
`test_scaled_regime_many_blocks_per_wave` runs M = 64 as well: there each wave streams several
blocks and the pair held from one block is settled in the next.
"""

import numpy as np
import pytest

import _pq_filter_rule as R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

N = 3001
DSUBS = (96, 48, 64, 128, 160, 192, 140, 8, 24, 20)
EXPS = (-41, -9, -8, 8, 9, 39)
FAMILY_DSUBS = (96, 64, 192)


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _h(t):
    return t.detach().cpu().numpy()


def _paths(dsub):
    from haag_vq import _native

    p = [("default", {}), ("exact", dict(exact=True))]
    if dsub <= 128:
        p.append(("legacy", dict(flags_extra=_native.MIVQ_PQ_LEGACY_MFMA)))
    return p


def _encode_all(dev, X, C):
    """name -> (n, M) codes of every path, one prepare."""
    from haag_vq import _native

    Cd, Xd = _t(C, dev), _t(X, dev)
    prep = _native.pq_prepare(Cd, 8)
    return {name: _h(_native.pq_encode(Xd, Cd, prep, 8, **kw)) for name, kw in _paths(C.shape[2])}


def _check_all(dev, oracle, X, C, also=None):
    ref = oracle.pq_encode(X, C)
    got = _encode_all(dev, X, C)
    for name, codes in got.items():
        np.testing.assert_array_equal(codes, ref, err_msg=f"{name} path vs the oracle")
        if also is not None:
            np.testing.assert_array_equal(codes, also[name], err_msg=f"{name} path vs its codes at scale 1")
    return got


_at_scale_one = {}


def _scale_one(dev, n, dsub, M):
    """The device's codes of scaled(0) on every path (computed once per shape)."""
    key = (n, dsub, M)
    if key not in _at_scale_one:
        _at_scale_one[key] = _encode_all(dev, *R.scaled(0, n, dsub, M))
    return _at_scale_one[key]


@pytest.mark.parametrize("e", EXPS)
@pytest.mark.parametrize("dsub", DSUBS)
def test_scaled_regimes_bit_exact(dev, oracle, dsub, e):
    X, C = R.scaled(R.s_for_exp(e, N, dsub), N, dsub)
    assert R.exps(C) == [e, e]
    _check_all(dev, oracle, X, C, also=_scale_one(dev, N, dsub, 2))


@pytest.mark.parametrize("e", [-9, 9])
def test_scaled_regimes_headline_shape(dev, oracle, e):
    """1536 x M 16 at n = 1008, a multiple of 16: the 16-byte code transpose."""
    n, dsub, M = 1008, 96, 16
    X, C = R.scaled(R.s_for_exp(e, n, dsub, M), n, dsub, M)
    assert R.exps(C) == [e] * M
    _check_all(dev, oracle, X, C, also=_scale_one(dev, n, dsub, M))


@pytest.mark.parametrize("e", EXPS)
@pytest.mark.parametrize("dsub", DSUBS)
def test_prep_constants_follow_the_rule(dev, dsub, e):
    """bnd = {sigma, 1.0625 a, 1.0625 b, tau} of the prepare buffer: sigma and tau exactly the
    rule's; a and b at least the rule's fp64 values (the kernel evaluates them in fp32 with
    (1 + 1e-5) and (1 + 1e-6) factors) and at most 1e-3 above."""
    from haag_vq import _native

    M = 2
    _, C = R.scaled(R.s_for_exp(e, N, dsub), N, dsub)
    raw = _h(_native.pq_prepare(_t(C, dev), 8))
    off = R.prep_offsets(M, dsub)["bnd"]
    bnd = raw[off:off + 16 * M].view(np.float32).reshape(M, 4).astype(np.float64)
    for m in range(M):
        sigma, tau = R.sigma_tau(R.scale_exp(C[m]))
        a, b = R.window(C[m])
        print(f"dsub {dsub} e {e} m {m}: sigma {bnd[m, 0]:g} tau {bnd[m, 3]:g} "
              f"a / rule {bnd[m, 1] / (R.SAFETY * a):.7f} b / rule {bnd[m, 2] / (R.SAFETY * b):.7f}")
        assert bnd[m, 0] == sigma and bnd[m, 3] == tau
        for got, want in ((bnd[m, 1], a), (bnd[m, 2], b)):
            assert got >= R.SAFETY * want * (1 - 1e-4), (m, got, want)
            assert got <= R.SAFETY * want * (1 + 1e-3), (m, got, want)


@pytest.mark.parametrize("dsub", FAMILY_DSUBS)
@pytest.mark.parametrize("name", sorted(R.FAMILIES))
def test_families_bit_exact(dev, oracle, name, dsub):
    X, C = R.family(name, N, dsub)
    _check_all(dev, oracle, X, C)


def test_pairs_and_fulls_many_chunks(dev, oracle):
    """n = 40 001 at dsub 96: more than a hundred row chunks per subspace, each with both of its
    lists nearly full, side by side in the workspace."""
    X, C = R.pairs_and_fulls(40_001, 96)
    _check_all(dev, oracle, X, C)


@pytest.mark.parametrize("dsub", [96, 64])
def test_scaled_regime_many_blocks_per_wave(dev, oracle, dsub):
    """M = 64 (d = 64 dsub) at n = 6145: four row chunks of 49 blocks, so every wave streams three
    or four 32-row blocks (the pair held from one block settles in the next; dsub 64 tests sigma
    per block), on pairs_and_fulls times 2^10 (e = 13: the scaled staging loop, both lists in
    use)."""
    X, C = R.pairs_and_fulls(6145, dsub, M=64)
    f = np.float32(2.0 ** 10)
    X, C = X * f, C * f
    assert all(R.sigma_tau(e)[0] != 1.0 for e in R.exps(C))
    _check_all(dev, oracle, X, C)


@pytest.mark.parametrize("exact_assign", [False, True])
@pytest.mark.parametrize("s", [-20, 12])
def test_train_pq_is_scale_equivariant(dev, s, exact_assign):
    """train_pq(2^s X) == 2^s train_pq(X) bit for bit: the assignment is the canonical encode
    (here through the filter's scaled regime), and the update's ascending-row sums and its
    division commute with a power of two."""
    from haag_vq.methods._kmeans import train_pq

    X = R.base(4096, 96, 2, seed=7)[0]
    f = np.float32(2.0 ** s)
    C1 = _h(train_pq(_t(X, dev), 2, 8, niter=4, exact_assign=exact_assign))
    Cs = _h(train_pq(_t(X * f, dev), 2, 8, niter=4, exact_assign=exact_assign))
    assert all(R.sigma_tau(e)[0] != 1.0 for e in R.exps(Cs))
    np.testing.assert_array_equal(Cs, C1 * f)
