"""The fast Hadamard rotation of include/mivq.h in numpy, on np.longdouble rows by default, and
the Extended RaBitQ pipeline (the reference's normalize / searchsorted / t) with it as rotation."""

import numpy as np

ROUNDS = 4
U = 2.0 ** -53


def draw_signs(seed, D, rounds=ROUNDS):
    return np.random.default_rng(seed).integers(0, 2, size=(rounds, D)).astype(np.uint8)


def bound(D, rounds=ROUNDS):
    """Per element, for a row of unit norm: log2 T + 3 rounding stages a round, a margin of 2."""
    return 2 * rounds * ((D.bit_length() - 1) + 3) * U


def apply(x, signs, inverse=False, dtype=np.longdouble):
    x = np.array(x, dtype=dtype, ndmin=2)
    n, D = x.shape
    T, h = 1 << (D.bit_length() - 1), D // 2

    def flip(r):
        x[:, signs[r] == 1] *= -1

    def hadamard(r):
        off, ln = (D - T if r % 2 else 0), 1
        while ln < T:
            w = x[:, off:off + T].reshape(n, T // (2 * ln), 2, ln)
            x[:, off:off + T] = np.stack((w[:, :, 0] + w[:, :, 1], w[:, :, 0] - w[:, :, 1]), axis=2).reshape(n, T)
            ln *= 2
        x[:, off:off + T] /= np.sqrt(dtype(T))

    def mix(r):
        if T < D:
            a, b = x[:, :h].copy(), x[:, D - h:].copy()
            x[:, :h], x[:, D - h:] = (a + b) / np.sqrt(dtype(2)), (a - b) / np.sqrt(dtype(2))

    steps = (flip, hadamard, mix)
    for r in (range(len(signs) - 1, -1, -1) if inverse else range(len(signs))):
        for step in (steps[::-1] if inverse else steps):
            step(r)
    return x


def case(D, n=200, seed=3):
    """(X f32, c, signs, levels) of test 3: what ExtendedRaBitQuantizer(4, seed, "fht").fit(X) holds."""
    from haag_vq.methods.extended_rabitq import _lloyd_1d_normal

    X = (np.random.default_rng(100 + D).standard_normal((n, D)) * 1.5 + 0.25).astype(np.float32)
    return X, X.mean(axis=0).astype(np.float64), draw_signs(seed, D), _lloyd_1d_normal(16, seed=seed)


def encode(X, c, signs, levels, dtype=np.longdouble):
    """(idx, s, nrm, t): the reference's compress in fp64 with apply(dtype) as the rotation."""
    r = X.astype(np.float64) - c
    nrm = np.linalg.norm(r, axis=1)
    s = apply(r / np.maximum(nrm, 1e-12)[:, None], signs, dtype=dtype) * np.sqrt(dtype(X.shape[1]))
    idx = np.searchsorted(0.5 * (levels[:-1] + levels[1:]), s.astype(np.float64))
    sh = levels[idx]
    den = (sh * sh).sum(axis=1)
    t = np.where(den > 1e-12, (s.astype(np.float64) * sh).sum(axis=1) / np.maximum(den, 1e-300), 1.0)
    return idx, s, nrm, t


def decode(idx, nrm, t, c, signs, levels):
    o_hat = levels[idx] / np.sqrt(idx.shape[1]) * t.astype(np.float32).astype(np.float64)[:, None]
    y = apply(o_hat, signs, inverse=True).astype(np.float64)
    return y * nrm.astype(np.float32).astype(np.float64)[:, None] + c


# The buffer-contract cases of the three entry points (tests/_bounds.py; test_guard_cpu.py asks for
# one of each kind per entry point).  The byte-level reference is the staged composition's call on
# the same inputs.  d = 37 rotates in LDS, d = 256 in registers with a partial last workgroup.
def _bounds_case(entry, n, d, nb=3):
    import _bounds as B

    def build(O):
        r = B.rng(n, d, 40)
        X, cen, lv = r.standard_normal((n, d)), r.standard_normal(d) * 0.1, np.sort(r.standard_normal(1 << nb))
        sg, cs = draw_signs(5, d), (d * nb + 7) // 8 + 8
        codes = r.integers(0, 256, (n, cs), dtype=np.uint8)
        codes[:, cs - 8:] = r.uniform(0.5, 2.0, (n, 2)).astype(np.float32).view(np.uint8)
        np_ = lambda t: t.cpu().numpy()  # noqa: E731
        if entry == "mivq_fht_rotate":
            return B.Call([B.In("in", X), n, d, B.In("signs", sg), ROUNDS, 1, B.Out("out", n * d * 8), None],
                          expect=lambda c: {"out": np_(c.N.fht_rotate(c.t(X), c.t(sg), True))})
        if entry == "mivq_extrabitq_encode_fht":
            def want(c):
                o, nrm = c.N.extrabitq_normalize(c.t(X), c.t(cen))
                return {"codes": np_(c.N.extrabitq_quantize(c.N.fht_rotate(o, c.t(sg)), c.t(lv), nb, nrm))}
            return B.Call([B.In("x", X), 1, n, d, B.In("centroid", cen), B.In("signs", sg), ROUNDS, B.In("levels", lv), nb,
                           B.Out("codes", n * cs), None], expect=want)

        def want(c):
            y = c.N.fht_rotate(c.N.extrabitq_dequantize(c.t(codes), c.t(lv), nb, d), c.t(sg), True)
            return {"out": np_(c.N.extrabitq_finish(y, c.t(codes), c.t(cen), nb))}
        return B.Call([B.In("codes", codes), n, d, B.In("centroid", cen), B.In("signs", sg), ROUNDS, B.In("levels", lv), nb,
                       B.Out("out", n * d * 4), None], expect=want)
    B.add(entry, f"n{n}-d{d}", B.EMPTY if n == 0 else B.RAGGED if d == 37 else B.EDGE, build)
    return B.CASES[-1]


BOUNDS_CASES = [_bounds_case(e, n, d) for e in ("mivq_fht_rotate", "mivq_extrabitq_encode_fht", "mivq_extrabitq_decode_fht")
                for n, d in ((130, 37), (5, 256), (0, 37))]
