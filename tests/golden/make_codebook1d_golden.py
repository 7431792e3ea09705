"""Generate tests/golden/codebook1d_golden.npz from the REFERENCE's codebook builders.

Run on the CPU where the reference's sources are, with the reference's ``haag_vq`` and its ``saq``
extension module importable (the module is taken from its wheel, unpacked with zipfile into a
scratch directory; nothing of it is installed or copied here):

    PYTHONPATH=<reference>/src:<scratch dir with saq> python tests/golden/make_codebook1d_golden.py

Column cases (tests/_codebook1d_rule.COLUMN_CASES, inputs regenerated from the case's seed):

  col_<case>_seed, _kind      what the column is drawn from: (n, width, draw) and the kind's name,
                              the arguments of _codebook1d_rule.column's generator
  col_<case>_sha              digest of the sorted f32 column
  col_<case>_<method>         saq.build_codebook_exact / build_codebook_lloyd at the case's width:
                              the 2 ** w f32 levels (the reference's short Lloyd table of a
                              degenerate column padded with its last level)
  col_<case>_<method>_cost    the reference's cost, f32(sse / n)
  col_<case>_lloyd_seed       the Lloyd builder with max_iters = 0: the seeding, as levels
                              (non-degenerate columns only)

Fit cases (every case of tests/_rankaware_rule.CASES):

  <case>_cb_lloyd, _cb_exact  RankAwareQuantizer(codebook=...).fit(X).cb, concatenated f64 (a short
                              Lloyd table of a degenerate dimension padded with its last level)

Nothing is written unless
  * the rule (tests/_codebook1d_rule.py) gives the reference's bits for every array above,
  * the Lloyd column cases hold a run with a repair, a run that uses all 50 passes and a run that
    converges earlier,
  * every fit's ``bits`` are those of rankaware_golden.npz, and projecting the sample in another
    fp64 summation order (_rankaware_rule.project) changes no f32 sample value.
Plain arrays only, written with fixed member timestamps so the same arrays give the same bytes.
"""

from __future__ import annotations

import io
import sys
import zipfile
from pathlib import Path

import numpy as np

OUT = Path(__file__).resolve().parent
sys.path.insert(0, str(OUT.parent))

import _codebook1d_rule as CR  # noqa: E402
import _rankaware_rule as RR  # noqa: E402


def _savez_fixed(path: Path, arrays: dict) -> None:
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for key in arrays:
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[key]), allow_pickle=False)
            zf.writestr(zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue())


def _same_bits(a, b) -> bool:
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _reference(saq, s, w: int, method: str, max_iters=None):
    if method == "exact":
        r = saq.build_codebook_exact(s, w)
    else:
        o = saq.LloydOpts()
        o.max_bits = w
        if max_iters is not None:
            o.max_iters = max_iters
        r = saq.build_codebook_lloyd(s, o)
    levels = np.asarray(r.codebooks[w].centroids, dtype=np.float32)
    return CR._pad(levels, 1 << w), np.float32(r.costs[w])


def column_cases(saq, arrays: dict) -> None:
    seen = dict(repair=False, full=False, early=False)
    for name, (n, w, _, _) in CR.COLUMN_CASES.items():
        s = CR.column(name)
        assert s.dtype == np.float32 and s.shape == (n,) and np.all(s[1:] >= s[:-1])
        arrays[f"col_{name}_sha"] = np.array(CR.sha(s))
        arrays[f"col_{name}_seed"] = np.array([n, w, CR.COLUMN_CASES[name][3]], dtype=np.int64)
        arrays[f"col_{name}_kind"] = np.array(CR.COLUMN_CASES[name][2])
        degenerate = (1 << w) >= len(CR.distinct(s))
        for method in CR.METHODS:
            want, cost = _reference(saq, s, w, method)
            info = {}
            got, sse = CR.exact(s, w) if method == "exact" else CR.lloyd(s, w, info=info)
            if not _same_bits(got, want) or np.float32(sse / n) != cost:
                raise SystemExit(f"{name} {method}: the rule differs from the reference")
            arrays[f"col_{name}_{method}"] = want
            arrays[f"col_{name}_{method}_cost"] = cost
            if method == "lloyd" and not degenerate:
                seed, _ = _reference(saq, s, w, "lloyd", max_iters=0)
                mine = CR._pad(np.unique(CR.seed_centres(s, 1 << w).astype(np.float32)), 1 << w)
                if not _same_bits(mine, seed):
                    raise SystemExit(f"{name}: the rule's seeding differs from the reference's")
                arrays[f"col_{name}_lloyd_seed"] = seed
                seen["repair"] |= info["repairs"] > 0
                seen["full"] |= info["passes"] == CR.MAX_PASSES and not info["converged"]
                seen["early"] |= info["converged"] and info["passes"] < CR.MAX_PASSES
                print(f"{name}: n={n} w={w} lloyd {info}")
    if not all(seen.values()):
        raise SystemExit(f"the Lloyd cases miss a path: {seen}")


def fit_cases(ram, arrays: dict) -> None:
    z = RR.load_golden(OUT)
    lloyd, memo = ram._lloyd_1d_normal, {}

    def lloyd_memo(num_levels, seed, *a, **k):
        key = (num_levels, seed, a, tuple(sorted(k.items())))
        if key not in memo:
            memo[key] = lloyd(num_levels, seed, *a, **k)
        lv, dmse = memo[key]
        return lv.copy(), dmse

    ram._lloyd_1d_normal = lloyd_memo
    for name, c in RR.CASES.items():
        X = RR.inputs(name)
        assert RR.sha(X) == str(z[f"{name}_X_sha"])
        for method in CR.METHODS:
            q = ram.RankAwareQuantizer(c["avg_bits"], alpha=c["alpha"], max_bits=c["max_bits"], seed=0, codebook=method)
            q.fit(X)
            if not np.array_equal(q.bits, z[f"{name}_bits"]):
                raise SystemExit(f"{name} {method}: bits differ from {RR.GOLDEN}")
            assert _same_bits(q.mu, z[f"{name}_mu"]) and _same_bits(np.ascontiguousarray(q.V), z[f"{name}_V"])
            Y = ((np.asarray(X, dtype=np.float64) - q.mu) @ q.V).astype(np.float32)
            Y2 = RR.project(X, RR.fixture_state(z, name, "dense")).astype(np.float32)
            if not _same_bits(Y, Y2):
                raise SystemExit(f"{name}: {int((Y != Y2).sum())} f32 sample values depend on the summation order")
            short = [d for d, b in enumerate(q.bits) if len(q.cb[d]) != 2 ** b]
            assert method == "lloyd" or not short, f"{name}: a short exact table"
            cb = np.concatenate([np.concatenate((t, np.full(2 ** int(b) - len(t), t[-1])))
                                 for t, b in zip(q.cb, q.bits)]).astype(np.float64)
            mine = [CR.fit(np.sort(Y[:, d]), int(b), method)[0].astype(np.float64) if b else np.array([0.0])
                    for d, b in enumerate(q.bits)]
            if not _same_bits(np.concatenate(mine), cb):
                raise SystemExit(f"{name} {method}: the rule differs from the reference's fit")
            arrays[f"{name}_cb_{method}"] = cb
        print(f"{name}: N={c['N']} D={c['D']} fits stored, {len(short)} short lloyd tables padded")


def main() -> None:
    import haag_vq.methods.rank_aware_quantization as ram
    import saq

    assert "/reference/" in str(Path(ram.__file__).resolve()), "this must import the reference's haag_vq"
    arrays = {"column_cases": np.array(list(CR.COLUMN_CASES)), "fit_cases": np.array(list(RR.CASES))}
    column_cases(saq, arrays)
    fit_cases(ram, arrays)
    path = OUT / CR.GOLDEN
    _savez_fixed(path, arrays)
    print(f"wrote {path} ({path.stat().st_size} bytes)")


if __name__ == "__main__":
    main()
