"""Generate tests/golden/ivf_quantized_golden.npz from the REFERENCE implementation.

Run in the build container only (it imports the reference's sources, which do not exist on the
GPU box), on the CPU, with the reference's src directory first on the path:

    PYTHONPATH=<reference>/src python tests/golden/make_ivf_quantized_golden.py

For every case of tests/_ivf_quantized_rule.py (inputs regenerated from the seed) and both
metrics it builds the reference's IvfQuantizedIndex (methods/search/ivf_quantized_index.py) by
setting its state directly -- IvfQuantizedIndex.fit imports faiss, which is absent -- from the
case's seeded centroids and the fp64 nearest-centroid assignment, fits and compresses the
reference's ScalarQuantizer / LVQQuantizer per list exactly as fit() does, puts a stub in
place of the faiss centroid index (it returns the fp64 nearest lists), and runs the reference's
own search_with_scores.  Stored:

  <case>_seed, _X_sha, _Q_sha, _coarse_sha   the seed and digests of the inputs
  <case>_<metric>_assign, _probes            the assignment (N,) and the probed lists (nq, nprobe)
  <case>_<metric>_lo, _den | _mu             the per-list parameters (K, D) (an empty list:
                                             lo = 0, den = 1e-8, mu = 0, the library's convention)
  <case>_<metric>_codes_sha, _codes_head     compress() of every list, in row order: digest and
                                             the first 8 rows
  <case>_<metric>_ids, _dists, _open         the reference's result and the open masks of the
                                             per-query Judges (tests/_search_rule.py)

A case whose open share exceeds OPEN_CAP, or whose reference result the Judge rejects, is
refused: give it another draw in _ivf_quantized_rule.DRAWS.  Plain arrays only, written with
fixed member timestamps so the same arrays give the same bytes.
"""

from __future__ import annotations

import io
import sys
import zipfile
from pathlib import Path

import numpy as np

OUT = Path(__file__).resolve().parent
sys.path.insert(0, str(OUT.parent))
sys.path.insert(0, str(OUT.parents[1] / "oracle"))

import _ivf_quantized_rule as IR  # noqa: E402
import _search_rule as SR  # noqa: E402


def _savez_fixed(path: Path, arrays: dict) -> None:
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for key in arrays:
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[key]), allow_pickle=False)
            zf.writestr(zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue())


class _Probes:
    """Stands in for the faiss centroid index: search() returns the fp64 nearest lists."""

    def __init__(self, coarse, metric):
        self.coarse, self.metric = coarse, metric

    def search(self, Q, n):
        return None, IR.probes64(Q, self.coarse, self.metric, n)


def main() -> None:
    import oracle as O
    from haag_vq.methods.lvq_quantization import LVQQuantizer
    from haag_vq.methods.scalar_quantization import ScalarQuantizer
    from haag_vq.methods.search.ivf_quantized_index import IvfQuantizedIndex

    for cls in (LVQQuantizer, IvfQuantizedIndex):
        src = Path(sys.modules[cls.__module__].__file__).resolve()
        assert "/reference/" in str(src), f"this must import the reference's haag_vq, not {src}"
    arrays = {"cases": np.array(list(IR.CASES))}
    for name, c in IR.CASES.items():
        kind, bits, N, D = c["kind"], c["bits"], c["N"], c["D"]
        X, Q, coarse = IR.inputs(name)
        arrays[f"{name}_seed"] = np.array(IR.seed_of(name))
        arrays[f"{name}_X_sha"] = np.array(IR.sha(X))
        arrays[f"{name}_Q_sha"] = np.array(IR.sha(Q))
        arrays[f"{name}_coarse_sha"] = np.array(IR.sha(coarse))
        factory = (lambda: ScalarQuantizer(num_bits=bits)) if kind == "sq" else (lambda: LVQQuantizer(num_bits=bits))
        line = f"{name}: N={N} D={D} {kind}-{bits}"
        for metric in IR.METRICS:
            key = f"{name}_{metric}"
            assign = IR.assign64(X, coarse, metric)
            counts = np.bincount(assign, minlength=IR.K)
            assert (counts == 0).sum() == 1, f"{key}: list sizes {counts}: exactly one list must be empty"
            idx = IvfQuantizedIndex(factory, K=IR.K, nprobe=IR.NPROBE)
            idx._centroids, idx._metric, idx._N, idx._D = coarse, metric, N, D
            idx._centroid_index = _Probes(coarse, metric)
            width, dt = IR.code_shape(kind, bits, D)
            codes = np.zeros((N, width), dt)
            params = [np.zeros((IR.K, D), np.float32) for _ in range(2 if kind == "sq" else 1)]
            if kind == "sq":
                params[1][:] = np.float32(1e-8)
            for l in range(IR.K):  # the loop of IvfQuantizedIndex.fit
                mask = assign == l
                vid = np.where(mask)[0].astype(np.uint32)
                if not mask.any():
                    idx._cluster_quantizers.append(None)
                    idx._cluster_codes.append(np.array([], dtype=np.uint8))
                    idx._cluster_ids.append(vid)
                    continue
                residuals = X[mask] - coarse[l]
                q = factory()
                q.fit(residuals)
                lc = q.compress(residuals)
                idx._cluster_quantizers.append(q)
                idx._cluster_codes.append(lc)
                idx._cluster_ids.append(vid)
                assert lc.dtype == dt and lc.shape == (int(mask.sum()), width), (lc.dtype, lc.shape)
                codes[mask] = lc
                if kind == "sq":
                    assert q.min.dtype == np.float32
                    params[0][l] = q.min
                    params[1][l] = q.max - q.min + 1e-8  # the denominator of _compress_block / decompress
                    assert params[1].dtype == np.float32
                else:
                    assert q.mu.dtype == np.float32
                    params[0][l] = q.mu
            probes = IR.probes64(Q, coarse, metric, IR.NPROBE)
            ids, dists = idx.search_with_scores(Q, IR.TOPK)
            ids, dists = ids.astype(np.uint32), dists.astype(np.float32)
            # the Judges stand on the restatement's reconstruction of the reference's own codes
            offsets, order = O.bucket_sort(assign, IR.K)
            o64 = order.astype(np.int64)
            rec = IR.decode(O, codes, coarse, assign, params, kind, bits)
            js = IR.judges(Q, rec[o64], offsets, order.astype(np.uint32), IR.K, probes, metric, IR.TOPK)
            share = IR.open_share(js)
            if share > SR.OPEN_CAP:
                raise SystemExit(f"{key}: open share {share:.3f} > {SR.OPEN_CAP}: change its draw")
            bad = IR.problems(js, ids, dists, metric, tie_order=False)
            if bad:
                raise SystemExit(f"{key}: the reference's result breaks the rule: {bad[:3]}")
            arrays[f"{key}_assign"] = assign.astype(np.uint8)
            arrays[f"{key}_probes"] = probes.astype(np.uint8)
            for pname, p in zip(("lo", "den") if kind == "sq" else ("mu",), params):
                arrays[f"{key}_{pname}"] = p
            arrays[f"{key}_codes_sha"] = np.array(IR.sha(codes))
            arrays[f"{key}_codes_head"] = codes[:8]
            arrays[f"{key}_ids"] = ids
            arrays[f"{key}_dists"] = dists
            arrays[f"{key}_open"] = np.stack([j.open[0] for j, _ in js])
            line += f"  {metric}: lists {counts.tolist()} open {share:.4f}"
        print(line)
    path = OUT / "ivf_quantized_golden.npz"
    _savez_fixed(path, arrays)
    print(f"wrote {path} ({path.stat().st_size} bytes)")


if __name__ == "__main__":
    main()
