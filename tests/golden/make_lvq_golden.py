"""Generate tests/golden/lvq_golden.npz from the REFERENCE implementation.

Run in the build container only (it imports /root/reference/src, which does not exist on the
GPU box), on the CPU:

    PYTHONPATH=/root/reference/src python tests/golden/make_lvq_golden.py

For every case of tests/_lvq_rule.py (inputs regenerated from the seed [N, D, B]) it stores what
the reference's LVQQuantizer (methods/lvq_quantization.py:42-142) produced:

  <case>_seed, _X_sha, _Q_sha, _planted   the seed, digests of the inputs, the planted row
  <case>_mu                               fit's mean, in full
  <case>_codes | _codes_sha               compress(X): in full up to 64 KiB, else its digest
                                          and the first 8 rows (_codes_head)
  <case>_rec_sha, _rec_head               decompress(codes): digest and the first 4 rows
  <case>_{l2,ip}_{ids,dists,open}         (search cases) the reference's
                                          FlatQuantizedIndex(LVQQuantizer(B)) result and the open
                                          mask of tests/_search_rule.py's Judge
  round_b<B>_codes, _rec                  the planted half-to-even rows, mu = 0 set directly

A search case whose open share exceeds OPEN_CAP, or whose reference result the Judge rejects,
is refused: give it another draw in _lvq_rule.DRAWS.  Plain arrays only (numbers, masks,
digests), written with fixed member timestamps so the same arrays give the same bytes.
"""

from __future__ import annotations

import io
import sys
import zipfile
from pathlib import Path

import numpy as np

OUT = Path(__file__).resolve().parent
sys.path.insert(0, str(OUT.parent))

import _lvq_rule as LR  # noqa: E402
import _search_rule as SR  # noqa: E402

FULL_CODES_BYTES = 64 * 1024
ROUND_D = 16


def _savez_fixed(path: Path, arrays: dict) -> None:
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for key in arrays:
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[key]), allow_pickle=False)
            zf.writestr(zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue())


def main() -> None:
    from haag_vq.methods.lvq_quantization import LVQQuantizer
    from haag_vq.methods.search.flat_quantized_index import FlatQuantizedIndex

    src = Path(sys.modules[LVQQuantizer.__module__].__file__).resolve()
    assert "/reference/" in str(src), f"this must import the reference's haag_vq, not {src}"
    arrays = {"cases": np.array(list(LR.CASES))}
    for name, c in LR.CASES.items():
        N, D, B = c["N"], c["D"], c["B"]
        X, Q, planted = LR.inputs(name)
        q = LVQQuantizer(num_bits=B)
        q.fit(X)
        codes = q.compress(X)
        rec = q.decompress(codes)
        assert q.mu.dtype == np.float32 and codes.dtype == np.uint8 and rec.dtype == np.float32
        assert codes.shape == (N, LR.code_size(D, B))
        ib = codes.shape[1] - 8
        assert codes[planted, ib + 4:].copy().view("<f4")[0] == LR.TINY and not codes[planted, :ib].any()
        arrays[f"{name}_seed"] = np.array(LR.seed_of(name))
        arrays[f"{name}_X_sha"] = np.array(LR.sha(X))
        arrays[f"{name}_Q_sha"] = np.array(LR.sha(Q))
        arrays[f"{name}_planted"] = np.array(planted)
        arrays[f"{name}_mu"] = q.mu
        if codes.nbytes <= FULL_CODES_BYTES:
            arrays[f"{name}_codes"] = codes
        else:
            arrays[f"{name}_codes_sha"] = np.array(LR.sha(codes))
            arrays[f"{name}_codes_head"] = codes[:8]
        arrays[f"{name}_rec_sha"] = np.array(LR.sha(rec))
        arrays[f"{name}_rec_head"] = rec[:4]
        line = f"{name}: N={N} D={D} B={B} codes {codes.shape}"
        if name in LR.SEARCH_CASES:
            for metric in LR.METRICS:
                idx = FlatQuantizedIndex(LVQQuantizer(num_bits=B))
                idx.fit(X, metric)
                ids, dists = idx.search_with_scores(Q, c["k"])
                j = SR.Judge(Q, rec, metric, c["k"])
                if j.open_share > SR.OPEN_CAP:
                    raise SystemExit(f"{name} {metric}: open share {j.open_share:.3f} > {SR.OPEN_CAP}: change its draw")
                problems = j.problems(ids, dists.astype(np.float32))
                if problems:
                    raise SystemExit(f"{name} {metric}: the reference's result breaks the rule: {problems[:3]}")
                arrays[f"{name}_{metric}_ids"] = ids.astype(np.uint32)
                arrays[f"{name}_{metric}_dists"] = dists.astype(np.float32)
                arrays[f"{name}_{metric}_open"] = j.open
                line += f"  {metric}: open {j.open_share:.4f}"
        print(line)
    for B, lead, want in LR.ROUNDING:
        row, _ = LR.rounding_row(B, ROUND_D)
        q = LVQQuantizer(num_bits=B)
        q.mu = np.zeros(ROUND_D, dtype=np.float32)
        codes = q.compress(row[None, :])
        idx, _, _ = LR.unpack(codes, ROUND_D, B)
        assert list(idx[0, :len(want)]) == want, (B, idx[0])
        arrays[f"round_b{B}_codes"] = codes
        arrays[f"round_b{B}_rec"] = q.decompress(codes)
    path = OUT / "lvq_golden.npz"
    _savez_fixed(path, arrays)
    print(f"wrote {path} ({path.stat().st_size} bytes)")


if __name__ == "__main__":
    main()
