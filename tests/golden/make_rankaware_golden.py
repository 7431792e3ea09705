"""Generate tests/golden/rankaware_golden.npz from the REFERENCE implementation.

Run where the reference's sources are (they are not on the GPU box), on the CPU:

    PYTHONPATH=/root/reference/src python tests/golden/make_rankaware_golden.py

For every case of tests/_rankaware_rule.py (inputs regenerated from the case's seed) it stores
what the reference's RankAwareQuantizer (methods/rank_aware_quantization.py) produced:

  <case>_X_sha                          digest of the inputs
  <case>_mu, _V, _var, _bits, _cb       fit's state (cb: the per-dimension tables, concatenated);
                                        the same for both packings, which the generator asserts
  <case>_offsets                        the dense bit offsets (D + 1,)
  <case>_ffd_byte_idx, _ffd_bit_off     the FFD layout (packing="ffd")
  <case>_{dense,ffd}_code_size, _codes  compress(X) per packing
  <case>_rec                            decompress(codes): the same bits for both packings,
                                        which the generator asserts
  levels, Dg                            _levels[b] (b = 0..8, concatenated) and _Dg of seed 0

A case is refused (change its draw in _rankaware_rule.CASES) when
  * re-evaluating the projection in another fp64 summation order (matmul_seq against numpy's
    BLAS) flips more than 1e-3 of the indices, or a flipped index breaks the tie rule;
  * at any step of the allocation greedy the chosen gain is within 1e-9 relative of the
    runner-up: `bits` would then not be reproducible from a Gram matrix that differs in the
    last bits.
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

import _rankaware_rule as RR  # noqa: E402

GAIN_MARGIN = 1e-9


def _savez_fixed(path: Path, arrays: dict) -> None:
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for key in arrays:
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[key]), allow_pickle=False)
            zf.writestr(zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue())


def _greedy_margin(var, Dg, avg_bits, alpha, max_bits):
    """The allocation replayed with the smallest relative margin between the chosen gain and the
    runner-up over all steps: (bits, margin)."""
    D = len(var)
    bits = np.zeros(D, dtype=np.int64)
    vp = var ** (1.0 + alpha)
    gain = vp * (Dg[0] - Dg[1])
    margin = np.inf
    for _ in range(int(round(avg_bits * D))):
        d = int(np.argmax(gain))
        if not np.isfinite(gain[d]):
            break
        rest = np.delete(gain, d)
        if len(rest) and np.isfinite(rest.max()):
            margin = min(margin, (gain[d] - rest.max()) / abs(gain[d]))
        bits[d] += 1
        gain[d] = vp[d] * (Dg[bits[d]] - Dg[bits[d] + 1]) if bits[d] < max_bits else -np.inf
    return bits, margin


def main() -> None:
    import haag_vq.methods.rank_aware_quantization as ram

    src = Path(ram.__file__).resolve()
    assert "/reference/" in str(src), f"this must import the reference's haag_vq, not {src}"
    lloyd, memo = ram._lloyd_1d_normal, {}

    def lloyd_memo(num_levels, seed, *a, **k):
        key = (num_levels, seed, a, tuple(sorted(k.items())))
        if key not in memo:
            memo[key] = lloyd(num_levels, seed, *a, **k)
        lv, dmse = memo[key]
        return lv.copy(), dmse

    ram._lloyd_1d_normal = lloyd_memo
    arrays = {"cases": np.array(list(RR.CASES))}
    for name, c in RR.CASES.items():
        X = RR.inputs(name)
        arrays[f"{name}_X_sha"] = np.array(RR.sha(X))
        fitted = {}
        for packing in RR.PACKINGS:
            q = ram.RankAwareQuantizer(c["avg_bits"], alpha=c["alpha"], max_bits=c["max_bits"], seed=0, packing=packing)
            q.fit(X)
            codes = q.compress(X)
            rec = q.decompress(codes)
            assert codes.dtype == np.uint8 and codes.shape == (c["N"], q.code_size) and rec.dtype == np.float32
            assert q.bits.dtype == np.int64 and q.mu.dtype == np.float64 and q.V.dtype == np.float64
            fitted[packing] = (q, codes, rec)
            arrays[f"{name}_{packing}_code_size"] = np.array(q.code_size)
            arrays[f"{name}_{packing}_codes"] = codes
        (qd, cd, rd), (qf, cf, rf) = fitted["dense"], fitted["ffd"]
        for a, b in ((qd.mu, qf.mu), (qd.V, qf.V), (qd.var, qf.var), (qd.bits, qf.bits), (qd._offsets, qf._offsets),
                     (np.concatenate(qd.cb), np.concatenate(qf.cb)), (rd, rf)):
            assert np.array_equal(a, b), f"{name}: dense and ffd fits differ"
        arrays[f"{name}_mu"] = qd.mu
        arrays[f"{name}_V"] = np.ascontiguousarray(qd.V)
        arrays[f"{name}_var"] = qd.var
        arrays[f"{name}_bits"] = qd.bits
        arrays[f"{name}_cb"] = np.concatenate(qd.cb)
        arrays[f"{name}_offsets"] = qd._offsets
        arrays[f"{name}_ffd_byte_idx"] = qf._ffd_byte_idx
        arrays[f"{name}_ffd_bit_off"] = qf._ffd_bit_off
        arrays[f"{name}_rec"] = rd
        assert qf._ffd_n_bytes == qf.code_size
        if name == "all8":
            assert np.all(qd.bits == 8) and np.array_equal(cd, cf), "all8: dense and ffd bytes must be identical"
        if name == "w08":
            assert set(qd.bits.tolist()) == set(range(9)), f"w08: widths {sorted(set(qd.bits.tolist()))}"

        bits, margin = _greedy_margin(qd.var, qd._Dg, c["avg_bits"], c["alpha"], c["max_bits"])
        assert np.array_equal(bits, qd.bits)
        if margin < GAIN_MARGIN:
            raise SystemExit(f"{name}: greedy margin {margin:.3e} < {GAIN_MARGIN}: change its draw")
        line = f"{name}: N={c['N']} D={c['D']} widths {np.bincount(qd.bits, minlength=9).tolist()} margin {margin:.2e}"
        for packing in RR.PACKINGS:
            q, codes, _ = fitted[packing]
            st = RR.fixture_state(arrays, name, packing)
            Y = RR.project(X, st)
            ref_idx = RR.unpack(codes, st)
            assert np.array_equal(RR.pack(ref_idx, st), codes), f"{name} {packing}: bits outside the fields"
            problems = RR.tie_problems(RR.indices(Y, st), ref_idx, Y, X, st)
            if problems:
                raise SystemExit(f"{name} {packing}: {problems[:3]}: change its draw")
            flips = int((RR.indices(Y, st) != ref_idx).sum())
            line += f"  {packing}: code_size {q.code_size}, {flips} flips"
        print(line)

    q = ram.RankAwareQuantizer(4.0, max_bits=8, seed=0)
    q.fit(RR.inputs("all8"))
    arrays["levels"] = np.concatenate(q._levels)
    arrays["Dg"] = q._Dg
    path = OUT / RR.GOLDEN
    _savez_fixed(path, arrays)
    print(f"wrote {path} ({path.stat().st_size} bytes)")


if __name__ == "__main__":
    main()
