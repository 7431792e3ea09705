#!/usr/bin/env python3
"""RankAwareQuantizer against ExtendedRaBitQuantizer(4) of the same library, in one process.

Both quantizers centre a row, multiply it by a D x D fp64 matrix on mivq_extrabitq_rotate and
turn the product into about D / 2 bytes, so the row traffic and the GEMM are the same; the
difference is what the rank-aware format's kernels (ragged level tables, fields at any bit
position) cost.  Per shape and packing the two sides are warmed up, then timed alternately with
HIP events; medians are reported with the range.

  compress / decompress   the public calls on a device tensor, rank-aware vs Extended RaBitQ
  split                   the three launches of each direction on their own: center, GEMM,
                          quantize and dequantize, GEMM, finish; quantize and dequantize with the
                          share of 8 TB/s that 8 n d + n code_size bytes make of their time

  python tools/rankaware_ab.py                       # 100k x 1536 and 1M x 1024, avg_bits 4
  python tools/rankaware_ab.py --shapes 20000x256    # a smaller box
"""

from __future__ import annotations

import argparse
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "vector-quantization_amd"))

from haag_vq import _native  # noqa: E402
from haag_vq.methods.extended_rabitq import ExtendedRaBitQuantizer  # noqa: E402
from haag_vq.methods.rank_aware_quantization import RankAwareQuantizer  # noqa: E402

HBM_PEAK = 8.0e12


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3


def alternate(fns, reps, min_seconds):
    """Median / min / max seconds of each of `fns`, called in turn until each ran `reps` times
    and `min_seconds` in all."""
    for f in fns:
        f()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    while len(ts[0]) < reps or min(sum(t) for t in ts) < min_seconds:
        for t, f in zip(ts, fns):
            t.append(timed(f))
        if len(ts[0]) >= 200:
            break
    return [(sorted(t)[len(t) // 2], min(t), max(t), len(t)) for t in ts]


def ms(t):
    return f"{t[0] * 1e3:9.3f} ms ({t[1] * 1e3:.3f}..{t[2] * 1e3:.3f})"


def repacked(q, packing):
    """The same fit with another packing (the layout is a function of `bits`)."""
    r = RankAwareQuantizer(q.avg_bits, alpha=q.alpha, max_bits=q.max_bits, seed=q.seed, packing=packing)
    r.mu, r.V, r.var, r.bits, r.cb, r.D, r._levels, r._Dg = q.mu, q.V, q.var, q.bits, q.cb, q.D, q._levels, q._Dg
    r._layout()
    return r


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", nargs="+", default=["100000x1536", "1000000x1024"])
    ap.add_argument("--avg-bits", type=float, default=4.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--min-seconds", type=float, default=0.3)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    dev = _native.require_device()
    g = torch.Generator(device=dev).manual_seed(a.seed)
    print(f"# {torch.cuda.get_device_name(0)}  avg_bits={a.avg_bits}  kernels {_native.kernel_source_hash()}")
    for shape in a.shapes:
        n, d = (int(v) for v in shape.split("x"))
        std = 2.0 * 1e-2 ** (torch.arange(d, device=dev) / max(d - 1, 1))
        X = torch.randn((n, d), generator=g, device=dev) * std + torch.randn(d, generator=g, device=dev)
        t0 = time.perf_counter()
        base = RankAwareQuantizer(a.avg_bits)
        base.fit(X)
        torch.cuda.synchronize()
        t_fit = time.perf_counter() - t0
        erq = ExtendedRaBitQuantizer(4)
        erq.fit(X)
        ec = erq.compress(X)
        hist = torch.bincount(torch.from_numpy(base.bits), minlength=9).tolist()
        print(f"# {n} x {d}: fit {t_fit:.2f} s (host and device, N(0,1) tables "
              f"{'cached' if shape != a.shapes[0] else 'computed'}), widths 0..8: {hist}, levels {sum(len(c) for c in base.cb)}")
        for packing in ("dense", "ffd"):
            q = repacked(base, packing)
            st = q._state()
            cs = q.code_size
            codes = q.compress(X)
            tc, te = alternate([lambda: q.compress(X), lambda: erq.compress(X)], a.reps, a.min_seconds)
            td, tf = alternate([lambda: q.decompress(codes), lambda: erq.decompress(ec)], a.reps, a.min_seconds)
            print(f"  {packing:5s} code_size {cs} (extrabitq {ec.shape[1]}), {tc[3]} calls each, alternated")
            print(f"    compress    rankaware {ms(tc)}   extrabitq {ms(te)}   ratio {tc[0] / te[0]:.3f}")
            print(f"    decompress  rankaware {ms(td)}   extrabitq {ms(tf)}   ratio {td[0] / tf[0]:.3f}")
            xc = _native.rankaware_center(X, st.mu)
            y = _native.gemm_f64(xc, st.V, False)
            yh = _native.rankaware_dequantize(codes, st)
            zz = _native.gemm_f64(yh, st.V, True)
            s = alternate([lambda: _native.rankaware_center(X, st.mu), lambda: _native.gemm_f64(xc, st.V, False),
                           lambda: _native.rankaware_quantize(y, st, out=codes),
                           lambda: _native.rankaware_dequantize(codes, st),
                           lambda: _native.gemm_f64(yh, st.V, True), lambda: _native.rankaware_finish(zz, st.mu)],
                          a.reps, a.min_seconds)
            qb = 8 * n * d + n * cs
            fl = 2.0 * n * d * d
            print(f"    center      {ms(s[0])}  {12 * n * d / s[0][0] / 1e9:8.1f} GB/s")
            print(f"    GEMM  x.V   {ms(s[1])}  {fl / s[1][0] / 1e12:8.2f} TFLOP/s fp64")
            print(f"    quantize    {ms(s[2])}  {qb / s[2][0] / 1e9:8.1f} GB/s  {qb / s[2][0] / HBM_PEAK:.3f} of 8 TB/s")
            print(f"    dequantize  {ms(s[3])}  {qb / s[3][0] / 1e9:8.1f} GB/s  {qb / s[3][0] / HBM_PEAK:.3f} of 8 TB/s")
            print(f"    GEMM  y.V^T {ms(s[4])}  {fl / s[4][0] / 1e12:8.2f} TFLOP/s fp64")
            print(f"    finish      {ms(s[5])}  {12 * n * d / s[5][0] / 1e9:8.1f} GB/s", flush=True)
            del xc, y, yh, zz, codes
            torch.cuda.empty_cache()
        del X, ec
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
