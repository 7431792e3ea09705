#!/usr/bin/env python3
"""LVQ-8 against the SQ-8 kernels of the same shapes, in one process on seeded data.

The yardsticks are SQ-8's entry points (and, for one query, the decode path the code search
replaces); LVQ is never its own yardstick.  Per leg the two sides are warmed up, then timed
alternately with HIP events; the median is reported with the range.

  encode   mivq_lvq_encode (nbits 8)  vs  mivq_sq_encode_f32 (nbits 8), n x d rows: both read
           4 n d bytes and write n d (+ 8 n) bytes; printed with the share of 8 TB/s those
           algorithmic bytes make of the time
  mean     mivq_column_mean on the same rows (LVQ's fit; no yardstick: torch's mean sums in
           another order), against the 4 n d bytes it reads
  search   mivq_lvq_flat_search (nbits 8)  vs  mivq_sq_flat_search (nbits 8), k = 10, L2, on
           random codes; for the first nq also lvq_decode + flat_search, whose ids and distance
           bits must equal the code search's (it holds a 4 n d byte temporary)

  python tools/lvq_ab.py                                  # 1M x 1536 encode, 1M x 3072 search
  python tools/lvq_ab.py --n 65536 --d-encode 256 --d-search 256 --nq 1 100   # a smaller box
"""

from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "vector-quantization_amd"))

from haag_vq import _native  # noqa: E402

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


def same(a, b) -> bool:
    return torch.equal(a[1], b[1]) and torch.equal(a[0].view(torch.int32), b[0].view(torch.int32))


def lvq_codes(n, d, dev, g):
    codes = torch.randint(0, 256, (n, d + 8), generator=g, device=dev, dtype=torch.uint8)
    tail = torch.stack([torch.randn(n, generator=g, device=dev), (torch.rand(n, generator=g, device=dev) + 0.5) / 255],
                       dim=1)
    codes[:, d:] = tail.contiguous().view(torch.uint8).view(n, 8)
    return codes


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--d-encode", type=int, default=1536)
    ap.add_argument("--d-search", type=int, default=3072)
    ap.add_argument("--nq", type=int, nargs="+", default=[1, 100, 1000])
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--json", type=str, default=None, help="also write the rows to this file")
    a = ap.parse_args()
    dev = _native.require_device()
    g = torch.Generator(device=dev).manual_seed(a.seed)
    rows, ok = [], True
    print(f"# {torch.cuda.get_device_name(0)}  n={a.n} k={a.k} L2  kernels {_native.kernel_source_hash()}")

    # ---- encode and fit
    n, d = a.n, a.d_encode
    X = torch.randn((n, d), generator=g, device=dev) * (torch.rand(d, generator=g, device=dev) * 2.8 + 0.2)
    mu = _native.column_mean(X)
    lo = X.amin(dim=0)
    den = (X.amax(dim=0) - lo) + 1e-8
    out_l = torch.empty((n, _native.lvq_code_size(d, 8)), dtype=torch.uint8, device=dev)
    (tl, tl0, tl1, calls), (ts, ts0, ts1, _), (tm, tm0, tm1, _) = alternate(
        [lambda: _native.lvq_encode(X, mu, 8, out=out_l), lambda: _native.sq_encode(X, lo, den, 8),
         lambda: _native.column_mean(X)], a.reps, a.min_seconds)
    bl, bs, bm = 4 * n * d + out_l.numel(), 4 * n * d + n * d, 4 * n * d
    print(f"# encode {n} x {d}, nbits 8 ({calls} calls each, alternated)")
    print(f"  lvq_encode      {tl * 1e3:9.3f} ms ({tl0 * 1e3:.3f}..{tl1 * 1e3:.3f})  {bl / tl / 1e9:8.1f} GB/s  "
          f"{bl / tl / HBM_PEAK:.3f} of 8 TB/s")
    print(f"  sq_encode_f32   {ts * 1e3:9.3f} ms ({ts0 * 1e3:.3f}..{ts1 * 1e3:.3f})  {bs / ts / 1e9:8.1f} GB/s  "
          f"{bs / ts / HBM_PEAK:.3f} of 8 TB/s   lvq / sq time {tl / ts:.2f}")
    print(f"  column_mean     {tm * 1e3:9.3f} ms ({tm0 * 1e3:.3f}..{tm1 * 1e3:.3f})  {bm / tm / 1e9:8.1f} GB/s  "
          f"{bm / tm / HBM_PEAK:.3f} of 8 TB/s")
    rows.append(dict(leg="encode", n=n, d=d, lvq_ms=tl * 1e3, sq_ms=ts * 1e3, lvq_frac=bl / tl / HBM_PEAK,
                     sq_frac=bs / ts / HBM_PEAK, mean_ms=tm * 1e3, mean_frac=bm / tm / HBM_PEAK, calls=calls))
    del X, out_l
    torch.cuda.empty_cache()

    # ---- search
    d = a.d_search
    cl = lvq_codes(n, d, dev, g)
    csq = torch.randint(0, 256, (n, d), generator=g, device=dev, dtype=torch.uint8)
    mu = torch.randn(d, generator=g, device=dev)
    lo = torch.randn(d, generator=g, device=dev)
    den = torch.rand(d, generator=g, device=dev) + 0.5
    print(f"# search {n} x {d}, nbits 8, k={a.k}: code bytes lvq {cl.numel()}, sq {csq.numel()}")
    print(f"# {'nq':>5s} {'path':>6s} {'lvq ms':>9s} {'sq ms':>9s} {'lvq/sq':>7s} {'lvq q/s':>10s} {'sq q/s':>10s} "
          f"{'lvq code GB/s':>14s}")
    for j, nq in enumerate(a.nq):
        Q = torch.randn((nq, d), generator=g, device=dev)
        fl = lambda: _native.lvq_flat_search(Q, cl, mu, 8, a.k, _native.METRIC_L2)  # noqa: E731
        fs = lambda: _native.sq_flat_search(Q, csq, d, lo, den, 8, a.k, _native.METRIC_L2)  # noqa: E731
        (tl, tl0, tl1, calls), (ts, ts0, ts1, _) = alternate([fl, fs], a.reps, a.min_seconds)
        tiled = nq >= 16 and n >= 4096
        print(f"  {nq:5d} {'tiled' if tiled else 'scan':>6s} {tl * 1e3:9.3f} {ts * 1e3:9.3f} {tl / ts:7.2f} "
              f"{nq / tl:10.1f} {nq / ts:10.1f} {cl.numel() / tl / 1e9:14.1f}   (lvq {tl0 * 1e3:.3f}..{tl1 * 1e3:.3f} ms, "
              f"sq {ts0 * 1e3:.3f}..{ts1 * 1e3:.3f} ms, {calls} calls each)", flush=True)
        row = dict(leg="search", n=n, d=d, nq=nq, path="tiled" if tiled else "scan", lvq_ms=tl * 1e3, sq_ms=ts * 1e3,
                   calls=calls)
        if j == 0:  # the path the code search replaces
            fd = lambda: _native.flat_search(Q, _native.lvq_decode(cl, mu, 8), a.k, _native.METRIC_L2)  # noqa: E731
            identical = same(fl(), fd())
            ok = ok and identical
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            fd()
            torch.cuda.synchronize()
            peak = torch.cuda.max_memory_allocated() - base
            (tc, _, _, _), (td, td0, td1, c2) = alternate([fl, fd], a.reps, a.min_seconds)
            print(f"        nq={nq}: lvq_decode + flat_search {td * 1e3:9.3f} ms ({td0 * 1e3:.3f}..{td1 * 1e3:.3f}, "
                  f"{c2} calls, peak {peak / 1e9:.2f} GB) vs code search {tc * 1e3:.3f} ms: {td / tc:.2f}x, results "
                  f"{'identical' if identical else 'DIFFERENT'}", flush=True)
            row.update(decode_ms=td * 1e3, decode_peak=peak, same=bool(identical))
        rows.append(row)
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(rows, indent=1))
    print("# all results identical" if ok else "# RESULTS DIFFER")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
