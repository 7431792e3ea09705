#!/usr/bin/env python3
"""A/B of the two flat searches over rank-aware codes, in one process on seeded data:

  (a) FlatQuantizedIndex   decode the whole database (dequantize, N x D x D fp64 GEMM, finish),
                           then mivq_flat_search on the fp32 rows
  (b) RankAwareFlatIndex   rotate the queries, mivq_rankaware_flat_search on the packed codes

Rows have the geometric spectrum of tools/rankaware_ab.py.  Per packing and batch size the two
indices (sharing one fit and one code array) are warmed up, then timed alternately with HIP
events around ``search_with_scores``; medians are reported with the range.  Also printed: the
recall@k of each against the exact fp32 search of the rows themselves, the mean overlap of the
two id lists, ``torch.cuda.max_memory_allocated`` of one call of each (above what is resident),
and the LVQ-4 code search (``mivq_lvq_flat_search``) at the same shape, whose rows are nearly
the same size.

  python tools/rankaware_search_ab.py                          # 1M x 1024, avg_bits 4
  python tools/rankaware_search_ab.py --n 65536 --d 256        # a smaller box
"""

from __future__ import annotations

import argparse
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "vector-quantization_amd"))

from haag_vq import _native  # noqa: E402
from haag_vq.methods.lvq_quantization import LVQQuantizer  # noqa: E402
from haag_vq.methods.rank_aware_quantization import RankAwareQuantizer  # noqa: E402
from haag_vq.methods.search.flat_quantized_index import (FlatQuantizedIndex, RankAwareFlatIndex,  # noqa: E402
                                                         search_codes)


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


def peak_of(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    return out, torch.cuda.max_memory_allocated() - base


def overlap(a, b) -> float:
    """Mean share of a row's ids that the other list has too."""
    return float(np.mean([len(np.intersect1d(x, y)) / len(x) for x, y in zip(a, b)]))


def repacked(q, packing):
    """The same fit with another packing (the layout is a function of `bits`)."""
    r = RankAwareQuantizer(q.avg_bits, alpha=q.alpha, max_bits=q.max_bits, seed=q.seed, packing=packing)
    r.mu, r.V, r.var, r.bits, r.cb, r.D, r._levels, r._Dg = q.mu, q.V, q.var, q.bits, q.cb, q.D, q._levels, q._Dg
    r._layout()
    return r


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--d", type=int, default=1024)
    ap.add_argument("--nq", type=int, nargs="+", default=[1, 100, 1000])
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--avg-bits", type=float, default=4.0)
    ap.add_argument("--alpha", type=float, default=0.5)
    ap.add_argument("--max-bits", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--min-seconds", type=float, default=0.3)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    dev = _native.require_device()
    n, d, k = a.n, a.d, a.k
    g = torch.Generator(device=dev).manual_seed(a.seed)
    print(f"# {torch.cuda.get_device_name(0)}  n={n} d={d} k={k} L2  avg_bits={a.avg_bits} alpha={a.alpha} "
          f"max_bits={a.max_bits}  kernels {_native.kernel_source_hash()}")
    std = 2.0 * 1e-2 ** (torch.arange(d, device=dev) / max(d - 1, 1))
    off = torch.randn(d, generator=g, device=dev)
    X = torch.randn((n, d), generator=g, device=dev) * std + off
    t0 = time.perf_counter()
    base = RankAwareQuantizer(a.avg_bits, alpha=a.alpha, max_bits=a.max_bits)
    base.fit(X)
    torch.cuda.synchronize()
    hist = torch.bincount(torch.from_numpy(base.bits), minlength=9).tolist()
    print(f"# fit {time.perf_counter() - t0:.1f} s, widths 0..8: {hist}, levels {sum(len(c) for c in base.cb)}")
    lvq = LVQQuantizer(num_bits=4)
    lvq.fit(X)
    lvq_codes = lvq.compress(X)
    queries = {nq: torch.randn((nq, d), generator=g, device=dev) * std + off for nq in a.nq}
    truth = {nq: _native.flat_search(Q, X, k)[1].cpu().numpy().view(np.uint32) for nq, Q in queries.items()}
    print(f"# LVQ-4 rows {lvq_codes.shape[1]} bytes")
    for packing in ("dense", "ffd"):
        q = repacked(base, packing)
        codes = q.compress(X)
        ia, ib = FlatQuantizedIndex(q), RankAwareFlatIndex(q)
        for idx in (ia, ib):
            idx._codes, idx._N, idx._D, idx._metric = codes, n, d, "l2"
        print(f"{packing}: code_size {q.code_size} bytes, {codes.numel() / 1e6:.0f} MB of codes")
        for nq, Q in queries.items():
            (ids_a, _), pk_a = peak_of(lambda: ia.search_with_scores(Q, k))
            (ids_b, _), pk_b = peak_of(lambda: ib.search_with_scores(Q, k))
            (_, ids_l), pk_l = peak_of(lambda: search_codes(lvq, lvq_codes, Q, k))
            ids_l = ids_l.cpu().numpy().view(np.uint32)
            ta, tb, tl = alternate([lambda: ia.search_with_scores(Q, k), lambda: ib.search_with_scores(Q, k),
                                    lambda: search_codes(lvq, lvq_codes, Q, k)], a.reps, a.min_seconds)
            tr = timed(lambda: q.rotate_queries(Q))
            path = "tiled" if nq >= 16 and n >= 4096 else "scan"
            print(f"  nq {nq:5d} ({path}), {ta[3]} calls each, alternated")
            print(f"    decode + flat_search  {ms(ta)}  {nq / ta[0]:10.1f} q/s  peak {pk_a / 1e6:9.1f} MB  "
                  f"recall@{k} {overlap(truth[nq], ids_a):.4f}")
            print(f"    code search           {ms(tb)}  {nq / tb[0]:10.1f} q/s  peak {pk_b / 1e6:9.1f} MB  "
                  f"recall@{k} {overlap(truth[nq], ids_b):.4f}  codes at {codes.numel() / tb[0] / 1e9:.1f} GB/s  "
                  f"(query rotation {tr * 1e3:.3f} ms)")
            print(f"    LVQ-4 code search     {ms(tl)}  {nq / tl[0]:10.1f} q/s  peak {pk_l / 1e6:9.1f} MB  "
                  f"recall@{k} {overlap(truth[nq], ids_l):.4f}")
            print(f"    decode / code {ta[0] / tb[0]:.2f}x   code / LVQ-4 {tb[0] / tl[0]:.2f}x   "
                  f"id overlap of the two rank-aware paths {overlap(ids_a, ids_b):.4f}", flush=True)
        del codes, ia, ib
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
