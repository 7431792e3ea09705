#!/usr/bin/env python3
"""A/B of the flat searches over Extended RaBitQ codes, in one process on seeded data:

  (a) FlatQuantizedIndex        decode the whole database (dequantize, N x D x D fp64 GEMM, finish),
                                then mivq_flat_search on the fp32 rows
  (b) ExtendedRaBitQFlatIndex   rotate the queries, mivq_extrabitq_flat_search on the packed codes
  (c) mivq_lvq_flat_search      LVQ codes of the same rows at the same B: the same row bytes and
                                the same reader, another dequantisation -- the yardstick of the scan

Per B and batch size the three (a and b sharing one fit and one code array) are warmed up, then
timed alternately with HIP events around ``search_with_scores`` / ``search_codes``; medians are
reported with the range.  Also printed: the recall@k of each against the exact fp32 search of
the rows themselves, whether the two Extended RaBitQ paths return the same ids, and
``torch.cuda.max_memory_allocated`` of one call of each (above what is resident).

  python tools/extrabitq_search_ab.py                          # 1M x 1024: B = 4 at nq 1, 100, 1000; B = 1, 8 at nq 1, 1000
  python tools/extrabitq_search_ab.py --n 65536 --d 256        # a smaller box
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
from haag_vq.methods.extended_rabitq import ExtendedRaBitQuantizer  # noqa: E402
from haag_vq.methods.lvq_quantization import LVQQuantizer  # noqa: E402
from haag_vq.methods.search.flat_quantized_index import (ExtendedRaBitQFlatIndex, FlatQuantizedIndex,  # noqa: E402
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


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--d", type=int, default=1024)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--plan", type=str, default="4:1,100,1000 1:1,1000 8:1,1000",
                    help="space-separated B:nq,nq,... legs")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--min-seconds", type=float, default=0.3)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    plan = [(int(leg.split(":")[0]), [int(v) for v in leg.split(":")[1].split(",")]) for leg in a.plan.split()]
    dev = _native.require_device()
    n, d, k = a.n, a.d, a.k
    g = torch.Generator(device=dev).manual_seed(a.seed)
    print(f"# {torch.cuda.get_device_name(0)}  n={n} d={d} k={k} L2  plan {a.plan!r}  "
          f"kernels {_native.kernel_source_hash()}")
    std = 0.5 + 1.5 * torch.rand(d, generator=g, device=dev)
    off = torch.randn(d, generator=g, device=dev)
    X = torch.randn((n, d), generator=g, device=dev) * std + off
    queries = {nq: torch.randn((nq, d), generator=g, device=dev) * std + off for nq in sorted({v for _, nqs in plan for v in nqs})}
    truth = {nq: _native.flat_search(Q, X, k)[1].cpu().numpy().view(np.uint32) for nq, Q in queries.items()}
    for B, nqs in plan:
        t0 = time.perf_counter()
        q = ExtendedRaBitQuantizer(num_bits=B, seed=a.seed)
        q.fit(X)
        codes = q.compress(X)
        lvq = LVQQuantizer(num_bits=B)
        lvq.fit(X)
        lvq_codes = lvq.compress(X)
        torch.cuda.synchronize()
        ia, ib = FlatQuantizedIndex(q), ExtendedRaBitQFlatIndex(q)
        for idx in (ia, ib):
            idx._codes, idx._N, idx._D, idx._metric = codes, n, d, "l2"
        print(f"B = {B}: code_size {q.code_size} bytes ({codes.numel() / 1e6:.0f} MB of codes), LVQ-{B} rows "
              f"{lvq_codes.shape[1]} bytes; fit + encode of both {time.perf_counter() - t0:.1f} s")
        for nq in nqs:
            Q = queries[nq]
            (ids_a, _), pk_a = peak_of(lambda: ia.search_with_scores(Q, k))
            (ids_b, _), pk_b = peak_of(lambda: ib.search_with_scores(Q, k))
            (_, ids_l), pk_l = peak_of(lambda: search_codes(lvq, lvq_codes, Q, k))
            ids_l = ids_l.cpu().numpy().view(np.uint32)
            ta, tb, tl = alternate([lambda: ia.search_with_scores(Q, k), lambda: ib.search_with_scores(Q, k),
                                    lambda: search_codes(lvq, lvq_codes, Q, k)], a.reps, a.min_seconds)
            tr = timed(lambda: q.rotate_queries(Q))
            path = "tiled" if nq >= 16 and n >= 4096 else "scan"
            print(f"  B {B} nq {nq:5d} ({path}), {ta[3]} calls each, alternated")
            print(f"    decode + flat_search  {ms(ta)}  {nq / ta[0]:10.1f} q/s  peak {pk_a / 1e6:9.1f} MB  "
                  f"recall@{k} {overlap(truth[nq], ids_a):.4f}")
            print(f"    code search           {ms(tb)}  {nq / tb[0]:10.1f} q/s  peak {pk_b / 1e6:9.1f} MB  "
                  f"recall@{k} {overlap(truth[nq], ids_b):.4f}  codes at {codes.numel() / tb[0] / 1e9:.1f} GB/s  "
                  f"(query rotation {tr * 1e3:.3f} ms)")
            print(f"    LVQ-{B} code search     {ms(tl)}  {nq / tl[0]:10.1f} q/s  peak {pk_l / 1e6:9.1f} MB  "
                  f"recall@{k} {overlap(truth[nq], ids_l):.4f}")
            print(f"    decode / code {ta[0] / tb[0]:.2f}x   code / LVQ-{B} {tb[0] / tl[0]:.2f}x   "
                  f"ids of the two Extended RaBitQ paths: identical {bool(np.array_equal(ids_a, ids_b))}, "
                  f"equal positions {float(np.mean(ids_a == ids_b)):.4f}, overlap {overlap(ids_a, ids_b):.4f}", flush=True)
        del codes, lvq_codes, ia, ib
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
