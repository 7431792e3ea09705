#!/usr/bin/env python3
"""RankAwareQuantizer with its three codebooks on the same clustered rows, in one process:

  gaussian   analytic N(0,1) tables scaled by sqrt(var_d)                     (codebook="gaussian")
  lloyd      k-means++ / Lloyd on the projected sample, mivq_codebook1d_fit    (codebook_engine="device")
  exact      the optimal 1-D k-means on the same sample, mivq_codebook1d_fit   (codebook_engine="device")

The moments, eigh and the bit allocation are shared (they do not depend on the codebook), so one
fit supplies mu, V and bits and each stage is timed on its own:

  moments, eigh        RankAwareQuantizer._moments (device) and numpy's eigh (host)
  projection, sort     the sample's (x - mu) V rounded to f32 and transposed; torch.sort of the columns
  codebooks            mivq_codebook1d_fit: one warm-up call, then --reps calls, median and range;
                       a call that takes more than --long seconds is not repeated
  prefix / seeding /   the call's kernels by name from a torch.profiler run of one more call
  passes / DP          (device time; "not measured" when the profiler reports no kernels)

Then per codebook, with ffd packing: reconstruction MSE of all rows, recall@k of RankAwareFlatIndex
against mivq_flat_search on the rows, and the workspace the fit asked for.  A last section times
mivq_codebook1d_fit alone on 1 and 64 sorted N(0,1) columns of 200 000 values at --widths, the
shape of one-column CPU figures.

  python tools/codebook_fit_ab.py                       # 1M x 1024 and 200k x 1024, avg_bits 4
  python tools/codebook_fit_ab.py --n 20000 --d 128     # a smaller box
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
sys.path.insert(0, str(Path(__file__).resolve().parent))

from haag_vq import _native  # noqa: E402
from haag_vq.methods import rank_aware_quantization as raq  # noqa: E402
from haag_vq.methods.search.flat_quantized_index import RankAwareFlatIndex  # noqa: E402
from ivf_rabitq_ab import clustered, recall, timed  # noqa: E402

STAGES = {"cb1d_prefix_kernel": "prefix", "cb1d_seed_kernel": "seeding", "cb1d_lloyd_kernel": "passes",
          "cb1d_exact_kernel": "DP"}


def spread(ts) -> str:
    ts = sorted(ts)
    return f"{ts[len(ts) // 2] * 1e3:10.2f} ms ({ts[0] * 1e3:.2f}..{ts[-1] * 1e3:.2f}, {len(ts)} calls)"


def kernel_split(fn) -> dict:
    """Device seconds per stage of one call of fn, from torch.profiler; {} when it sees no kernel."""
    try:
        from torch.profiler import ProfilerActivity, profile

        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        out = {}
        for e in prof.key_averages():
            for k, stage in STAGES.items():
                if k in e.key:
                    us = getattr(e, "device_time_total", None) or getattr(e, "cuda_time_total", 0.0)
                    out[stage] = out.get(stage, 0.0) + us * 1e-6
        return out
    except Exception as exc:  # the profiler is an extra: the timings above do not depend on it
        print(f"    (profiler unavailable: {type(exc).__name__}: {exc})")
        return {}


def with_tables(base, cb, codebook):
    q = raq.RankAwareQuantizer(base.avg_bits, alpha=base.alpha, max_bits=base.max_bits, packing=base.packing,
                               codebook=codebook, codebook_engine="saq" if codebook == "gaussian" else "device")
    q.mu, q.V, q.var, q.bits, q.D, q._levels, q._Dg, q.cb = base.mu, base.V, base.var, base.bits, base.D, base._levels, \
        base._Dg, cb
    q._layout()
    return q


def run(n, a, dev) -> None:
    d, k = a.d, a.k
    X, Q = clustered(n, d, a.nq, a.centres, a.seed, dev)
    truth = _native.flat_search(Q, X, k)[1].to(torch.int64)
    print(f"\n## n={n} d={d}  avg_bits={a.avg_bits} alpha={a.alpha} max_bits={a.max_bits} packing=ffd  "
          f"{a.centres} centres, {a.nq} queries, k={k}")
    base = raq.RankAwareQuantizer(a.avg_bits, alpha=a.alpha, max_bits=a.max_bits, packing="ffd")
    base.fit(X)    # warm-up of the moments' kernels; fills the N(0,1) table cache
    t_mom = [timed(lambda: base._moments(X)) for _ in range(a.reps)]
    N, S, G = base._moments(X)
    t0 = time.perf_counter()
    np.linalg.eigh(G / N - np.outer(S / N, S / N))
    t_eigh = time.perf_counter() - t0
    hist = np.bincount(base.bits, minlength=9).tolist()
    print(f"  shared: moments {spread(t_mom)}  eigh (host, one call) {t_eigh:.3f} s  widths 0..8: {hist}")
    base._sample_projection(X)
    t_proj = [timed(lambda: base._sample_projection(X)) for _ in range(a.reps)]
    unsorted = base._sample_projection(X)
    torch.sort(unsorted, dim=1)
    t_sort = [timed(lambda: torch.sort(unsorted, dim=1)) for _ in range(a.reps)]
    cols = torch.sort(unsorted, dim=1).values.contiguous()
    del unsorted
    ns = cols.shape[1]
    print(f"  sample {ns} rows: projection {spread(t_proj)}  sort {spread(t_sort)}")

    tables = {"gaussian": base.cb}
    for method in ("lloyd", "exact"):
        ws_bytes, at_once = _native.codebook1d_workspace(ns, base.bits, method, dev)   # what the call allocates
        slot = ws_bytes // at_once
        call = lambda: _native.codebook1d_fit(cols, base.bits, method)  # noqa: E731
        first = timed(call)
        ts = [first] if first > a.long else [timed(call) for _ in range(a.reps)]
        note = f"  first call {first * 1e3:.2f} ms" + ("  (long: not repeated)" if first > a.long else "")
        print(f"  {method:8s} codebooks {spread(ts)}{note}")
        print(f"           workspace {ws_bytes / 2 ** 30:.2f} GiB = {at_once} slots of {slot / 2 ** 20:.1f} MiB "
              f"at the widest dimension ({int(base.bits.max())} bits), {int(np.count_nonzero(base.bits))} dimensions to fit")
        if first <= a.long:
            split = kernel_split(call)
            print("           kernels: " + ("  ".join(f"{s} {t * 1e3:.2f} ms" for s, t in split.items()) if split
                                            else "not measured"))
        else:
            print("           kernels: not measured (long call)")
        levels, lv_off, _ = call()
        lv = levels.cpu().numpy().astype(np.float64)
        tables[method] = [lv[lv_off[j]:lv_off[j + 1]] if b else np.array([0.0]) for j, b in enumerate(base.bits)]

    print(f"  {'':8s} {'mse':>12s} {'recall@' + str(k):>10s}  code_size")
    for name, cb in tables.items():
        q = with_tables(base, cb, name)
        codes = q.compress(X)
        se, rows = 0.0, 0
        for s in range(0, n, 1 << 17):
            xh = q.decompress(codes[s:s + (1 << 17)].contiguous())
            se += float(((xh - X[s:s + (1 << 17)]) ** 2).sum(dtype=torch.float64))
            rows += xh.shape[0]
        idx = RankAwareFlatIndex(q)
        idx._codes, idx._N, idx._D, idx._metric = codes, n, d, "l2"
        ids = torch.from_numpy(idx.search(Q, k).astype(np.int64)).to(dev)
        print(f"  {name:8s} {se / (rows * d):12.6e} {recall(ids, truth):10.4f}  {q.code_size}", flush=True)
        del codes, idx
    del X, Q, cols
    torch.cuda.empty_cache()


def normal_columns(a, dev) -> None:
    """mivq_codebook1d_fit alone on sorted N(0,1) columns of the sample cap's length, every column at
    one width: one column (what a CPU builder's one-column time compares with) and 64."""
    n = raq.CB_SAMPLE
    g = torch.Generator(device=dev).manual_seed(a.seed + 1)
    print(f"\n## N(0,1) columns of {n} values, one width per call (median of {a.reps} calls after a warm-up)")
    for w in a.widths:
        for d in (1, 64):
            cols = torch.sort(torch.randn((d, n), generator=g, device=dev), dim=1).values.contiguous()
            line = f"  {w} bits, {d:2d} column{'s' if d > 1 else ' '}:"
            for method in ("lloyd", "exact"):
                call = lambda: _native.codebook1d_fit(cols, [w] * d, method)  # noqa: E731
                first = timed(call)
                ts = [first] if first > a.long else [timed(call) for _ in range(a.reps)]
                line += f"  {method} {spread(ts)}"
            print(line, flush=True)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, nargs="+", default=[1_000_000, 200_000])
    ap.add_argument("--d", type=int, default=1024)
    ap.add_argument("--nq", type=int, default=1000)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--centres", type=int, default=1024)
    ap.add_argument("--avg-bits", type=float, default=4.0)
    ap.add_argument("--alpha", type=float, default=0.5)
    ap.add_argument("--max-bits", type=int, default=8)
    ap.add_argument("--widths", type=int, nargs="*", default=[4, 8], help="widths of the N(0,1) column section")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--long", type=float, default=60.0, help="seconds above which a codebook call is not repeated")
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    dev = _native.require_device()
    print(f"# {torch.cuda.get_device_name(0)}  kernels {_native.kernel_source_hash()}  "
          f"sample cap {raq.CB_SAMPLE} rows, workspace budget {_native.CB1D_WORKSPACE_BUDGET / 2 ** 30:.0f} GiB")
    for n in a.n:
        run(n, a, dev)
    normal_columns(a, dev)
    return 0


if __name__ == "__main__":
    sys.exit(main())
