#!/usr/bin/env python3
"""RaBitQIVFIndex against the flat RaBitQIndex on the same clustered rows and queries, in one process.

The yardstick is the flat estimator search (RaBitQIndex: every code for every query); the IVF
index is never its own yardstick.  Both are fitted on the same seeded, clustered n x d rows and
searched with the same nq queries; ground truth is mivq_flat_search (exact L2).  Per leg the
searches are warmed up, then timed alternately with HIP events (device-resident queries and
results); the median is reported with the range, and recall@k against the ground truth.

  flat      RaBitQIndex(qb)                              one centre, n codes per query
  ivf       RaBitQIVFIndex(nlist, nprobe, qb)            for every nprobe of --nprobe
            split per leg: the probe selection (pairwise_distances + topk_rows) and
            mivq_ivf_rabitq_search, timed separately with HIP events; and the share of the flat
            search's nq * n keys that the probed lists hold

The kernel split inside mivq_ivf_rabitq_search comes from a kernel trace taken in a run of its own:
  rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/ivf_rabitq_ab.py --trace-leg 64
  python tools/ivf_rabitq_ab.py --split DIR

  python tools/ivf_rabitq_ab.py                          # 1M x 1024, 1000 queries, nlist 1024
  python tools/ivf_rabitq_ab.py --n 65536 --d 256 --nlist 64 --nprobe 1 8 64     # a smaller box
"""

from __future__ import annotations

import argparse
import csv
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "vector-quantization_amd"))


def timed(fn):
    import torch

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3


def alternate(fns, reps, min_seconds):
    """Median / min / max seconds of each of `fns`, called in turn until each ran `reps` times
    and `min_seconds` in all."""
    import torch

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


def clustered(n, d, nq, centres, seed, dev):
    """n rows around `centres` Gaussian centres (sigma 0.3 per dimension), queries = rows + noise."""
    import torch

    g = torch.Generator(device=dev).manual_seed(seed)
    cen = torch.randn((centres, d), generator=g, device=dev)
    X = torch.empty((n, d), dtype=torch.float32, device=dev)
    for s in range(0, n, 1 << 18):
        e = min(n, s + (1 << 18))
        pick = torch.randint(0, centres, (e - s,), generator=g, device=dev)
        X[s:e] = cen[pick] + 0.3 * torch.randn((e - s, d), generator=g, device=dev)
    qi = torch.randint(0, n, (nq,), generator=g, device=dev)
    Q = (X[qi] + 0.05 * torch.randn((nq, d), generator=g, device=dev)).contiguous()
    return X, Q


def recall(ids, gt) -> float:
    """Mean share of the ground-truth ids found, per query (ids, gt: (nq, k) int64 on the device)."""
    hit = (ids[:, :, None] == gt[:, None, :]).any(dim=2).float().sum(dim=1) / gt.shape[1]
    return float(hit.mean())


def split(trace_dir: str) -> int:
    """Kernel time by name from the kernel-trace CSV(s) under trace_dir (steady state: the last
    half of each kernel's dispatches)."""
    files = sorted(Path(trace_dir).rglob("*kernel_trace.csv"))
    if not files:
        print(f"no *kernel_trace.csv under {trace_dir}")
        return 1
    per = {}
    for f in files:
        for r in csv.DictReader(open(f)):
            name = r["Kernel_Name"].replace("(anonymous namespace)::", "")
            per.setdefault(name, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    tot = {k: sum(v[len(v) // 2:]) for k, v in per.items()}
    whole = sum(tot.values())
    print(f"# kernel split ({sum(len(v) for v in per.values())} dispatches, last half of each kernel's): share of GPU time")
    for k, t in sorted(tot.items(), key=lambda kv: -kv[1])[:16]:
        v = per[k][len(per[k]) // 2:]
        print(f"  {100 * t / whole:5.1f} %  {t / len(v):10.1f} us x {len(v):4d}  {k[:110]}")
    return 0


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--d", type=int, default=1024)
    ap.add_argument("--nq", type=int, default=1000)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--qb", type=int, default=4)
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--nprobe", type=int, nargs="+", default=[1, 16, 64, 256])
    ap.add_argument("--centres", type=int, default=4096, help="Gaussian centres of the data")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--json", type=str, default=None, help="also write the rows to this file")
    ap.add_argument("--trace-leg", type=int, default=None, metavar="NPROBE",
                    help="only fit the IVF index and run this leg's search a few times (for a kernel trace)")
    ap.add_argument("--split", type=str, default=None, metavar="DIR", help="summarise a kernel trace and exit")
    a = ap.parse_args()
    if a.split:
        return split(a.split)

    import torch

    from haag_vq import _native
    from haag_vq.methods.search import RaBitQIndex, RaBitQIVFIndex

    dev = _native.require_device()
    print(f"# {torch.cuda.get_device_name(0)}  n={a.n} d={a.d} nq={a.nq} k={a.k} qb={a.qb} L2  "
          f"{a.centres} centres  kernels {_native.kernel_source_hash()}")
    X, Q = clustered(a.n, a.d, a.nq, a.centres, a.seed, dev)
    ivf = RaBitQIVFIndex(nlist=a.nlist, nprobe=a.nprobe[0], qb=a.qb)
    t_fit = timed(lambda: ivf.fit(X, "l2"))
    eng = ivf._index
    sizes = (eng.lists.offsets[1:] - eng.lists.offsets[:-1]).float()
    print(f"# ivf fit {t_fit:.2f} s (coarse k-means + assign + encode + bucket sort); lists: mean {sizes.mean():.0f}, "
          f"min {int(sizes.min())}, max {int(sizes.max())} rows")
    if a.trace_leg is not None:
        ivf.nprobe = a.trace_leg
        for _ in range(6):
            ivf.search_device(Q, a.k)
        torch.cuda.synchronize()
        return 0

    gt = _native.flat_search(Q, X, a.k, _native.METRIC_L2)[1].long()
    flat = RaBitQIndex(qb=a.qb)
    t_fit = timed(lambda: flat.fit(X, "l2"))
    print(f"# flat fit {t_fit:.2f} s")
    del X
    torch.cuda.empty_cache()
    rows = []
    r_flat = recall(flat.search_device(Q, a.k)[1].long() & 0xFFFFFFFF, gt)
    print(f"# {'index':>14s} {'ms':>9s} {'q/s':>10s} {'recall@' + str(a.k):>10s} {'vs flat':>8s}   split / range")
    for nprobe in a.nprobe:
        ivf.nprobe = nprobe
        npc = max(1, min(nprobe, a.nlist))

        def probe():
            return _native.topk_rows(_native.pairwise_distances(Q, eng.coarse, eng.metric), npc)[1]

        pl = probe()
        L = eng.lists
        # (query, code) keys the scan evaluates: the rows of every probed list (the flat search: nq * n)
        keys = int(sizes[pl.long()].sum())

        def scan():
            return _native.ivf_rabitq_search(Q, eng.coarse, pl, L.offsets, L.codes, L.ids, a.qb, eng.metric, a.k)

        (tf, tf0, tf1, calls), (ti, ti0, ti1, _), (tp, _, _, _), (ts, _, _, _) = alternate(
            [lambda: flat.search_device(Q, a.k), lambda: ivf.search_device(Q, a.k), probe, scan], a.reps, a.min_seconds)
        r_ivf = recall(ivf.search_device(Q, a.k)[1].long() & 0xFFFFFFFF, gt)
        if nprobe == a.nprobe[0]:
            print(f"  {'flat':>14s} {tf * 1e3:9.3f} {a.nq / tf:10.1f} {r_flat:10.3f} {'1.00':>8s}   "
                  f"({tf0 * 1e3:.3f}..{tf1 * 1e3:.3f} ms, {calls} calls, alternated with the first ivf leg)")
        print(f"  {'ivf nprobe ' + str(nprobe):>14s} {ti * 1e3:9.3f} {a.nq / ti:10.1f} {r_ivf:10.3f} {tf / ti:8.2f}   "
              f"probe selection {tp * 1e3:.3f} ms + ivf_rabitq_search {ts * 1e3:.3f} ms; {keys / a.nq / a.n:.4f} of the "
              f"flat search's keys; ({ti0 * 1e3:.3f}..{ti1 * 1e3:.3f} ms, flat alongside {tf * 1e3:.3f} ms)", flush=True)
        rows.append(dict(nprobe=nprobe, ivf_ms=ti * 1e3, flat_ms=tf * 1e3, probe_ms=tp * 1e3, scan_ms=ts * 1e3, keys=keys,
                         recall_ivf=r_ivf, recall_flat=r_flat, calls=calls))
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(rows, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
