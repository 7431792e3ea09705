#!/usr/bin/env python3
"""IvfQuantizedIndex against the flat code search on the same clustered rows and queries, in one process.

The yardstick is the flat exact search over the codes of a globally fitted quantizer of the same
bits (FlatQuantizedIndex: every row for every query); the IVF index is never its own yardstick.
Both are fitted on the same seeded, clustered n x d rows (the IVF formats share one set of
coarse centroids) and searched with the same nq queries; ground truth is mivq_flat_search on the
f32 rows (exact L2).  Per leg the searches are warmed up, then timed alternately with HIP events
(device-resident queries and results); the median is reported with the range.  Per run:

  q/s           queries per second of the whole search (IVF: probe selection + scan)
  recall@k      against the f32 ground truth
  rows          the share of the n rows inside a query's probes (mean over the queries)
  pairs/s       (row, query) pairs scanned per second: the rows of the probed lists (flat: nq * n)
                over the time of the scan alone (IVF: mivq_ivf_*_search without the probe selection)

  python tools/ivf_quantized_ab.py                       # 1M x 1024, 1000 queries, nlist 1024
  python tools/ivf_quantized_ab.py --n 65536 --d 256 --nlist 64 --nprobe 1 8 64     # a smaller box
"""

from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "vector-quantization_amd"))
sys.path.insert(0, str(ROOT / "tools"))

from ivf_rabitq_ab import alternate, clustered, recall, timed  # noqa: E402


def quantizer(fmt: str):
    from haag_vq.methods.lvq_quantization import LVQQuantizer
    from haag_vq.methods.scalar_quantization import ScalarQuantizer

    kind, bits = fmt.split("-")
    if kind == "sq":
        return ScalarQuantizer(num_bits=int(bits))
    if kind == "lvq":
        return LVQQuantizer(num_bits=int(bits))
    raise SystemExit(f"unknown format {fmt!r}: sq-4/8/16 or lvq-1..8")


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--d", type=int, default=1024)
    ap.add_argument("--nq", type=int, default=1000)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--formats", nargs="+", default=["sq-8", "lvq-4", "lvq-8"])
    ap.add_argument("--nprobe", type=int, nargs="+", default=[1, 4, 16, 64, 256])
    ap.add_argument("--centres", type=int, default=4096, help="Gaussian centres of the data")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--json", type=str, default=None, help="also write the rows to this file")
    a = ap.parse_args()

    import torch

    from haag_vq import _native
    from haag_vq.methods._ivf import train_coarse
    from haag_vq.methods.search import FlatQuantizedIndex, IvfQuantizedIndex, search_codes

    dev = _native.require_device()
    print(f"# {torch.cuda.get_device_name(0)}  n={a.n} d={a.d} nq={a.nq} k={a.k} L2  {a.centres} centres  "
          f"nlist {a.nlist}  kernels {_native.kernel_source_hash()}")
    X, Q = clustered(a.n, a.d, a.nq, a.centres, a.seed, dev)
    gt = _native.flat_search(Q, X, a.k, _native.METRIC_L2)[1].long()
    coarse = None
    t_coarse = timed(lambda: None)
    rows = []
    for fmt in a.formats:
        ivf = IvfQuantizedIndex(lambda: quantizer(fmt), K=a.nlist, nprobe=a.nprobe[0])
        if coarse is None:
            holder = {}
            t_coarse = timed(lambda: holder.setdefault("c", train_coarse(X, a.nlist)))
            coarse = holder["c"]
        t_fit = timed(lambda: ivf.fit(X, "l2", centroids=coarse))
        eng = ivf._index
        sizes = (eng.lists.offsets[1:] - eng.lists.offsets[:-1]).float()
        flat = FlatQuantizedIndex(quantizer(fmt))
        t_flat = timed(lambda: flat.fit(X, "l2"))
        print(f"# {fmt}: coarse k-means {t_coarse:.2f} s (shared), ivf assign + per-list fit + encode + bucket sort "
              f"{t_fit:.2f} s, flat fit + encode {t_flat:.2f} s; lists: mean {sizes.mean():.0f}, min {int(sizes.min())}, "
              f"max {int(sizes.max())} rows; footprint ivf {ivf.memory_footprint() / 2**20:.1f} MiB, "
              f"flat {flat.memory_footprint() / 2**20:.1f} MiB")

        def flat_search():
            return search_codes(flat.quantizer, flat._codes, Q, a.k, "l2")

        r_flat = recall(flat_search()[1].long() & 0xFFFFFFFF, gt)
        print(f"# {'index':>20s} {'ms':>9s} {'q/s':>10s} {'recall@' + str(a.k):>10s} {'rows':>7s} {'Gpairs/s':>9s} {'vs flat':>8s}   split / range")
        for nprobe in a.nprobe:
            ivf.nprobe = nprobe
            pl = eng.probes(Q, nprobe)
            L = eng.lists
            pairs = int(sizes[pl.long()].sum())  # (row, query) pairs the scan evaluates (the flat search: nq * n)

            def probe():
                return eng.probes(Q, nprobe)

            def scan():
                return _native.ivf_code_search(eng.kind, Q, eng.coarse, pl, L.offsets, L.codes, L.ids, eng.params,
                                               eng.nbits, eng.metric, a.k)

            (tf, tf0, tf1, calls), (ti, ti0, ti1, _), (tp, _, _, _), (ts, _, _, _) = alternate(
                [flat_search, lambda: ivf.search_device(Q, a.k), probe, scan], a.reps, a.min_seconds)
            r_ivf = recall(ivf.search_device(Q, a.k)[1].long() & 0xFFFFFFFF, gt)
            if nprobe == a.nprobe[0]:
                print(f"  {fmt + ' flat':>20s} {tf * 1e3:9.3f} {a.nq / tf:10.1f} {r_flat:10.3f} {1.0:7.4f} "
                      f"{a.nq * a.n / tf / 1e9:9.2f} {'1.00':>8s}   ({tf0 * 1e3:.3f}..{tf1 * 1e3:.3f} ms, {calls} calls, "
                      f"alternated with the first ivf leg)")
            print(f"  {fmt + ' ivf nprobe ' + str(nprobe):>20s} {ti * 1e3:9.3f} {a.nq / ti:10.1f} {r_ivf:10.3f} "
                  f"{pairs / a.nq / a.n:7.4f} {pairs / ts / 1e9:9.2f} {tf / ti:8.2f}   probe selection {tp * 1e3:.3f} ms + "
                  f"scan {ts * 1e3:.3f} ms; ({ti0 * 1e3:.3f}..{ti1 * 1e3:.3f} ms, flat alongside {tf * 1e3:.3f} ms, "
                  f"{a.nq * a.n / tf / 1e9:.2f} Gpairs/s)", flush=True)
            rows.append(dict(format=fmt, nprobe=nprobe, ivf_ms=ti * 1e3, flat_ms=tf * 1e3, probe_ms=tp * 1e3,
                             scan_ms=ts * 1e3, pairs=pairs, recall_ivf=r_ivf, recall_flat=r_flat, calls=calls))
        del ivf, eng, flat
        torch.cuda.empty_cache()
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(rows, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
