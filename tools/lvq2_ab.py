#!/usr/bin/env python3
"""Two-level LVQ (LVQ-4x4, LVQ-4x8) against the single-level paths it replaces, in one process.

The yardsticks are the single-level entry points and RefinedIndex; the two-level code is never
its own yardstick.  Per leg the sides are warmed up, then timed alternately with HIP events; the
median is reported with the range.

  encode   mivq_lvq2_encode (4,4) and (4,8)  vs  mivq_lvq_encode at B = 8, and vs the B = 4 plus
           B = 8 pair of calls RefinedIndex pays for its two stores; n x d-encode seeded rows.
           Printed with the share of 8 TB/s the algorithmic bytes (4 n d read, both rows
           written) make of the time.
  rerank   mivq_rerank_lvq2 (4,4) and (4,8)  vs  mivq_rerank_lvq at B = 8, on the same candidate
           lists (the LVQ-4 scan's top r), r = 10 / 40 / 100 / 250; the two-level calls read 1.0x
           and 1.5x the candidate bytes of the B = 8 call.  Clustered n x d rows, nq queries.
  index    LVQ2Index(4, 4 | 8, f)  vs  RefinedIndex(FlatQuantizedIndex(LVQQuantizer(4)),
           LVQQuantizer(8), f), f = 1 / 4 / 10 / 25: recall@k against the exact f32 search,
           queries per second of search_with_scores (device queries in, host results out),
           index bytes.

  python tools/lvq2_ab.py                                   # 1M x 1536 encode, 1M x 1024 search
  python tools/lvq2_ab.py --n 65536 --d 256 --d-encode 256 --nq 100 --centres 256    # a smaller box
"""

from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "vector-quantization_amd"))
sys.path.insert(0, str(ROOT / "tools"))

from ivf_rabitq_ab import alternate, clustered, recall  # noqa: E402

HBM_PEAK = 8.0e12


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--d", type=int, default=1024)
    ap.add_argument("--d-encode", type=int, default=1536)
    ap.add_argument("--nq", type=int, default=1000)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--r", type=int, nargs="+", default=[10, 40, 100, 250])
    ap.add_argument("--factor", type=int, nargs="+", default=[1, 4, 10, 25])
    ap.add_argument("--centres", type=int, default=4096, help="Gaussian centres of the data")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--min-seconds", type=float, default=0.3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--json", type=str, default=None, help="also write the rows to this file")
    a = ap.parse_args()

    import torch

    from haag_vq import _native
    from haag_vq.methods.lvq_quantization import LVQQuantizer
    from haag_vq.methods.search import FlatQuantizedIndex, LVQ2Index, RefinedIndex

    dev = _native.require_device()
    L2 = _native.METRIC_L2
    rows_out = []
    print(f"# {torch.cuda.get_device_name(0)}  n={a.n} k={a.k} L2  kernels {_native.kernel_source_hash()}")

    def ms(t):
        return f"{t[0] * 1e3:9.3f} ms ({t[1] * 1e3:.3f}..{t[2] * 1e3:.3f})"

    # ---- encode
    n, d = a.n, a.d_encode
    g = torch.Generator(device=dev).manual_seed(a.seed)
    X = torch.randn((n, d), generator=g, device=dev) * (torch.rand(d, generator=g, device=dev) * 2.8 + 0.2)
    mu = _native.column_mean(X)
    o8 = torch.empty((n, _native.lvq_code_size(d, 8)), dtype=torch.uint8, device=dev)
    o4 = torch.empty((n, _native.lvq_code_size(d, 4)), dtype=torch.uint8, device=dev)
    o2 = {b2: torch.empty((n, _native.lvq2_code_sizes(d, 4, b2)[1]), dtype=torch.uint8, device=dev) for b2 in (4, 8)}

    def pair():
        _native.lvq_encode(X, mu, 4, out=o4)
        _native.lvq_encode(X, mu, 8, out=o8)

    t44, t48, t8, tp = alternate([lambda: _native.lvq2_encode(X, mu, 4, 4, out1=o4, out2=o2[4]),
                                  lambda: _native.lvq2_encode(X, mu, 4, 8, out1=o4, out2=o2[8]),
                                  lambda: _native.lvq_encode(X, mu, 8, out=o8), pair], a.reps, a.min_seconds)
    same1 = torch.equal(_native.lvq2_encode(X, mu, 4, 8)[0], _native.lvq_encode(X, mu, 4))
    byt = {"44": 4 * n * d + o4.numel() + o2[4].numel(), "48": 4 * n * d + o4.numel() + o2[8].numel(),
           "8": 4 * n * d + o8.numel(), "pair": 8 * n * d + o4.numel() + o8.numel()}
    print(f"# encode {n} x {d} ({t44[3]} calls each, alternated); codes1 equal to lvq_encode(4): {same1}")
    for nm, t, b in (("lvq2_encode 4x4", t44, byt["44"]), ("lvq2_encode 4x8", t48, byt["48"]), ("lvq_encode 8", t8, byt["8"]),
                     ("lvq_encode 4 + 8", tp, byt["pair"])):
        print(f"  {nm:18s} {ms(t)}  {b / t[0] / 1e9:8.1f} GB/s  {b / t[0] / HBM_PEAK:.3f} of 8 TB/s   "
              f"x{t[0] / t8[0]:.2f} of lvq_encode 8, x{t[0] / tp[0]:.2f} of the 4 + 8 pair")
    rows_out.append(dict(leg="encode", n=n, d=d, lvq2_44_ms=t44[0] * 1e3, lvq2_48_ms=t48[0] * 1e3, lvq8_ms=t8[0] * 1e3,
                         pair_ms=tp[0] * 1e3, frac_44=byt["44"] / t44[0] / HBM_PEAK, frac_48=byt["48"] / t48[0] / HBM_PEAK,
                         frac_8=byt["8"] / t8[0] / HBM_PEAK, codes1_same=bool(same1), calls=t44[3]))
    del X, o8, o4, o2
    torch.cuda.empty_cache()

    # ---- the search data
    d = a.d
    X, Q = clustered(a.n, d, a.nq, a.centres, a.seed, dev)
    gt = _native.flat_search(Q, X, a.k, L2)[1].long()
    mu = _native.column_mean(X)
    c1, c28 = _native.lvq2_encode(X, mu, 4, 8)
    _, c24 = _native.lvq2_encode(X, mu, 4, 4)
    c8 = _native.lvq_encode(X, mu, 8)
    print(f"# search data {a.n} x {d}, {a.centres} centres, nq={a.nq}: LVQ-4 rows {c1.numel() / 2**20:.0f} MiB, residual "
          f"4 / 8 bits {c24.numel() / 2**20:.0f} / {c28.numel() / 2**20:.0f} MiB, LVQ-8 rows {c8.numel() / 2**20:.0f} MiB")

    # ---- the re-rank call alone
    print(f"# {'r':>5s} {'lvq2 4x4 ms':>28s} {'lvq2 4x8 ms':>28s} {'lvq 8 ms':>28s}  4x4/8  4x8/8   recall@{a.k} 4x4 / 4x8 / 8")
    for r in a.r:
        r = min(r, a.n, 256)
        cand = _native.lvq_flat_search(Q, c1, mu, 4, r, L2)[1].contiguous()
        f44 = lambda: _native.rerank_lvq2(Q, cand, c1, c24, mu, 4, 4, min(a.k, r), L2)  # noqa: E731
        f48 = lambda: _native.rerank_lvq2(Q, cand, c1, c28, mu, 4, 8, min(a.k, r), L2)  # noqa: E731
        f8 = lambda: _native.rerank("lvq", Q, cand, c8, (mu,), 8, min(a.k, r), L2)  # noqa: E731
        t44, t48, t8 = alternate([f44, f48, f8], a.reps, a.min_seconds)
        rec = [recall(f()[1].long() & 0xFFFFFFFF, gt) for f in (f44, f48, f8)]
        print(f"  {r:5d} {ms(t44):>28s} {ms(t48):>28s} {ms(t8):>28s}  {t44[0] / t8[0]:5.2f}  {t48[0] / t8[0]:5.2f}   "
              f"{rec[0]:.3f} / {rec[1]:.3f} / {rec[2]:.3f}  ({t44[3]} calls each)", flush=True)
        rows_out.append(dict(leg="rerank", r=r, lvq2_44_ms=t44[0] * 1e3, lvq2_48_ms=t48[0] * 1e3, lvq8_ms=t8[0] * 1e3,
                             recall_44=rec[0], recall_48=rec[1], recall_8=rec[2], calls=t44[3]))
    del c1, c24, c28, c8
    torch.cuda.empty_cache()

    # ---- the indexes
    print(f"# {'index':>32s} {'recall@' + str(a.k):>10s} {'q/s':>10s} {'MiB':>8s}")
    for f in a.factor:
        if a.k * f > 256:
            continue
        made = [(f"LVQ2Index(4, {b2}, {f})", (lambda b2=b2: LVQ2Index(4, b2, refine_factor=f))) for b2 in (4, 8)]
        made.append((f"RefinedIndex(LVQ-4, LVQ-8, {f})",
                     lambda: RefinedIndex(FlatQuantizedIndex(LVQQuantizer(4)), LVQQuantizer(8), refine_factor=f)))
        built = []
        for name, make in made:
            ix = make()
            ix.fit(X, "l2")
            built.append((name, ix))
        times = alternate([(lambda ix=ix: ix.search_with_scores(Q, a.k)) for _, ix in built], a.reps, a.min_seconds)
        for (name, ix), t in zip(built, times):
            ids = torch.from_numpy(ix.search(Q, a.k).astype("int64")).to(dev)
            rec, foot = recall(ids, gt), ix.memory_footprint()
            print(f"  {name:>32s} {rec:10.3f} {a.nq / t[0]:10.1f} {foot / 2**20:8.1f}   ({ms(t)}, {t[3]} calls)", flush=True)
            rows_out.append(dict(leg="index", name=name, factor=f, recall=rec, qps=a.nq / t[0], bytes=foot, calls=t[3]))
        del built, ix
        torch.cuda.empty_cache()
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(rows_out, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
