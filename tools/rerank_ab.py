#!/usr/bin/env python3
"""Two-stage search (RefinedIndex's stages, device-resident) against its yardsticks, in one process.

A cheap base index over-fetches r = k * refine_factor candidates per query and mivq_rerank_* ranks
them again on a finer store of the same rows.  Neither yardstick is the code under test:

  base     the base index alone at k: what a user of the single-stage index gets today
  torch    the same re-rank written in torch on the same device: X[cand] (an (nq, r, d) f32 block),
           broadcast difference, square, sum, topk; for a code store the candidates' code rows are
           gathered and decoded first (mivq_lvq_decode / mivq_sq_decode_f32), then the same

Bases: FlatADCIndex (PQ, every --M), RaBitQIndex, IvfListPqIndex (the last --M, every --nprobe; its
centroids as tools/ivf_listpq_ab.py makes them).  Stores: the f32 rows, LVQ-8 and SQ-8 codes.  All
fitted once on the same seeded, clustered n x d rows.  Ground truth is mivq_flat_search on the f32
rows (exact L2).  Per (base, store, factor) the legs are warmed up, then timed alternately with HIP
events (device-resident queries, candidates and results); medians are reported.  Columns:

  recall@k   of the two stages, against the f32 ground truth (factor 1 re-ranks the base's own k)
  base q/s   the base index alone, asked for k results; its recall is printed once per base
  2st q/s    the base asked for r results, then the re-rank, as one leg
  rerank     ms of the mivq_rerank_* call alone on the base's candidates, and its peak scratch
             (workspace + results)
  torch      ms and peak scratch of the torch composition on the same candidates

  python tools/rerank_ab.py                                  # 1M x 1024, 1000 queries, k = 10
  python tools/rerank_ab.py --n 65536 --d 256 --nlist 32 --M 16 --nprobe 1 4     # a smaller box
"""

from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "vector-quantization_amd"))
sys.path.insert(0, str(ROOT / "tools"))

from ivf_listpq_ab import long_lists, with_heartbeat  # noqa: E402
from ivf_rabitq_ab import alternate, clustered, recall, timed  # noqa: E402


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--d", type=int, default=1024)
    ap.add_argument("--nq", type=int, default=1000)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--M", type=int, nargs="+", default=[16, 128])
    ap.add_argument("--nprobe", type=int, nargs="+", default=[1, 16])
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
    from haag_vq.methods.product_quantization import ProductQuantizer
    from haag_vq.methods.scalar_quantization import ScalarQuantizer
    from haag_vq.methods.search import FlatADCIndex, IvfListPqIndex, RaBitQIndex, search_codes

    dev = _native.require_device()
    print(f"# {torch.cuda.get_device_name(0)}  n={a.n} d={a.d} nq={a.nq} k={a.k} L2  {a.centres} centres  "
          f"kernels {_native.kernel_source_hash()}")
    X, Q = clustered(a.n, a.d, a.nq, a.centres, a.seed, dev)
    gt = _native.flat_search(Q, X, a.k, _native.METRIC_L2)[1].long()

    # --- the stores
    lvq, sq = LVQQuantizer(8), ScalarQuantizer(8)
    t_lvq = timed(lambda: lvq.fit(X))
    lvq_codes = lvq.compress(X)
    t_sq = timed(lambda: sq.fit(X))
    sq_codes = sq.compress(X)
    lo, den = sq._params(torch.float32)
    mu = lvq._mu_device()
    stores = {"f32": ("f32", X, (), 0), "lvq8": ("lvq", lvq_codes, (mu,), 8), "sq8": ("sq", sq_codes, (lo, den), 8)}
    mib = {nm: (s[1].numel() * s[1].element_size() + sum(p.numel() * 4 for p in s[2])) / 2**20 for nm, s in stores.items()}
    print(f"# stores: f32 {mib['f32']:.0f} MiB, LVQ-8 {mib['lvq8']:.0f} MiB (fit {t_lvq:.2f} s), SQ-8 {mib['sq8']:.0f} MiB "
          f"(fit {t_sq:.2f} s)")

    # --- the bases: name -> (search(r) -> (dists, ids int32 holding uint32), footprint MiB)
    bases = {}
    for M in a.M:
        flat = FlatADCIndex(ProductQuantizer(M=M, B=8))
        t = timed(lambda: flat.fit(X, "l2"))
        bases[f"adc M={M}"] = (lambda r, f=flat: search_codes(f.quantizer, f._codes, Q, r, "l2"), flat.memory_footprint() / 2**20)
        print(f"# fit adc M={M}: {t:.2f} s")
    rb = RaBitQIndex()
    t = timed(lambda: rb.fit(X, "l2"))
    bases["rabitq"] = (lambda r: rb.search_device(Q, r), rb.memory_footprint() / 2**20)
    print(f"# fit rabitq: {t:.2f} s")
    coarse, t_coarse, sizes = long_lists(X, a.nlist, 256)
    K, M = int(coarse.shape[0]), a.M[-1]
    ivf = IvfListPqIndex(lambda: ProductQuantizer(M=M, B=8), K=K, nprobe=a.nprobe[0])
    t = with_heartbeat("per-list fit", lambda: timed(lambda: ivf.fit(X, "l2", centroids=coarse)))
    print(f"# fit listpq M={M}: coarse k-means {t_coarse:.2f} s, K = {K} lists of at least 256 rows (mean "
          f"{sizes.float().mean():.0f}, max {int(sizes.max())}), per-list fit {t:.2f} s")

    def probe(r, nprobe):
        ivf.nprobe = nprobe
        return ivf.search_device(Q, r)

    for nprobe in a.nprobe:
        bases[f"listpq M={M} nprobe {nprobe}"] = (lambda r, p=nprobe: probe(r, p), ivf.memory_footprint() / 2**20)

    inf = torch.tensor(float("inf"), device=dev)

    def torch_rerank(store, cand):
        """The yardstick: gather (decode), broadcast difference, square, sum, topk."""
        kind, data, params, bits = stores[store]
        live = cand != -1  # 0xFFFFFFFF, the padding of the IVF searches
        rows = cand.long().clamp_(min=0)
        if kind == "f32":
            G = data[rows]
        elif kind == "lvq":
            G = _native.lvq_decode(data[rows.reshape(-1)], params[0], bits).view(*rows.shape, a.d)
        else:
            G = _native.sq_decode(data[rows.reshape(-1)].contiguous(), a.d, params[0], params[1], bits).view(*rows.shape, a.d)
        dist = torch.where(live, ((G - Q[:, None, :]) ** 2).sum(dim=2), inf)
        v, j = dist.topk(a.k, dim=1, largest=False)
        return v, torch.gather(cand, 1, j)

    def kernel_rerank(store, cand):
        kind, data, params, bits = stores[store]
        return _native.rerank(kind, Q, cand, data, params, bits, a.k, _native.METRIC_L2)

    def peak_mib(fn) -> float:
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        out = fn()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - before
        del out
        return peak / 2**20

    rows_out = []
    for bname, (search, foot) in bases.items():
        r_base = recall(search(a.k)[1].long() & 0xFFFFFFFF, gt)
        print(f"# {bname}: footprint {foot:.1f} MiB, recall@{a.k} alone {r_base:.3f}")
        print(f"# {'base / store / factor':>38s} {'recall@' + str(a.k):>10s} {'base q/s':>10s} {'2st q/s':>10s} {'rerank ms':>10s} "
              f"{'MiB':>7s} {'torch ms':>9s} {'MiB':>8s}   torch/rerank")
        for f in a.factor:
            r = min(a.k * f, 256)
            cand = search(r)[1].contiguous()
            short = float((cand == -1).any(dim=1).float().mean())
            for store in stores:
                got = kernel_rerank(store, cand)[1]
                want = torch_rerank(store, cand)[1]
                agree = float((got == want).all(dim=1).float().mean())  # not bit-identical chains: near-ties may differ
                rec = recall(got.long() & 0xFFFFFFFF, gt)
                (tb, _, _, _), (t2, _, _, calls), (tk, tk0, tk1, _), (tt, tt0, tt1, _) = alternate(
                    [lambda: search(a.k), lambda: kernel_rerank(store, search(r)[1]), lambda: kernel_rerank(store, cand),
                     lambda: torch_rerank(store, cand)], a.reps, a.min_seconds)
                pk, pt = peak_mib(lambda: kernel_rerank(store, cand)), peak_mib(lambda: torch_rerank(store, cand))
                print(f"  {bname + ' / ' + store + ' / x' + str(f):>38s} {rec:10.3f} {a.nq / tb:10.1f} {a.nq / t2:10.1f} "
                      f"{tk * 1e3:10.3f} {pk:7.2f} {tt * 1e3:9.3f} {pt:8.1f}   {tt / tk:5.2f}x  (r={r}, rerank "
                      f"{tk0 * 1e3:.3f}..{tk1 * 1e3:.3f} ms, torch {tt0 * 1e3:.3f}..{tt1 * 1e3:.3f} ms, {calls} calls, "
                      f"same ids as torch on {100 * agree:.1f} % of the queries, padded lists {100 * short:.0f} %)", flush=True)
                rows_out.append(dict(base=bname, store=store, factor=f, r=r, recall=rec, recall_base=r_base, base_ms=tb * 1e3,
                                     two_stage_ms=t2 * 1e3, rerank_ms=tk * 1e3, torch_ms=tt * 1e3, rerank_mib=pk,
                                     torch_mib=pt, agree=agree, padded=short, calls=calls))
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(rows_out, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
