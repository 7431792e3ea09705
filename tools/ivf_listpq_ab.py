#!/usr/bin/env python3
"""IvfListPqIndex against two yardsticks on the same clustered rows and queries, in one process.

Neither yardstick is the code under test:

  ivfpq     FaissIvfPqIndex at the same K, M, B and nprobe: the same code bytes per row, scanned
            with one shared residual codebook and one lookup table per query
  flat      FlatQuantizedIndex(ProductQuantizer(M, B)): the flat ADC over every row

All three are fitted on the same seeded, clustered n x d rows; the two IVF indexes share one set of
coarse centroids.  A codebook of 2^B centroids is not trained on fewer points, so IvfListPqIndex
refuses a fit in which a non-empty list holds fewer than 2^B rows.  The tool therefore trains
--nlist centroids, assigns the rows, and drops the centroids whose lists are shorter than that
(their rows go to the nearest remaining centroid, so no remaining list shrinks); the K it reports
is what is left, for both IVF indexes.  Ground truth is mivq_flat_search on the f32 rows (exact
L2).  Per leg the searches are warmed up, then timed alternately with HIP events (device-resident
queries and results); the median is reported with the range.  Per run:

  q/s        queries per second of the whole search (IVF: probe selection + tables + scan)
  recall@k   against the f32 ground truth
  mse        mean squared reconstruction error over --mse-rows sampled rows (one sample for all)
  tables     IvfListPqIndex: mivq_ivf_listpq_search on the same probes over lists emptied of their
             rows (all offsets 0): the pair prologue, the sort, the table build and the merge run
             as before, no row is scanned
  scan       the time of mivq_ivf_listpq_search minus `tables`
  fit        seconds of IvfListPqIndex.fit with the given centroids (assign + K codebook trainings
             + encode), next to the yardsticks' fits

  python tools/ivf_listpq_ab.py                          # 1M x 1024, 1000 queries, nlist 1024, M 16 and 128
  python tools/ivf_listpq_ab.py --n 65536 --d 256 --nlist 32 --M 16 --nprobe 1 8     # a smaller box
"""

from __future__ import annotations

import argparse
import json
import sys
import threading
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "vector-quantization_amd"))
sys.path.insert(0, str(ROOT / "tools"))

from ivf_rabitq_ab import alternate, clustered, recall, timed  # noqa: E402


def with_heartbeat(what: str, fn, every: float = 60.0):
    """fn(), with a line every `every` seconds while it runs (a fit of K codebooks is silent)."""
    done = threading.Event()
    t0 = time.time()

    def beat():
        while not done.wait(every):
            print(f"#   ... {what}: {time.time() - t0:.0f} s", flush=True)

    th = threading.Thread(target=beat, daemon=True)
    th.start()
    try:
        return fn()
    finally:
        done.set()
        th.join()


def long_lists(X, nlist: int, ksub: int):
    """Coarse centroids whose lists all hold at least ksub rows: train nlist, drop the short ones.
    Returns (centroids, seconds of the k-means, list sizes after the drop)."""
    import torch

    from haag_vq.methods._ivf import assign, train_coarse

    holder = {}
    t = timed(lambda: holder.setdefault("c", train_coarse(X, nlist)))
    C = holder["c"]
    cnt = torch.bincount(assign(X, C)[1].long(), minlength=nlist)
    C = C[cnt >= ksub].contiguous()
    cnt = torch.bincount(assign(X, C)[1].long(), minlength=C.shape[0])
    assert int(cnt.min()) >= ksub  # rows were only added to the lists that stayed
    return C, t, cnt


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--d", type=int, default=1024)
    ap.add_argument("--nq", type=int, default=1000)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--M", type=int, nargs="+", default=[16, 128])
    ap.add_argument("--B", type=int, default=8)
    ap.add_argument("--nprobe", type=int, nargs="+", default=[1, 4, 16, 64])
    ap.add_argument("--centres", type=int, default=4096, help="Gaussian centres of the data")
    ap.add_argument("--mse-rows", type=int, default=50_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--json", type=str, default=None, help="also write the rows to this file")
    a = ap.parse_args()

    import numpy as np
    import torch

    from haag_vq import _native
    from haag_vq.methods import _ivf
    from haag_vq.methods.product_quantization import ProductQuantizer
    from haag_vq.methods.search import FaissIvfPqIndex, FlatQuantizedIndex, IvfListPqIndex, search_codes

    dev = _native.require_device()
    print(f"# {torch.cuda.get_device_name(0)}  n={a.n} d={a.d} nq={a.nq} k={a.k} L2  {a.centres} centres  "
          f"B={a.B}  kernels {_native.kernel_source_hash()}")
    X, Q = clustered(a.n, a.d, a.nq, a.centres, a.seed, dev)
    gt = _native.flat_search(Q, X, a.k, _native.METRIC_L2)[1].long()
    coarse, t_coarse, sizes = long_lists(X, a.nlist, 1 << a.B)
    K = int(coarse.shape[0])
    sizes_f = sizes.float()
    print(f"# coarse k-means {t_coarse:.2f} s for {a.nlist} centroids; {a.nlist - K} of them had lists under {1 << a.B} rows "
          f"and were dropped: K = {K} for both IVF indexes; lists: mean {sizes_f.mean():.0f}, min {int(sizes.min())}, "
          f"max {int(sizes.max())} rows")
    sample = torch.from_numpy(np.sort(np.random.default_rng(a.seed).permutation(a.n)[:min(a.n, a.mse_rows)])).to(dev)
    Xs = X[sample]

    def mse(xh) -> float:
        return float(((Xs - xh) ** 2).mean(dim=1).double().mean())

    rows = []
    for M in a.M:
        tag = f"M={M}"

        def pq():
            return ProductQuantizer(M=M, B=a.B)

        # --- the index under test
        ivf = IvfListPqIndex(pq, K=K, nprobe=a.nprobe[0])
        t_fit = with_heartbeat(f"{tag} per-list fit", lambda: timed(lambda: ivf.fit(X, "l2", centroids=coarse)))
        eng = ivf._index
        mse_ivf = mse(eng.reconstruct(sample))
        # --- yardstick 1: shared-codebook IVF-PQ on the same centroids (its coarse step replaced)
        ypq = FaissIvfPqIndex(K=K, m=M, nbits=a.B, nprobe=a.nprobe[0])
        orig = _ivf.train_coarse
        _ivf.train_coarse = lambda *args, **kw: coarse
        try:
            t_ypq = timed(lambda: ypq.fit(X, "l2"))
        finally:
            _ivf.train_coarse = orig
        ye = ypq._index
        assert ye.coarse is coarse and torch.equal(ye.lists.offsets, eng.lists.offsets)
        pos = torch.empty(a.n, dtype=torch.int64, device=dev)
        pos[ye.lists.ids.long()] = torch.arange(a.n, device=dev)
        p = pos[sample]
        cs = ye.lists.codes[p].long()  # one byte per sub-code: the gather of the shared codebook, plus the centroid
        dec = torch.cat([ye.pq[m][cs[:, m]] for m in range(M)], dim=1)
        mse_ypq = mse(dec + coarse[ye._list_of()[p].long()])
        # --- yardstick 2: flat ADC
        flat = FlatQuantizedIndex(pq())
        t_flat = timed(lambda: flat.fit(X, "l2"))
        mse_flat = mse(flat.quantizer.decompress(flat._codes[sample].contiguous()))

        def flat_search():
            return search_codes(flat.quantizer, flat._codes, Q, a.k, "l2")

        r_flat = recall(flat_search()[1].long() & 0xFFFFFFFF, gt)
        print(f"# {tag}: fit: listpq (assign + {K} codebook trainings + encode) {t_fit:.2f} s, ivfpq (one codebook + "
              f"encode) {t_ypq:.2f} s, flat {t_flat:.2f} s; footprint listpq {ivf.memory_footprint() / 2**20:.1f} MiB "
              f"(codebooks {K * a.d * (1 << a.B) * 4 / 2**20:.1f}), ivfpq {ypq.memory_footprint() / 2**20:.1f} MiB, "
              f"flat {flat.memory_footprint() / 2**20:.1f} MiB")
        print(f"# {tag}: reconstruction mse over {sample.numel()} rows: listpq {mse_ivf:.6f}, ivfpq {mse_ypq:.6f}, "
              f"flat {mse_flat:.6f}")
        print(f"# {'index':>26s} {'ms':>9s} {'q/s':>10s} {'recall@' + str(a.k):>10s} {'mse':>9s}   split / range")
        L = eng.lists
        no_rows = torch.zeros_like(L.offsets)
        for nprobe in a.nprobe:
            ivf.nprobe = ypq.nprobe = nprobe
            pl = eng.probes(Q, nprobe)

            def search(offsets):
                return _native.ivf_listpq_search(Q, eng.codebooks, eng.coarse, pl, offsets, L.codes, L.ids, eng.nbits,
                                                 eng.metric, a.k)

            (tf, tf0, tf1, calls), (ti, ti0, ti1, _), (ty, ty0, ty1, _), (tp, _, _, _), (ts, _, _, _), (tt, _, _, _) = alternate(
                [flat_search, lambda: ivf.search_device(Q, a.k), lambda: ye.search(Q, a.k, nprobe),
                 lambda: eng.probes(Q, nprobe), lambda: search(L.offsets), lambda: search(no_rows)], a.reps, a.min_seconds)
            r_ivf = recall(ivf.search_device(Q, a.k)[1].long() & 0xFFFFFFFF, gt)
            r_ypq = recall(ye.search(Q, a.k, nprobe)[1].long() & 0xFFFFFFFF, gt)
            if nprobe == a.nprobe[0]:
                print(f"  {tag + ' flat':>26s} {tf * 1e3:9.3f} {a.nq / tf:10.1f} {r_flat:10.3f} {mse_flat:9.6f}   "
                      f"({tf0 * 1e3:.3f}..{tf1 * 1e3:.3f} ms, {calls} calls, alternated with the first ivf legs)")
            print(f"  {tag + ' ivfpq nprobe ' + str(nprobe):>26s} {ty * 1e3:9.3f} {a.nq / ty:10.1f} {r_ypq:10.3f} "
                  f"{mse_ypq:9.6f}   ({ty0 * 1e3:.3f}..{ty1 * 1e3:.3f} ms)")
            print(f"  {tag + ' listpq nprobe ' + str(nprobe):>26s} {ti * 1e3:9.3f} {a.nq / ti:10.1f} {r_ivf:10.3f} "
                  f"{mse_ivf:9.6f}   probe selection {tp * 1e3:.3f} ms + tables {tt * 1e3:.3f} ms + scan "
                  f"{max(ts - tt, 0.0) * 1e3:.3f} ms; ({ti0 * 1e3:.3f}..{ti1 * 1e3:.3f} ms, flat alongside {tf * 1e3:.3f} ms)",
                  flush=True)
            rows.append(dict(M=M, B=a.B, K=K, nprobe=nprobe, listpq_ms=ti * 1e3, ivfpq_ms=ty * 1e3, flat_ms=tf * 1e3,
                             probe_ms=tp * 1e3, search_ms=ts * 1e3, tables_ms=tt * 1e3, recall_listpq=r_ivf,
                             recall_ivfpq=r_ypq, recall_flat=r_flat, mse_listpq=mse_ivf, mse_ivfpq=mse_ypq,
                             mse_flat=mse_flat, fit_listpq_s=t_fit, fit_ivfpq_s=t_ypq, fit_flat_s=t_flat, calls=calls))
        del ivf, eng, ypq, ye, flat, L
        torch.cuda.empty_cache()
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(rows, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
