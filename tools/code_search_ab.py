#!/usr/bin/env python3
"""A/B of the two exact flat searches over SQ / RaBitQ-1 codes, in one process on seeded data:

  (a) decode + flat_search   the fp32 reconstruction of the whole database, then mivq_flat_search
  (b) code search            mivq_sq_flat_search / mivq_rabitq_flat_search on the codes

Both are in the library; (a) is what search_codes ran before (b) existed and what bench.py's
SQ-8 / RaBitQ-1 "search" figures still time.  Per shape the two are warmed up, then timed
alternately with HIP events; ids and distance bits must be identical.  Printed per shape: q/s
of both, the algorithmic code bytes (n x row bytes, read once) over the time of (b), and
torch.cuda.max_memory_allocated of one call of each (above what the inputs occupy).

  python tools/code_search_ab.py                       # 1M x 3072, the shapes of DESIGN.md §3.3
  python tools/code_search_ab.py --n 65536 --d 256 --nq 1 100   # a smaller box
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


def make_db(fmt: str, n: int, d: int, dev, seed: int):
    g = torch.Generator(device=dev).manual_seed(seed)
    if fmt == "rabitq":
        nb = (d + 7) // 8
        codes = torch.randint(0, 256, (n, nb + 8), generator=g, device=dev, dtype=torch.uint8)
        tail = torch.stack([torch.ones(n, device=dev), torch.rand(n, generator=g, device=dev) + 0.5], dim=1)
        codes[:, nb:] = tail.contiguous().view(torch.uint8).view(n, 8)
        return dict(fmt=fmt, d=d, codes=codes)
    nbits = int(fmt[2:])
    if nbits == 16:
        codes = torch.randint(-32768, 32768, (n, d), generator=g, device=dev, dtype=torch.int16)
    else:
        codes = torch.randint(0, 256, (n, d if nbits == 8 else (d + 1) // 2), generator=g, device=dev, dtype=torch.uint8)
    lo = torch.randn(d, generator=g, device=dev)
    den = torch.rand(d, generator=g, device=dev) + 0.5
    return dict(fmt=fmt, d=d, codes=codes, lo=lo, den=den, nbits=nbits)


def path_a(db, Q, k):
    if db["fmt"] == "rabitq":
        xh = _native.rabitq_decode(db["codes"], db["d"], None)
    else:
        xh = _native.sq_decode(db["codes"], db["d"], db["lo"], db["den"], db["nbits"])
    return _native.flat_search(Q, xh, k, _native.METRIC_L2)


def path_b(db, Q, k):
    if db["fmt"] == "rabitq":
        return _native.rabitq_flat_search(Q, db["codes"], db["d"], None, k, _native.METRIC_L2)
    return _native.sq_flat_search(Q, db["codes"], db["d"], db["lo"], db["den"], db["nbits"], k, _native.METRIC_L2)


def peak_of(fn, *args):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn(*args)
    torch.cuda.synchronize()
    return out, torch.cuda.max_memory_allocated() - base


def timed(fn, *args):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn(*args)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--d", type=int, default=3072)
    ap.add_argument("--nq", type=int, nargs="+", default=[1, 8, 100, 1000])
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5, help="timed calls of each path per shape (alternated)")
    ap.add_argument("--min-seconds", type=float, default=0.5, help="keep alternating until each path ran this long")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--json", type=str, default=None, help="also write the rows to this file")
    a = ap.parse_args()
    dev = _native.require_device()
    print(f"# {torch.cuda.get_device_name(0)}  n={a.n} d={a.d} k={a.k} L2  kernels {_native.kernel_source_hash()}")
    print(f"# {'format':7s} {'nq':>5s} {'path':>6s} {'a q/s':>10s} {'b q/s':>10s} {'b/a':>6s} {'b ms':>9s} "
          f"{'code GB/s':>10s} {'a peak MB':>10s} {'b peak MB':>10s}  same")
    shapes = [("sq8", nq) for nq in a.nq] + [("rabitq", nq) for nq in a.nq]
    mid = 100 if 100 in a.nq else a.nq[-1]
    shapes += [("sq4", mid), ("sq16", mid)]
    rows, db, ok = [], None, True
    for fmt, nq in shapes:
        if db is None or db["fmt"] != fmt:
            db = None
            torch.cuda.empty_cache()
            db = make_db(fmt, a.n, a.d, dev, a.seed)
        g = torch.Generator(device=dev).manual_seed(a.seed + 1 + nq)
        Q = torch.randn((nq, a.d), generator=g, device=dev)
        (da, ia), pk_a = peak_of(path_a, db, Q, a.k)  # also the warm-up of both paths
        (dbb, ib), pk_b = peak_of(path_b, db, Q, a.k)
        same = torch.equal(ia, ib) and torch.equal(da.view(torch.int32), dbb.view(torch.int32))
        ok = ok and same
        ta, tb = [], []
        while len(ta) < a.reps or min(sum(ta), sum(tb)) < a.min_seconds:
            ta.append(timed(path_a, db, Q, a.k))
            tb.append(timed(path_b, db, Q, a.k))
            if len(ta) >= 200:
                break
        ma, mb = sorted(ta)[len(ta) // 2], sorted(tb)[len(tb) // 2]
        code_bytes = db["codes"].numel() * db["codes"].element_size()
        tiled = nq >= 16 and a.n >= 4096
        row = dict(fmt=fmt, nq=nq, path="tiled" if tiled else "scan", a_qps=nq / ma, b_qps=nq / mb, a_ms=ma * 1e3,
                   b_ms=mb * 1e3, a_min_ms=min(ta) * 1e3, a_max_ms=max(ta) * 1e3, b_min_ms=min(tb) * 1e3,
                   b_max_ms=max(tb) * 1e3, calls=len(ta), code_gbps=code_bytes / mb / 1e9, a_peak=pk_a, b_peak=pk_b,
                   same=bool(same))
        rows.append(row)
        print(f"  {fmt:7s} {nq:5d} {row['path']:>6s} {row['a_qps']:10.1f} {row['b_qps']:10.1f} {ma / mb:6.2f} "
              f"{mb * 1e3:9.3f} {row['code_gbps']:10.1f} {pk_a / 1e6:10.1f} {pk_b / 1e6:10.1f}  "
              f"{'identical' if same else 'DIFFERENT'}   (a {min(ta) * 1e3:.3f}..{max(ta) * 1e3:.3f} ms, "
              f"b {min(tb) * 1e3:.3f}..{max(tb) * 1e3:.3f} ms, {len(ta)} calls each)", flush=True)
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(rows, indent=1))
    print("# all results identical" if ok else "# RESULTS DIFFER")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
