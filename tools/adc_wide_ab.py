"""The wide flat ADC scan (csrc/adc_wide.hip, M * 2^nbits * 4 B > 160 KiB) next to the routes that
served such quantizers before it and next to the resident-table scan of its neighbours.

usage: python tools/adc_wide_ab.py [--n 1000000] [--d 1536] [--M 192 384] [--nq 1 100 1000] [--k 10]
                                   [--neighbours 128 160] [--reps 11]
Per M and query count, seeded Gaussian codebooks and queries, uniform random codes:
  (a) mivq_adc_search over the codes (the wide scan), alone and with mivq_adc_lut;
  (b) mivq_flat_search over mivq_pq_decode's rows, alone and with the decode: the route that
      worked before; its ids are compared with (a)'s slot by slot (they may differ on fp32 near-ties);
  (c) the resident-table scan (one query per workgroup) at the neighbouring M, same n and nq.
Each call is timed between device events and synchronised.  The legs of one shape are warmed up once
each and then called in turn, --reps rounds of (a scan, a lut + scan, b, b with decode), so that drift
of the machine falls on all of them alike; a time is printed as median [min .. max] of its --reps calls.
(a) is called faster or slower than (b) only where the two [min .. max] ranges do not overlap, on par
otherwise.  (a) and (c) also print the time per lookup, t / (nq n M), and the lookups' LDS bytes per
second (4 B each).  The first line names the library that is measured: the in-tree build of
csrc/Makefile (adc_wide.o with the Makefile's own per-file flags).
"""
import argparse
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "vector-quantization_amd"))
from haag_vq import _native  # noqa: E402


class T:
    """Times of one leg: median [min .. max] in ms."""

    def __init__(self, ts):
        ts = sorted(ts)
        self.med, self.lo, self.hi = ts[len(ts) // 2], ts[0], ts[-1]

    def __str__(self):
        return f"{self.med:.3f} ms [{self.lo:.3f} .. {self.hi:.3f}]"


def timed(legs, reps):
    """legs: functions; one warm-up each, then reps rounds calling them in turn."""
    for f in legs:
        f()
    torch.cuda.synchronize()
    ts, outs = [[] for _ in legs], [None] * len(legs)
    for _ in range(reps):
        for j, f in enumerate(legs):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            outs[j] = f()
            e.record()
            torch.cuda.synchronize()
            ts[j].append(s.elapsed_time(e))
    return [T(t) for t in ts], outs


def verdict(a, b):
    """a against b: faster / slower only where the ranges are disjoint."""
    if a.hi < b.lo:
        return f"faster, {b.med / a.med:.2f}x"
    if a.lo > b.hi:
        return f"slower, {b.med / a.med:.2f}x"
    return f"on par ({b.med / a.med:.2f}x by the medians, ranges overlap)"


def per_lookup(tag, t, nq, n, M):
    look = nq * n * M
    print(f"{tag}: {t} = {nq / t.med * 1e3:.0f} queries/s, {t.med * 1e6 / look * 1e3:.3f} ps per lookup, "
          f"{look * 4 / (t.med * 1e-3) / 1e12:.1f} TB/s of LDS lookups", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--d", type=int, default=1536)
    ap.add_argument("--M", type=int, nargs="+", default=[192, 384])
    ap.add_argument("--nq", type=int, nargs="+", default=[1, 100, 1000])
    ap.add_argument("--neighbours", type=int, nargs="*", default=[128, 160])
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--reps", type=int, default=11)
    a = ap.parse_args()
    dev = _native.require_device()
    g = torch.Generator(device=dev).manual_seed(3)
    Qall = torch.randn((max(a.nq), a.d), device=dev, generator=g)
    notfaster = []
    lib = Path(_native.LIB_PATH).resolve()
    print(f"library: {lib.relative_to(ROOT) if ROOT in lib.parents else lib} (the in-tree build of csrc/Makefile "
          f"unless MIVQ_LIB names another), reps {a.reps}", flush=True)
    for M in a.M:
        C = torch.randn((M, 256, a.d // M), device=dev, generator=g)
        codes = torch.randint(0, 256, (a.n, M), dtype=torch.uint8, device=dev, generator=g)
        xh = _native.pq_decode(codes, C, 8)
        for nq in a.nq:
            Q = Qall[:nq].contiguous()
            tag = f"M={M} n={a.n} nq={nq} k={a.k}"
            lut = _native.adc_lut(Q, C, 8)
            (ta, tal, tb, tbd), (oa, _, ob, _) = timed(
                [lambda: _native.adc_search(lut, codes, a.k, 8),
                 lambda: _native.adc_search(_native.adc_lut(Q, C, 8), codes, a.k, 8),
                 lambda: _native.flat_search(Q, xh, a.k),
                 lambda: _native.flat_search(Q, _native.pq_decode(codes, C, 8), a.k)], a.reps)
            per_lookup(f"(a) {tag} wide scan", ta, nq, a.n, M)
            print(f"(a) {tag} lut + wide scan: {tal} = {nq / tal.med * 1e3:.0f} queries/s", flush=True)
            print(f"(b) {tag} flat search of decoded rows: {tb}; decode + flat search: {tbd}", flush=True)
            diff = int((oa[1] != ob[1]).sum())
            v1, v2 = verdict(tal, tb), verdict(tal, tbd)
            print(f"(a) vs (b) {tag}: {diff} of {nq * a.k} id slots differ; (a) lut + scan against (b) without the "
                  f"decode: {v1}; with it: {v2}", flush=True)
            if not v1.startswith("faster"):
                notfaster.append(f"{tag}: {v1}")
        del xh
    for M in a.neighbours:
        codes = torch.randint(0, 256, (a.n, M), dtype=torch.uint8, device=dev, generator=g)
        for nq in a.nq:
            lut = torch.randn((nq, M, 256), device=dev, generator=g) ** 2
            (tc,), _ = timed([lambda: _native.adc_search(lut, codes, a.k, 8)], a.reps)
            per_lookup(f"(c) M={M} n={a.n} nq={nq} k={a.k} resident-table scan", tc, nq, a.n, M)
    print("(a) lut + scan is faster than (b) without the decode at every shape" if not notfaster
          else f"(a) lut + scan is not faster than (b) without the decode at: {notfaster}")


if __name__ == "__main__":
    main()
