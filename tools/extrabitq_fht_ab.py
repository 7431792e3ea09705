#!/usr/bin/env python3
"""A/B of the two rotations of ExtendedRaBitQuantizer, in one process on seeded data:

  dense   the seeded QR matrix P: normalize -> (n, D) x (D, D) fp64 MFMA GEMM -> quantize
  fht     four rounds of sign flips + Walsh-Hadamard transform, fused into one kernel a side
          (mivq_extrabitq_encode_fht / _decode_fht), and the same work staged through
          mivq_extrabitq_normalize -> mivq_fht_rotate -> mivq_extrabitq_quantize

Per shape, at B bits: compress, decompress and rotate_queries (1 and 1000 queries) of both are
warmed up, then timed alternately with HIP events, 11 calls each; medians with [min .. max].  Also
printed: that the fused codes equal the staged ones, the reconstruction MSE of both rotations and
the recall@10 of ExtendedRaBitQFlatIndex over both code arrays against the exact fp32 search.

  python tools/extrabitq_fht_ab.py                              # 1M x 1024 and 100k x 1536 at B = 4
  python tools/extrabitq_fht_ab.py --shapes 65536x256           # a smaller box
"""

from __future__ import annotations

import argparse
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "vector-quantization_amd"))

from haag_vq import _native as N  # noqa: E402
from haag_vq.methods.extended_rabitq import ExtendedRaBitQuantizer  # noqa: E402
from haag_vq.methods.search.flat_quantized_index import ExtendedRaBitQFlatIndex  # noqa: E402


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3


def alternate(fns, reps):
    """(median, min, max) seconds of each of `fns`, warmed up and then called in turn `reps` times."""
    for _ in range(2):
        for f in fns:
            f()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for t, f in zip(ts, fns):
            t.append(timed(f))
    return [(sorted(t)[len(t) // 2], min(t), max(t)) for t in ts]


def ms(t):
    return f"{t[0] * 1e3:9.3f} ms [{t[1] * 1e3:.3f} .. {t[2] * 1e3:.3f}]"


def overlap(a, b) -> float:
    return float(np.mean([len(np.intersect1d(x, y)) / len(x) for x, y in zip(a, b)]))


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", type=str, default="1000000x1024 100000x1536")
    ap.add_argument("--bits", type=int, default=4)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    dev = N.require_device()
    B, k = a.bits, a.k
    print(f"# {torch.cuda.get_device_name(0)}  B={B} k={k} L2  {a.reps} calls each, alternated  "
          f"kernels {N.kernel_source_hash()}")
    for shape in a.shapes.split():
        n, d = (int(v) for v in shape.split("x"))
        g = torch.Generator(device=dev).manual_seed(a.seed)
        std = 0.5 + 1.5 * torch.rand(d, generator=g, device=dev)
        off = torch.randn(d, generator=g, device=dev)
        X = torch.randn((n, d), generator=g, device=dev) * std + off
        Qs = {nq: torch.randn((nq, d), generator=g, device=dev) * std + off for nq in (1, 1000)}
        truth = N.flat_search(Qs[1000], X, k)[1].cpu().numpy().view(np.uint32)
        qd, qf = (ExtendedRaBitQuantizer(B, a.seed, rotation=r) for r in ("dense", "fht"))
        for q in (qd, qf):
            q.fit(X)
        c, signs, lv = qf._state()

        def staged_encode():
            o, nrm = N.extrabitq_normalize(X, c)
            return N.extrabitq_quantize(N.fht_rotate(o, signs, out=o), lv, B, nrm)

        def staged_decode(codes):
            y = N.extrabitq_dequantize(codes, lv, B, d)
            return N.extrabitq_finish(N.fht_rotate(y, signs, inverse=True, out=y), codes, c, B)

        cd, cf = qd.compress(X), qf.compress(X)
        same = bool(torch.equal(cf, staged_encode())) and bool(torch.equal(qf.decompress(cf), staged_decode(cf)))
        print(f"{n} x {d}: code rows {qd.code_size} bytes; rotation state dense {d * d * 8 / 1e6:.2f} MB, "
              f"fht {signs.numel() / 8 / 1e3:.2f} kB as bits; fused == staged bit for bit: {same}")
        legs = (("compress", [lambda: qd.compress(X), lambda: qf.compress(X), staged_encode]),
                ("decompress", [lambda: qd.decompress(cd), lambda: qf.decompress(cf), lambda: staged_decode(cf)]),
                ("rotate_queries nq 1", [lambda: qd.rotate_queries(Qs[1]), lambda: qf.rotate_queries(Qs[1])]),
                ("rotate_queries nq 1000", [lambda: qd.rotate_queries(Qs[1000]), lambda: qf.rotate_queries(Qs[1000])]))
        for name, fns in legs:
            t = alternate(fns, a.reps)
            print(f"  {name:23s} dense {ms(t[0])}   fht {ms(t[1])}   dense / fht {t[0][0] / t[1][0]:7.2f}x"
                  + (f"   fht staged {ms(t[2])}" if len(t) > 2 else ""), flush=True)
        for name, q, codes in (("dense", qd, cd), ("fht", qf, cf)):
            m = min(n, 100_000)
            mse = float(((q.decompress(codes[:m]) - X[:m]) ** 2).mean())
            idx = ExtendedRaBitQFlatIndex(q)
            idx._codes, idx._N, idx._D, idx._metric = codes, n, d, "l2"
            ids, _ = idx.search_with_scores(Qs[1000], k)
            print(f"  {name:5s} reconstruction MSE (first {m} rows) {mse:.6e}   recall@{k} over 1000 queries "
                  f"{overlap(truth, ids):.4f}", flush=True)
        del X, cd, cf, qd, qf
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
