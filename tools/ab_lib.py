"""Interleaved A/B of one entry point between two builds of libmivq.so (same process, same data).

usage: python tools/ab_lib.py OTHER.so [--what encode|adc|lut|flat|sq|rabitq|lvq|pairwise|ivf_rabitq|ivf_sq|ivf_lvq|
                                              gemm_f64|gram]
                              [--n 1000000] [--d 1536] [--M 16] [--data gaussian] [--reps 10]
                              [--nq 1000] [--k 10] [--metric l2|ip] [--nbits 8] [--this THIS.so]
                              [--nlist 1024] [--nprobe 16] [--qb 4] [--transpose]
The in-tree library (vector-quantization_amd/lib/libmivq.so) is "this"; OTHER.so is e.g. a
build of the previous commit (git stash; make; cp lib/libmivq.so /tmp/old.so; git stash pop).
--this names another build in its place (the same file as OTHER.so: an A/A pass, the noise floor
of the comparison).  Both must report this build's mivq_abi_version().
Prints per-call medians of alternating single calls (HIP events) and back-to-back rates, and
checks that both builds give identical outputs:
  encode    mivq_pq_encode, the codes
  adc, lut  mivq_adc_search over the encoded rows (ids and distances), mivq_adc_lut
  flat, sq, rabitq, lvq   the exact searches mivq_flat_search, mivq_sq_flat_search,
            mivq_rabitq_flat_search, mivq_lvq_flat_search (SQ / LVQ: --nbits) of --nq queries
            over seeded random rows / codes, ids and distances
  pairwise  mivq_pairwise_distances of --n rows against --nq rows, the whole matrix
  ivf_rabitq, ivf_sq, ivf_lvq   the searches over probed lists mivq_ivf_rabitq_search (--qb),
            mivq_ivf_sq_search, mivq_ivf_lvq_search (--nbits): seeded random code rows in --nlist lists
            of seeded uneven sizes, --nprobe random distinct lists per query, no training; ids and keys
  gemm_f64  mivq_extrabitq_rotate (the fp64 GEMM of csrc/gemm_f64.hip): a seeded Gaussian (n, d) o times a
            QR factor P, or P^T with --transpose; the product, and the fp64 MFMA rate (2 n d^2 FLOP per call)
  gram      mivq_opq_gram: seeded Gaussian f32 X and Y (Y with per-column scales 0.01 .. 100), the Gram matrix
"""
import argparse
import ctypes
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "vector-quantization_amd"))
sys.path.insert(0, str(ROOT))
from haag_vq import _native  # noqa: E402
from haag_vq.methods._kmeans import train_pq  # noqa: E402
from bench import synth  # noqa: E402

P = ctypes.c_void_p


def bind(path):
    lib = ctypes.CDLL(str(path))
    for name, (res, args) in _native.SIGNATURES.items():
        if hasattr(lib, name):
            f = getattr(lib, name)
            f.restype, f.argtypes = res, args
    want = _native.load_library().mivq_abi_version()
    got = lib.mivq_abi_version() if hasattr(lib, "mivq_abi_version") else None
    if got != want:  # SIGNATURES describes this build's ABI only
        sys.exit(f"ab_lib: {path} has ABI version {got}, this build {want}")
    return lib


def _ptr(t):
    return None if t is None else P(t.data_ptr())


def _rows(n, code_bytes, trailer, seed, dev):
    """(n, code_bytes + 8 * trailer) random code bytes; the trailer two floats in [0.5, 1.5)."""
    g = torch.Generator(device=dev).manual_seed(seed)
    rows = torch.randint(0, 256, (n, code_bytes + 8 * trailer), dtype=torch.uint8, device=dev, generator=g)
    if trailer:
        f = torch.rand((n, 2), dtype=torch.float32, device=dev, generator=g) + 0.5
        rows[:, code_bytes:] = f.view(torch.uint8)
    return rows


# --what of an exact search: its entry point and, from (args, device), the database and the
# arguments that stand between d and the metric in its signature.
def _f32_db(a, dev):
    return synth(a.n, a.d, 0, dev, kind=a.data), []


def _sq_db(a, dev):
    lo = synth(1, a.d, 3, dev).reshape(-1)
    den = lo.abs() + 0.5
    return _rows(a.n, {4: (a.d + 1) // 2, 8: a.d, 16: 2 * a.d}[a.nbits], 0, 5, dev), [lo, den, a.nbits]


def _rabitq_db(a, dev):
    return _rows(a.n, (a.d + 7) // 8, 1, 5, dev), [synth(1, a.d, 3, dev).reshape(-1)]


def _lvq_db(a, dev):
    return _rows(a.n, (a.d * a.nbits + 7) // 8, 1, 5, dev), [synth(1, a.d, 3, dev).reshape(-1), a.nbits]


EXACT = {
    "flat": ("mivq_flat_search", _f32_db),
    "sq": ("mivq_sq_flat_search", _sq_db),
    "rabitq": ("mivq_rabitq_flat_search", _rabitq_db),
    "lvq": ("mivq_lvq_flat_search", _lvq_db),
}


IVF = ("ivf_rabitq", "ivf_sq", "ivf_lvq")
GEMM = ("gemm_f64", "gram")


def exact_leg(a, libs, dev, st):
    """run(k) and outputs() of an exact search or of mivq_pairwise_distances."""
    metric = _native.METRIC_L2 if a.metric == "l2" else _native.METRIC_INNER_PRODUCT
    Q = synth(a.nq, a.d, 7, dev, kind=a.data)
    if a.what == "pairwise":
        X = synth(a.n, a.d, 0, dev, kind=a.data)
        out = {k: torch.empty((a.n, a.nq), dtype=torch.float32, device=dev) for k in libs}

        def run(k):
            rc = libs[k].mivq_pairwise_distances(_ptr(X), a.n, _ptr(Q), a.nq, a.d, metric, _ptr(out[k]), P(st))
            assert rc == 0, (rc, libs[k].mivq_last_error())

        return run, lambda k: (out[k],)
    name, make = EXACT[a.what]
    db, params = make(a, dev)
    bufs = {}
    for k, lb in libs.items():
        nb = getattr(lb, name + "_workspace_bytes")(a.nq, a.n, a.d, a.k)
        bufs[k] = (torch.empty(max(nb, 256), dtype=torch.uint8, device=dev),
                   torch.empty((a.nq, a.k), dtype=torch.float32, device=dev),
                   torch.empty((a.nq, a.k), dtype=torch.int32, device=dev))

    def run(k):
        ws, od, oi = bufs[k]
        mid = [_ptr(v) if isinstance(v, torch.Tensor) else v for v in params]
        rc = getattr(libs[k], name)(_ptr(Q), a.nq, _ptr(db), a.n, a.d, *mid, metric, a.k, 0, _ptr(ws), ws.numel(),
                                    _ptr(od), _ptr(oi), P(st))
        assert rc == 0, (rc, libs[k].mivq_last_error())

    return run, lambda k: bufs[k][1:]


def ivf_leg(a, libs, dev, st):
    """run(k) and outputs() of a search over probed lists of constructed code rows."""
    metric = _native.METRIC_L2 if a.metric == "l2" else _native.METRIC_INNER_PRODUCT
    g = torch.Generator(device=dev).manual_seed(11)
    w = torch.rand(a.nlist, device=dev, generator=g) ** 2 + 0.05  # list sizes from 1 to about 20 shares
    sizes = (w / w.sum() * a.n).long()
    sizes[0] += a.n - sizes.sum()
    offsets = torch.cat([sizes.new_zeros(1), sizes.cumsum(0)])
    ids = torch.randperm(a.n, device=dev, generator=g).to(torch.int32)
    probe_l = torch.rand((a.nq, a.nlist), device=dev, generator=g).argsort(1)[:, :a.nprobe].to(torch.int32).contiguous()
    Q = synth(a.nq, a.d, 7, dev, kind=a.data)
    coarse = synth(a.nlist, a.d, 9, dev)
    par = synth(a.nlist, a.d, 3, dev)
    if a.what == "ivf_rabitq":
        codes, mid, extra = _rows(a.n, (a.d + 7) // 8, 1, 5, dev), [a.qb], []
    elif a.what == "ivf_sq":
        codes = _rows(a.n, {4: (a.d + 1) // 2, 8: a.d, 16: 2 * a.d}[a.nbits], 0, 5, dev)
        mid, extra = [par, par.abs() + 0.5, a.nbits], [a.nbits]
    else:
        codes, mid, extra = _rows(a.n, (a.d * a.nbits + 7) // 8, 1, 5, dev), [par, a.nbits], [a.nbits]
    name = f"mivq_{a.what}_search"
    bufs = {}
    for k, lb in libs.items():
        nb = getattr(lb, name + "_workspace_bytes")(a.nq, a.n, a.nlist, a.nprobe, a.d, *extra, a.k)
        assert nb > 0, name
        bufs[k] = (torch.empty(nb, dtype=torch.uint8, device=dev),
                   torch.empty((a.nq, a.k), dtype=torch.float32, device=dev),
                   torch.empty((a.nq, a.k), dtype=torch.int32, device=dev))

    def run(k):
        ws, od, oi = bufs[k]
        args = [_ptr(v) if isinstance(v, torch.Tensor) else v for v in mid]
        rc = getattr(libs[k], name)(_ptr(Q), a.nq, a.d, _ptr(coarse), a.nlist, _ptr(probe_l), a.nprobe, _ptr(offsets),
                                    _ptr(codes), _ptr(ids), *args, metric, a.k, _ptr(ws), ws.numel(), _ptr(od), _ptr(oi),
                                    P(st))
        assert rc == 0, (rc, libs[k].mivq_last_error())

    return run, lambda k: bufs[k][1:]


def gemm_leg(a, libs, dev, st):
    """run(k) and outputs() of the fp64 GEMM (mivq_extrabitq_rotate) or of mivq_opq_gram."""
    g = torch.Generator(device=dev).manual_seed(5)
    if a.what == "gemm_f64":
        o = torch.randn((a.n, a.d), dtype=torch.float64, device=dev, generator=g)
        Pm = torch.linalg.qr(torch.randn((a.d, a.d), dtype=torch.float64, device=dev, generator=g))[0].contiguous()
        out = {k: torch.empty((a.n, a.d), dtype=torch.float64, device=dev) for k in libs}

        def run(k):
            rc = libs[k].mivq_extrabitq_rotate(_ptr(o), a.n, a.d, _ptr(Pm), int(a.transpose), _ptr(out[k]), P(st))
            assert rc == 0, (rc, libs[k].mivq_last_error())

        return run, lambda k: (out[k],)
    X = torch.randn((a.n, a.d), device=dev, generator=g)
    Y = torch.randn((a.n, a.d), device=dev, generator=g) * (torch.rand(a.d, device=dev, generator=g) * 99.99 + 0.01)
    bufs = {}
    for k, lb in libs.items():
        ws = torch.empty(max(lb.mivq_opq_gram_workspace_bytes(a.n, a.d), 256), dtype=torch.uint8, device=dev)
        bufs[k] = (ws, torch.empty((a.d, a.d), dtype=torch.float64, device=dev))

    def run(k):
        ws, G = bufs[k]
        rc = libs[k].mivq_opq_gram(_ptr(X), _ptr(Y), a.n, a.d, _ptr(ws), ws.numel(), _ptr(G), P(st))
        assert rc == 0, (rc, libs[k].mivq_last_error())

    return run, lambda k: (bufs[k][1],)


def pq_leg(a, libs, dev, st):
    """run(k) and outputs() of mivq_pq_encode, mivq_adc_lut or mivq_adc_search."""
    X = synth(a.n, a.d, 0, dev, kind=a.data)
    C = train_pq(X[:65536], a.M, 8, niter=25, seed=1234).contiguous()
    state = {}
    for k, lb in libs.items():
        prep = torch.empty(lb.mivq_pq_prep_bytes(a.d, a.M, 8), dtype=torch.uint8, device=dev)
        assert lb.mivq_pq_prepare(P(C.data_ptr()), a.d, a.M, 8, P(prep.data_ptr()), P(st)) == 0
        nb = lb.mivq_pq_encode_workspace_bytes(a.n, a.d, a.M, 8)
        ws = torch.empty(nb, dtype=torch.uint8, device=dev)
        out = torch.empty((a.n, a.M), dtype=torch.uint8, device=dev)
        state[k] = (prep, ws, out)

    def run_encode(k):
        lb = libs[k]
        prep, ws, out = state[k]
        rc = lb.mivq_pq_encode(P(X.data_ptr()), a.n, a.d, a.M, 8, P(C.data_ptr()), P(prep.data_ptr()),
                               P(ws.data_ptr()), ws.numel(), P(out.data_ptr()), 0, P(st))
        assert rc == 0, rc

    if a.what == "encode":
        return run_encode, lambda k: (state[k][2],)
    Q = synth(a.nq, a.d, 7, dev, kind=a.data)
    if a.what == "lut":  # mivq_adc_lut alone: the LUTs of nq queries
        luts = {k: torch.empty((a.nq, a.M, 256), dtype=torch.float32, device=dev) for k in libs}

        def run_lut(k):
            rc = libs[k].mivq_adc_lut(P(Q.data_ptr()), a.nq, a.d, a.M, 8, P(C.data_ptr()), 1, P(luts[k].data_ptr()), P(st))
            assert rc == 0, rc

        return run_lut, lambda k: (luts[k],)
    run_encode("this")
    codes = state["this"][2]
    lut = torch.empty((a.nq, a.M, 256), dtype=torch.float32, device=dev)
    assert libs["this"].mivq_adc_lut(P(Q.data_ptr()), a.nq, a.d, a.M, 8, P(C.data_ptr()), 1, P(lut.data_ptr()),
                                     P(st)) == 0
    adc = {}
    for k, lb in libs.items():
        nb = lb.mivq_adc_search_workspace_bytes(a.nq, a.n, a.M, 8, a.k)
        adc[k] = (torch.empty(max(nb, 256), dtype=torch.uint8, device=dev),
                  torch.empty((a.nq, a.k), dtype=torch.float32, device=dev),
                  torch.empty((a.nq, a.k), dtype=torch.int32, device=dev))

    def run_adc(k):
        ws, od, oi = adc[k]
        rc = libs[k].mivq_adc_search(P(lut.data_ptr()), a.nq, P(codes.data_ptr()), a.n, a.M, 8, a.k, 0,
                                     P(ws.data_ptr()), ws.numel(), P(od.data_ptr()), P(oi.data_ptr()), 0, P(st))
        assert rc == 0, rc

    return run_adc, lambda k: adc[k][1:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("other")
    ap.add_argument("--this", default=str(_native.LIB_PATH))
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--d", type=int, default=1536)
    ap.add_argument("--M", type=int, default=16)
    ap.add_argument("--data", default="gaussian")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--what", choices=("encode", "adc", "lut", "pairwise", *EXACT, *IVF, *GEMM), default="encode")
    ap.add_argument("--nq", type=int, default=1000)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--metric", choices=("l2", "ip"), default="l2")
    ap.add_argument("--nbits", type=int, default=8)
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--nprobe", type=int, default=16)
    ap.add_argument("--qb", type=int, default=4)
    ap.add_argument("--transpose", action="store_true")
    a = ap.parse_args()
    dev = _native.require_device()
    libs = {k: bind(p if Path(p).is_absolute() else ROOT / p) for k, p in (("this", a.this), ("other", a.other))}
    st = torch.cuda.current_stream().cuda_stream
    leg = (pq_leg if a.what in ("encode", "adc", "lut") else ivf_leg if a.what in IVF
           else gemm_leg if a.what in GEMM else exact_leg)
    run, outputs = leg(a, libs, dev, st)
    for k in libs:
        run(k)
    torch.cuda.synchronize()
    same = all(torch.equal(x, y) for x, y in zip(outputs("this"), outputs("other")))
    print(f"{a.what}: outputs identical: {same}", flush=True)
    res = {k: [] for k in libs}
    for _ in range(a.reps * 3):
        for k in libs:
            s_, e_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s_.record(); run(k); e_.record()
            torch.cuda.synchronize()
            res[k].append(s_.elapsed_time(e_))
    for k in libs:
        t = sorted(res[k])
        print(f"AB {k}: median {t[len(t) // 2]:.3f} ms  min {t[0]:.3f}  max {t[-1]:.3f}", flush=True)
    for rnd in range(2):
        for k in libs:
            s_, e_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            for _ in range(3):
                run(k)
            s_.record()
            for _ in range(20):
                run(k)
            e_.record()
            torch.cuda.synchronize()
            ms = s_.elapsed_time(e_) / 20
            if a.what == "encode":
                gbs = a.n * (4 * a.d + a.M) / (ms * 1e-3) / 1e9
                print(f"AB {k} round {rnd}: back-to-back {ms:.3f} ms/call = {gbs / 8000:.3f} of 8 TB/s", flush=True)
            elif a.what in GEMM:
                tf = 2.0 * a.n * a.d * a.d / (ms * 1e-3) / 1e12
                print(f"AB {k} round {rnd}: back-to-back {ms:.3f} ms/call = {tf:.1f} TF/s", flush=True)
            else:
                print(f"AB {k} round {rnd}: back-to-back {ms:.3f} ms/call = {a.nq / ms * 1e3:.0f} queries/s", flush=True)
    if not same:
        sys.exit(1)


if __name__ == "__main__":
    main()
