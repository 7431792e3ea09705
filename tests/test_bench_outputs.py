"""bench.py's plain run and its --dump-outputs: a run without --full times the headline encode
only, and the dumped codes are those of the timed path on seeded inputs, so that two builds can
be compared output for output."""

import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]


def test_options_default_off():
    import bench

    a = bench.parse([])
    assert a.full is False and a.dump_outputs is None
    a = bench.parse(["--full", "--dump-outputs", "d"])
    assert a.full is True and a.dump_outputs == "d"


def test_dump_outputs_all_rows_and_sample(tmp_path, monkeypatch):
    import bench

    codes = torch.from_numpy(np.random.default_rng(0).integers(0, 256, (1000, 16), dtype=np.uint8))
    info = bench.dump_outputs(codes, tmp_path / "all", 0, 1)
    got = np.load(tmp_path / "all" / "codes.npy")
    assert got.dtype == np.float32 and info["rows"] == "all"
    assert np.array_equal(got, codes.numpy().astype(np.float32))

    monkeypatch.setattr(bench, "DUMP_ROWS", 256)
    first = bench.dump_outputs(codes, tmp_path / "s1", 0, 1)
    bench.dump_outputs(codes, tmp_path / "s2", 0, 1)
    s1, s2 = np.load(tmp_path / "s1" / "codes.npy"), np.load(tmp_path / "s2" / "codes.npy")
    assert s1.shape == (256, 16) and first["shape"] == [256, 16] and np.array_equal(s1, s2)
    rows = np.sort(np.random.default_rng(bench.DUMP_SEED).choice(1000, 256, replace=False))
    assert np.array_equal(s1, codes.numpy()[rows].astype(np.float32))
    # per-rank files, the row budget shared between the ranks
    info = bench.dump_outputs(codes, tmp_path / "r", 1, 2)
    assert info["file"] == "codes_rank1.npy" and np.load(tmp_path / "r" / "codes_rank1.npy").shape == (128, 16)


@pytest.mark.gpu
def test_plain_run_dumps_the_timed_codes(dev, tmp_path):
    """One plain run (no --full) at a small shape: the legs behind --full are absent from the
    line, --steps is the number of timed steps, and codes.npy equals the encode of the same
    seeded rows and codebooks computed here."""
    import bench
    from haag_vq import _native

    n, d, M = 30000, 1536, 16
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--n", str(n),
           "--d", str(d), "--M", str(M), "--dump-outputs", str(tmp_path / "out")]
    p = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=120, cwd=str(tmp_path))
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-3000:]
    out = json.loads(lines[0])
    assert out["full"] is False and out["steps"] == 3 and out["warmup"] == 1
    assert out["ms_per_step"] > 0 and out["value"] == pytest.approx(n / (out["ms_per_step"] * 1e-3))
    for key in ("cpu_baseline", "parity_sample", "adc", "alt_data", "north_star", "config5", "configs"):
        assert out[key] is None, key
    assert out["outputs_dumped"]["shape"] == [n, M]
    assert sorted(f.name for f in (tmp_path / "out").iterdir()) == ["codes.npy"]
    got = np.load(tmp_path / "out" / "codes.npy")
    assert got.dtype == np.float32 and got.shape == (n, M)

    X = bench.synth(n, d, seed=0, dev=dev)
    C = bench.train_codebook(X, M, 8, 0, 1, dev)
    ref = _native.pq_encode(X, C, _native.pq_prepare(C, 8), 8)
    assert np.array_equal(got, ref.cpu().numpy().astype(np.float32))
