"""`vq-benchmark sweep` / `streaming-sweep` end to end on the GPU (BASELINE.json configs[0]).

The sweep runs through the CLI (typer) exactly as a user would start it, writes rows with
the reference's SQLite schema (utils/run_logger.py:71-115), and on the reference's dummy
dataset (np.random.seed(42); randn(10000, 1024), data/datasets.py:79-81) reproduces the
logged known answers of rows 38 (SQ-8) and 52 (RaBitQ-1) of logs/benchmark_runs.db
(tests/golden/kat.json).  PQ's logged numbers depend on faiss' k-means (absent), so the PQ
row is checked for schema, metric set, the exact compression ratio and a distortion within
3 % of the logged 916.89 (same data, different k-means implementation).
"""

import json
import sqlite3

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REF_COLUMNS = ["id", "timestamp", "git_branch", "git_commit", "package_version", "method", "dataset",
               "cli_command", "metrics_json", "config_json", "sweep_id"]


@pytest.fixture(scope="module")
def kat(golden_dir):
    return json.loads((golden_dir / "kat.json").read_text())


def _sweep(tmp_path, *args):
    from typer.testing import CliRunner

    from haag_vq.cli import app

    db = tmp_path / "runs.db"
    res = CliRunner().invoke(app, ["sweep", "--dataset", "dummy", "--db-path", str(db),
                                   "--codebooks-dir", str(tmp_path / "cb"), *args])
    assert res.exit_code == 0, res.output + repr(res.exception)
    con = sqlite3.connect(db)
    cols = [r[1] for r in con.execute("PRAGMA table_info(runs)")]
    rows = con.execute("SELECT method, dataset, metrics_json, config_json, sweep_id FROM runs").fetchall()
    con.close()
    assert cols == REF_COLUMNS
    return [(m, d, json.loads(mj), json.loads(cj), sid) for m, d, mj, cj, sid in rows]


DEVICE_FIELDS = {"device", "n_gpus", "encode_device_ms", "roofline_frac"}


def test_sweep_pq_m8_b8_dummy(tmp_path, kat):
    rows = _sweep(tmp_path, "--method", "pq", "--pq-subquantizers", "8", "--pq-bits", "8")
    assert len(rows) == 1
    method, dataset, metrics, config, sid = rows[0]
    ref = kat["46"]  # PQ(subquantizers=8, bits=8) on the same dummy dataset
    assert (method, dataset) == ("pq", "dummy")
    assert config == ref["config"]
    assert sid.startswith("sweep_")
    # the reference's fields, plus the device fields this build adds (sweep.py)
    assert set(metrics) == set(ref["metrics"]) | DEVICE_FIELDS
    assert metrics["n_gpus"] == 1 and metrics["device"] and 0.0 < metrics["roofline_frac"] < 1.0
    assert metrics["compression_ratio"] == ref["metrics"]["compression_ratio"] == 512.0
    assert metrics["reconstruction_distortion"] == pytest.approx(ref["metrics"]["reconstruction_distortion"], rel=0.03)
    assert metrics["rank_distortion@10"] == pytest.approx(1.0 - metrics["recall@10"])
    assert metrics["qps"] > 0


def test_sweep_pq_grid_rows(tmp_path):
    rows = _sweep(tmp_path, "--method", "pq", "--pq-subquantizers", "8,16", "--pq-bits", "8",
                  "--no-with-pairwise", "--no-with-rank", "--no-with-recall")
    assert [r[3]["subquantizers"] for r in rows] == [8, 16]
    assert len({r[4] for r in rows}) == 1  # one sweep id for the whole grid


def _check_kat(metrics, ref, rel_dist):
    assert metrics["compression_ratio"] == pytest.approx(ref["compression_ratio"])
    assert metrics["reconstruction_distortion"] == pytest.approx(ref["reconstruction_distortion"], rel=rel_dist)
    # ranking in fp32 on the GPU (the reference ranks fp64 reconstructions with sklearn):
    # at most a couple of near-tie swaps out of 1000 / 10000 hits
    for key in ("recall@10", "recall@100", "rank_distortion@10"):
        assert abs(metrics[key] - ref[key]) <= 0.002, key
    for key in ("pairwise_distortion_mean", "pairwise_distortion_median", "pairwise_distortion_max"):
        assert metrics[key] == pytest.approx(ref[key], rel=1e-5), key


def test_sweep_sq8_reproduces_row38(tmp_path, kat):
    rows = _sweep(tmp_path, "--method", "sq", "--sq-bits", "4,8")  # 4-bit is skipped, as upstream
    assert len(rows) == 1
    method, _, metrics, config, _ = rows[0]
    assert method == "sq" and config == kat["38"]["config"]
    _check_kat(metrics, kat["38"]["metrics"], rel_dist=1e-12)


def test_sweep_rabitq_reproduces_row52(tmp_path, kat):
    rows = _sweep(tmp_path, "--method", "rabitq", "--rabitq-metric-type", "L2")
    assert len(rows) == 1
    method, _, metrics, config, _ = rows[0]
    assert method == "rabitq" and config == kat["52"]["config"]
    _check_kat(metrics, kat["52"]["metrics"], rel_dist=1e-5)


def test_streaming_sweep_local_file(tmp_path):
    from typer.testing import CliRunner

    from haag_vq.cli import app

    rng = np.random.default_rng(5)
    X = rng.standard_normal((25_000, 64)).astype(np.float32)
    np.save(tmp_path / "stream.npy", X)
    db = tmp_path / "s.db"
    res = CliRunner().invoke(app, ["streaming-sweep", "--method", "pq", "--pq-subquantizers", "8",
                                   "--training-size", "5000", "--batch-size", "10000",
                                   "--data-path", str(tmp_path / "stream.npy"), "--db-path", str(db)])
    assert res.exit_code == 0, res.output + repr(res.exception)
    con = sqlite3.connect(db)
    (ds, mj), = con.execute("SELECT dataset, metrics_json FROM runs").fetchall()
    con.close()
    m = json.loads(mj)
    assert ds == "cohere-msmarco-streaming"
    assert m["total_vectors_compressed"] == 25_000 and m["num_batches"] == 3
    assert m["compression_ratio"] == 64 * 4 / 8
    # the streamed, batch-weighted MSE equals the whole-set distortion of the same model
    from haag_vq.methods.product_quantization import ProductQuantizer

    pq = ProductQuantizer(M=8, B=8)
    pq.fit(X[:5000])
    rec = pq.decompress(pq.compress(X))
    assert m["mse"] == pytest.approx(float(((X.astype(np.float64) - rec) ** 2).sum(1).mean()), rel=1e-6)


@pytest.mark.parametrize("method,margs", [("pq", ["--pq-subquantizers", "8"]), ("opq", ["--opq-quantizers", "8"]),
                                          ("sq", []), ("rabitq", [])], ids=["pq", "opq", "sq", "rabitq"])
def test_streaming_sweep_grouped_calls_equal_per_batch_calls(tmp_path, monkeypatch, method, margs):
    """The device encode takes several stream batches per call (streaming_sweep.CALL_ROWS); the
    logged row must equal the one of upstream's one-call-per-batch loop bit for bit (ragged
    last batch and a group boundary inside the run included), for every method the command
    streams."""
    from typer.testing import CliRunner

    from haag_vq.benchmarks import streaming_sweep as ss
    from haag_vq.cli import app

    X = np.random.default_rng(6).standard_normal((23_456, 96)).astype(np.float32)
    np.save(tmp_path / "stream.npy", X)
    out = {}
    for tag, rows in (("per_batch", 3000), ("grouped", 9000), ("one_call", 1 << 20)):
        monkeypatch.setattr(ss, "CALL_ROWS", rows)
        db = tmp_path / f"{tag}.db"
        res = CliRunner().invoke(app, ["streaming-sweep", "--method", method, *margs,
                                       "--training-size", "4096", "--batch-size", "3000",
                                       "--data-path", str(tmp_path / "stream.npy"), "--db-path", str(db)])
        assert res.exit_code == 0, res.output + repr(res.exception)
        con = sqlite3.connect(db)
        (mj,), = con.execute("SELECT metrics_json FROM runs").fetchall()
        con.close()
        out[tag] = json.loads(mj)
    assert ss.batches_per_call(3000, 96) == (1 << 20) // 3000
    for tag in ("grouped", "one_call"):
        assert out[tag]["mse"] == out["per_batch"]["mse"]
        assert out[tag]["num_batches"] == out["per_batch"]["num_batches"] == 8
        assert out[tag]["total_vectors_compressed"] == 23_456


def test_sweep_config1_standin_shape(tmp_path, monkeypatch, oracle):
    """BASELINE config #1's shape through the caller (SURVEY §8d row 1's stand-in for the
    offline dbpedia-100k): `sweep --dataset dbpedia-100k --method pq --pq-subquantizers 8
    --pq-bits 8` on a local 100k x 1536 unit-normalised Gaussian file (seed 0).  The logged row
    has the reference's schema and metric set, compression ratio 4 D / M = 768 (row 56), and the
    PQ8 (dsub 192) codes of a 20k-row sample equal the oracle's canonical encode under the
    codebook the sweep trained -- both the codes the sweep itself scored (the output of its
    compress call, captured during the run) and a fresh encode of the same rows."""
    from typer.testing import CliRunner

    import torch
    from haag_vq.benchmarks import sweep as sw
    from haag_vq.cli import app

    X = np.random.default_rng(0).standard_normal((100_000, 1536), dtype=np.float32)
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    np.save(tmp_path / "dbpedia-100k.npy", X)
    models, scored = [], []
    build = sw._build_model

    def capture(method, config):
        model = build(method, config)
        compress = model.compress

        def recording(rows):  # (rows of the call, its output): the first call is the one the sweep scores
            out = compress(rows)
            scored.append((rows.shape[0], out.cpu().numpy() if hasattr(out, "cpu") else np.array(out)))
            return out

        model.compress = recording
        models.append(model)
        return model

    monkeypatch.setattr(sw, "_build_model", capture)
    db = tmp_path / "runs.db"
    res = CliRunner().invoke(app, ["sweep", "--dataset", "dbpedia-100k", "--cache-dir", str(tmp_path), "--method",
                                   "pq", "--pq-subquantizers", "8", "--pq-bits", "8", "--db-path", str(db),
                                   "--codebooks-dir", str(tmp_path / "cb")])
    assert res.exit_code == 0, res.output + repr(res.exception)
    con = sqlite3.connect(db)
    cols = [r[1] for r in con.execute("PRAGMA table_info(runs)")]
    (method, dataset, mj, cj), = con.execute("SELECT method, dataset, metrics_json, config_json FROM runs").fetchall()
    con.close()
    assert cols == REF_COLUMNS and (method, dataset) == ("pq", "dbpedia-100k")
    m = json.loads(mj)
    assert json.loads(cj) == {"name": "PQ(subquantizers=8, bits=8)", "subquantizers": 8, "bits": 8}
    assert m["compression_ratio"] == 768.0
    for key in ("reconstruction_distortion", "recall@10", "recall@100", "qps", "rank_distortion@10",
                "pairwise_distortion_mean", "roofline_frac", "encode_device_ms"):
        assert key in m, key
    assert 0.0 < m["recall@10"] <= 1.0 and m["n_gpus"] == 1
    pq, = models
    C = pq.centroids_device.cpu().numpy()
    assert C.shape == (8, 256, 192)
    got = pq.compress(torch.from_numpy(X[:20_000]).cuda())
    got = got.cpu().numpy() if hasattr(got, "cpu") else np.asarray(got)
    want = oracle.pq_encode(X[:20_000], C)
    np.testing.assert_array_equal(got, want)
    rows, codes = scored[0]  # time_compress(model, X): what distortion, pairwise and recall were computed from
    assert rows == 100_000 and codes.shape == (100_000, 8) and codes.dtype == np.uint8
    np.testing.assert_array_equal(codes[:20_000], want)
