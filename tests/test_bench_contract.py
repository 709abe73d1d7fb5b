"""The JSON line bench.py prints (the copy kept under profiles/) carries every field the driver's contract names; a plain run
prints the headline alone and --dump-outputs writes the last timed step's outputs."""
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_line_contract():
    d = json.load(open(os.path.join(ROOT, "profiles", "r01_bench_default_run.json")))
    base = json.load(open(os.path.join(ROOT, "BASELINE.json")))
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["metric"] == base["metric"] and d["higher_is_better"] is True and d["scaling"] == "weak"
    assert d["vs_baseline"] is None and not base.get("published")            # no published number for this metric
    assert d["dtype"] == "f32" and d["data"] == "synthetic" and "workload" in d["config"] and "model" not in d["config"]
    r = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in r, k
    assert r["bound"] in ("hbm", "mfma") and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9
    assert r["traffic"] is None or r["traffic"] > 0
    c = d["cpu_baseline"]
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in c, k
    assert c["kind"] in ("reference", "port") and c["cores"] >= 1
    # value = clips of all ranks / max-over-ranks time
    assert abs(d["value"] - d["n_gpus"] * d["config"]["global_batch"] / d["n_gpus"] / (d["ms_per_step"] * 1e-3)) < 1e-6 * d["value"]


def test_bench_line_self_verifying_distributed_fields():
    """round 5: the line of a run with a process group (`profiles/r05_bench_force_dist_one_rank.json`: `bench.py --gpus 1 --force-dist`,
    the code path of N = 2, 4, 8) carries what makes a multi-GPU run verify itself — how many ranks RCCL really reduced over, the
    library version, every rank's step time, what DistributedDataParallel did with the gradients, and the k-means row's exchange"""
    path = os.path.join(ROOT, "profiles", "r05_bench_force_dist_one_rank.json")
    d = json.load(open(path))
    assert "watchdog" not in d, "the secondary rows of this run were cut short by bench.py's watchdog: the line is a headline only"
    dist = d["distributed"]
    assert dist["initialised"] is True and dist["backend"] == "nccl"
    assert dist["rccl_ranks_seen"] == d["n_gpus"] == dist["world_size_env"] == len(dist["ms_per_step_per_rank"])
    assert dist["rccl_version"].count(".") == 2
    assert dist["ms_per_step_min"] <= dist["ms_per_step_max"] <= d["ms_per_step"] * 1.001
    ddp = dist["ddp"]
    assert ddp["buckets"] == len([b for b in ddp["bucket_sizes_bytes"].split(",") if b.strip()]) >= 1
    assert isinstance(ddp["gradient_as_bucket_view"], bool) and ddp["gradient_bytes"] == 34520896 * 4       # R3D-18: 34.52 M parameters
    sec = d["secondary"]
    ex = sec["exchange"]
    assert ex["kind"] in ("allreduce", "allgather", "oneshot") and ex["collectives_per_iteration"] == 1
    assert ex["payload_bytes_per_rank"] == (500 * 512 + 500 + 2) * 8                                      # fp64 [K D sums | K counts | n_changed]
    assert sec["weak_scaled"]["scaling"] == "weak" and sec["weak_scaled"]["n_gpus"] == d["n_gpus"]
    one = d.get("kmeans_oneshot_row_from_stderr")
    assert one and one["exchange"]["kind"] == "oneshot" and one["value"] > 0


def test_bench_cli_has_full_and_dump_outputs():
    """--full (everything beyond the headline) and --dump-outputs DIR are options of the command line; parsing needs no GPU"""
    import subprocess
    import sys
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:]
    assert "--full" in p.stdout and "--dump-outputs DIR" in p.stdout


@pytest.mark.gpu
def test_bench_plain_run_headline_and_dumped_outputs(gpu, tmp_path):
    """a plain `bench.py --gpus 1 --steps K --warmup W --dump-outputs DIR`: one JSON line with the headline keys and none of --full's
    rows, K timed steps in ms_per_step, and the last step's outputs as float32 .npy files under 64 MB"""
    import subprocess
    import sys
    import numpy as np
    out = tmp_path / "dump"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(out)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-4000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    d = json.loads(lines[0])
    base = json.load(open(os.path.join(ROOT, "BASELINE.json")))
    assert d["metric"] == base["metric"] and d["unit"] == "clips/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0
    assert abs(d["value"] - d["config"]["global_batch"] / (d["ms_per_step"] * 1e-3)) < 1e-6 * d["value"]
    for k in ("roofline", "whole_step", "cpu_baseline", "secondary"):
        assert k not in d, k
    files = {f: np.load(os.path.join(out, f)) for f in os.listdir(out)}
    assert set(files) == {"loss.npy", "embeddings.npy", "params_sample.npy", "grads_sample.npy", "buffers_sample.npy"}
    assert sum(os.path.getsize(os.path.join(out, f)) for f in files) <= 64 << 20
    for f, a in files.items():
        assert a.dtype in (np.float32, np.float64) and a.size > 0 and np.isfinite(a).all(), f
    assert files["embeddings.npy"].shape == (32, 128)
    assert abs(float(files["loss.npy"][0]) - d["config"]["final_loss"]) <= 1e-6 * max(1.0, abs(d["config"]["final_loss"]))
    assert files["params_sample.npy"].shape == files["grads_sample.npy"].shape
