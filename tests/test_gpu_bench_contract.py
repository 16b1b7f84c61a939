"""-m gpu: bench.py keeps the driver's contract -- one JSON line on stdout with the agreed keys and exactly K timed steps; a
plain run carries nothing else, --full adds the roofline and cpu_baseline objects (shortened: small CPU-baseline sample, no
frame / style extras)."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_bench_prints_one_contract_line(tmp_path):
    dump = tmp_path / "outputs"
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "24", "--warmup", "3", "--full", "--cpu-rays", "4096",
                          "--no-frame", "--no-style", "--dump-outputs", str(dump)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    j = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in j, k
    assert j["unit"] == "Mrays/s" and j["n_gpus"] == 1 and j["steps"] == 24 and j["higher_is_better"] is True
    assert j["scaling"] == "weak" and j["vs_baseline"] is None and j["data"] == "synthetic"
    assert "workload" in j["config"] and "model" not in j["config"]
    assert abs(j["value"] - 4096 / (j["ms_per_step"] * 1e-3) / 1e6) < 1e-2 * j["value"]
    r = j["roofline"]
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3 and 0.05 < r["frac"] < 1.0
    assert abs(r["achieved"] - r["bytes_per_sample"] * r["samples_per_launch"] / r["avg_launch_us"] / 1e3) < 0.02 * r["achieved"]
    c = j["cpu_baseline"]
    assert c["kind"] == "port" and c["unit"] == "Mrays/s" and c["cores"] >= 1 and c["value"] > 0 and "sample" in c
    assert j["value"] > 100 * c["value"]
    assert c["cpu_model"] and c["one_thread"]["value"] > 0 and c["one_thread"]["value"] <= 1.5 * c["value"]
    assert j["windows"]["median"] == j["ms_per_step"] and j["world_size"] == 1 and j["backend"] is None
    m = j["roofline_more"]                                           # the kernels furthest below their roofline
    for k in ("grid_backward_main_stream", "grid_backward_total"):
        assert m[k]["bound"] == "hbm" and m[k]["peak"] == 8000.0 and 0.02 < m[k]["frac"] < 1.0
        assert abs(m[k]["achieved"] - 588 * m[k]["samples_per_launch"] / m[k]["avg_us"] / 1e3) < 0.02 * m[k]["achieved"]
    assert m["grid_backward_total"]["avg_us"] > m["grid_backward_main_stream"]["avg_us"]
    for k, flop in (("head_forward", 36864), ("head_backward", 73728)):
        assert m[k]["bound"] == "mfma" and m[k]["peak"] == 2500.0 and m[k]["flop_per_sample"] == flop and 0.01 < m[k]["frac"] < 1.0
    assert "frame_encoder" not in m                                  # --no-frame: no inference kernels in this run (the default line has it)
    # round 6: the line says what --warmup asked for beside what ran, where `traffic` comes from, and carries the zero-edit drop-in step
    assert j["warmup_requested"] == 3 and j["warmup"] >= 17
    assert r["traffic"] is None or "not counted in this run" in r["traffic_source"]
    d = j["drop_in_step"]
    assert "error" not in d, d
    assert d["rays"] == 4096 and d["ms_per_step"] > j["ms_per_step"] and 0 < d["device_ms_per_step"] <= 1.05 * d["ms_per_step"]
    assert abs(d["device_ms_per_step"] - sum(d["device_stretches_ms"])) < 0.05 * d["device_ms_per_step"] and len(d["device_stretches_ms"]) == 3
    assert d["bound_by"].startswith("host") or d["bound_by"] == "device"
    assert abs(d["device_time_vs_fused_step"] - d["device_ms_per_step"] / j["ms_per_step"]) < 0.02 * d["device_time_vs_fused_step"]
    nn = d["without_network_nan_check"]
    assert len(nn["device_stretches_ms"]) == 2 and nn["ms_per_step"] <= 1.1 * d["ms_per_step"]
    for k in ("with_one_edit", "with_two_edits"):                    # the optional edits of INTEGRATION 3b, in the order they pay
        assert "error" not in d[k] and 0 < d[k]["device_ms_per_step"] < d["device_ms_per_step"], (k, d[k])
    assert d["with_two_edits"]["device_ms_per_step"] < d["with_one_edit"]["device_ms_per_step"]
    # --dump-outputs: what the last timed step returned and the parameters it left, float32 / float64, <= 64 MB in all
    a = {f[:-4]: np.load(dump / f) for f in os.listdir(dump)}
    assert {"image", "depth", "weights_sum", "loss", "n_samples", "encoder.embeddings", "sigma_net.weights", "color_net.weights"} <= set(a)
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert all(np.isfinite(v).all() for v in a.values())
    missed = a["nears"] == np.finfo(np.float32).max                   # rays missing the box: the step's depth is 0/0, the dump's 0
    assert np.all(a["depth"][missed] == 0)
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    assert a["image"].shape == (4096, 3) and a["weights_sum"].shape == (4096,) and a["n_samples"] > 0
    assert a["encoder.embeddings"].shape == (1 << 20, 2)


# what a plain line may carry: the headline and what describes how it was measured; everything else needs --full
PLAIN_KEYS = {"metric", "value", "unit", "n_gpus", "world_size", "backend", "steps", "warmup", "warmup_requested", "ms_per_step",
              "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config", "windows", "side_stream"}


def test_plain_bench_is_the_headline_alone(tmp_path):
    """`bench.py --steps K --warmup W` without --full: set-up, warm-up, the K timed steps, the dump and the line -- no eager
    diagnostic steps, extra workloads or CPU baselines -- and at most 30 s of the process's wall time outside its steps."""
    dump = tmp_path / "outputs"
    steps, warmup = 24, 3
    t0 = time.perf_counter()
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
                          "--dump-outputs", str(dump)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    wall = time.perf_counter() - t0
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    j = json.loads(lines[0])
    assert set(j) == PLAIN_KEYS, set(j) ^ PLAIN_KEYS
    assert j["metric"] == "Mrays/s, lego 800x800 train-step (4096 rays/step)" and j["unit"] == "Mrays/s" and j["higher_is_better"] is True
    assert j["dtype"] == "f16 (table, MLP) / f32 (march, composite)"
    assert j["n_gpus"] == 1 and j["steps"] == steps and j["warmup_requested"] == warmup and j["warmup"] >= 17
    assert abs(j["value"] - 4096 / (j["ms_per_step"] * 1e-3) / 1e6) < 1e-2 * j["value"]
    assert j["windows"]["median"] == j["ms_per_step"] and j["config"]["hip_graph_replay"] is True
    outside = wall - (steps + warmup) * j["ms_per_step"] * 1e-3
    assert outside < 30.0, f"{outside:.1f} s outside the steps"
    a = {f[:-4]: np.load(dump / f) for f in os.listdir(dump)}       # --dump-outputs works without --full
    assert {"image", "depth", "weights_sum", "loss", "n_samples", "encoder.embeddings", "sigma_net.weights", "color_net.weights"} <= set(a)
    assert all(np.isfinite(v).all() for v in a.values()) and a["image"].shape == (4096, 3)
