"""bench.py's contract with the driver, checked on the device: ONE JSON line on stdout with the metric of BASELINE.json, the whole-job value,
and with --full the `roofline` and `cpu_baseline` objects (measurement section of the task: bound / achieved / peak / unit / frac / traffic;
value / unit / cores / kind / sample); a plain run carries the headline alone and --dump-outputs writes what its last timed step computed."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_default_bench_line_carries_the_contract_fields():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "2", "--pre-roll", "3",
                        "--full"], capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    base = json.load(open(os.path.join(ROOT, "BASELINE.json")))
    assert d["unit"] == "Gaussians/s" and d["n_gpus"] == 1 and d["steps"] == 4 and d["warmup"] == 2 and d["higher_is_better"] is True
    assert d["metric"].startswith("Gaussians/s fwd+bwd, 288x512, N_exposure=8") and "Gaussians/s fwd+bwd" in base["metric"]
    assert d["dtype"] == "f32" and d["data"] == "synthetic" and d["vs_baseline"] is None and d["scaling"] in ("weak", "strong")
    assert "cfg2" in d["config"]["workload"] and d["config"]["pre_roll_steps"] == 3 and "model" not in d["config"]
    assert abs(d["value"] - 300000 / (d["ms_per_step"] * 1e-3)) <= 1e-6 * d["value"]  # whole-job throughput = N / frame time
    assert 0.5 < d["ms_per_step"] < 10.0
    roof = d["roofline"]
    assert roof["bound"] in ("hbm", "mfma") and roof["unit"] in ("GB/s", "TFLOP/s") and roof["peak"] > 0
    assert abs(roof["frac"] - roof["achieved"] / roof["peak"]) < 1e-9 and "traffic" in roof and roof["kernel"].startswith("k_raster_bwd")
    assert roof["avg_launch_ms"] > 0 and roof["peak_measured"] > 0  # the kernel's live duration and the box's measured ceiling
    # the honest number first: what binds the kernel and the hardware fraction precede the contract's nominal fields
    keys = list(roof)
    assert roof["bound_actual"] == "valu" and keys.index("bound_actual") < keys.index("bound") and keys.index("frac_hardware") < keys.index("frac")
    if roof["frac_hardware"] is not None:  # (None while profiles/ holds the counters of another build of the library)
        assert roof["frac_hardware"] == roof["hardware"]["frac_necessary"] and 0 < roof["frac_hardware"] < roof["frac"]
    cpu = d["cpu_baseline"]
    assert cpu["kind"] in ("port", "reference") and cpu["unit"] == "Gaussians/s" and cpu["value"] > 0 and cpu["cores"] >= 1 and cpu["sample"]
    # BASELINE.md section 3 in the default line: scalar C + one torch-restatement frame on cfg1, the product's CPU twin on cfg1 and cfg2
    assert cpu["runs"]["cfg1/scalar_c"]["iters"] == 20 and cpu["runs"]["cfg1/torch"]["gaussians_per_s"] > 0 and cpu["runs"]["cfg2/scalar_c"]["iters"] == 3
    assert cpu["product_cpu_twin"]["config"] == "cfg1" and cpu["product_cpu_twin_cfg2"]["gaussians_per_s"] > 0 and cpu["product_cpu_twin_cfg2"]["cores"] == 1
    assert d["value"] > 100 * cpu["value"]  # (a reported baseline, not a target: only that both legs measured the same thing)
    # the sustained cross-check (default 6 s of the same step right after the timed region; never `value`).  This test times FOUR steps, so
    # one host stall may double its mean: only that the two rates describe the same step (the real lines agree to 1 %: profiles/r06s_bench_*.json)
    sus = d["sustained"]
    assert sus["seconds"] >= 6.0 and sus["steps"] >= 1000 and 0.5 < sus["ms_per_step"] / d["ms_per_step"] < 1.5, sus
    assert 0.9 < sus["ms_per_step"] < 2.0 and abs(sus["value"] - 300000 / (sus["ms_per_step"] * 1e-3)) <= 1e-6 * sus["value"]


def test_plain_bench_line_is_the_headline_and_dumps_the_last_step(tmp_path):
    import numpy as np

    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "5", "--warmup", "2", "--pre-roll", "3",
                        "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["metric"].startswith("Gaussians/s fwd+bwd, 288x512, N_exposure=8") and d["unit"] == "Gaussians/s" and d["dtype"] == "f32"
    assert d["higher_is_better"] is True and d["steps"] == 5 and d["warmup"] == 2 and 0.5 < d["ms_per_step"] < 10.0
    assert abs(d["value"] - 300000 / (d["ms_per_step"] * 1e-3)) <= 1e-6 * d["value"]
    assert not {"roofline", "cpu_baseline", "sustained", "peaks_measured", "kernels_ms_per_step", "n_isect_per_step"} & set(d)
    got = {p.stem: np.load(p) for p in tmp_path.glob("*.npy")}
    assert {"renders", "alphas", "blended", "acc", "grad_means", "grad_colors", "grad_motion_coefs", "grad_viewmat"} <= set(got), sorted(got)
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
    assert got["blended"].shape == (288, 512, 4) and got["renders"].shape == (8, 288, 512, 4) and got["grad_means"].shape == (300000, 3)
    for k, a in got.items():
        assert a.dtype in (np.float32, np.float64) and np.isfinite(a).all(), k
    assert np.abs(got["grad_means"]).sum() > 0 and 0.0 <= got["acc"].min() and got["acc"].max() <= 1.0 + 1e-5
