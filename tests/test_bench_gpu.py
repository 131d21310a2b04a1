"""bench.py end to end on the GPU box (child processes): the contract line at N = 1 and the sharded step of `--gpus N` -- the path
the driver's multi-GPU run takes -- at world 1 over RCCL and at world 2 on one device over gloo."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(cmd, env=None, timeout=900):
    e = dict(os.environ)
    e.update(env or {})
    e.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    p = subprocess.run(cmd, cwd=ROOT, env=e, capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, lines          # ONE JSON line on stdout
    return json.loads(lines[0])


def test_headline_line_has_the_contract_fields(device):
    r = _run([sys.executable, "bench.py", "--steps", "12", "--warmup", "3", "--full", "--no-extras", "--no-cpu-baseline"])
    assert r["n_gpus"] == 1 and r["steps"] == 12 and r["warmup"] == 3 and r["unit"] == "views/s" and r["dtype"] == "f32"
    assert r["config"]["workload"] == "h36m_4view_1000x1000_P17_C17"
    assert abs(r["value"] - 4 / r["ms_per_step"] * 1e3) < 1e-6 * r["value"]
    roof = r["roofline"]
    assert roof["bound"] == "hbm" and roof["launches_timed"] >= 32 and 0.3 < roof["frac"] < 1.0
    assert abs(roof["frac"] - roof["achieved"] / roof["peak"]) < 1e-9
    assert roof["avg_launch_us"] * 1e-3 <= 1.5 * r["ms_per_step"]                  # the dominant kernel fits inside its step (sampled launches carry event pairs)
    # the headline is the two-call form (an upstream gradient may depend on the image); the one-call form is reported beside it
    # (faster by ~8 % over 200 steps; 12 steps are 0.7 ms of GPU time, where one hiccup of the host moves a mean by more than
    # that: the two forms only have to be of one order here)
    assert r["config"]["form"] == "two calls" and "sks_forward, then sks_backward" in r["config"]["path"]
    assert 0.5 < r["ms_per_step"] / r["one_call_step"]["ms_per_step"] < 2.0
    # the roofline figure is the kernel over 8 output sets in turn (an HBM rate), non-temporal stores
    assert roof["rotating_output_sets"] == 8 and roof["stores"] == "non-temporal" and 0.3 < roof["frac_same_buffer"] < 1.0


def test_sharded_step_at_world_1_over_rccl(device):
    """The `--gpus N` code path (views sharded, the backward and the collective on the second stream) with one rank."""
    r = _run([sys.executable, "bench.py", "--gpus", "1", "--steps", "6", "--warmup", "2", "--full", "--no-extras",
              "--no-cpu-baseline"], env={"SKS_BENCH_FORCE_DIST": "1", "MASTER_PORT": "29577"})
    assert r["n_gpus"] == 1 and r["config"]["views_total"] == 31 and r["config"]["views_on_rank0"] == 31
    assert r["config"]["exchange"] in ("all_gather", "all_reduce") and "RCCL" in r["config"]["parallelism"]
    assert r["value"] > 0 and r["roofline"]["frac"] > 0.3
    # at world 1 the sharded step does what the one-GPU reference does plus one collective: within a few percent of it
    assert 0.5 < r["speedup_vs_one_gpu_same_workload"] < 2.0      # (six steps: a sanity bound, not a measurement)


def test_sharded_step_at_world_2_on_one_device(device):
    """Two ranks on GPU 0 over gloo (RCCL refuses two ranks on one device): the sharding logic at world > 1 -- 16 + 15 views, pad
    rows, rank-major mean -- with the hidden exchange; timings mean nothing."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", "29578", "bench.py", "--gpus", "2", "--steps", "4", "--warmup", "1", "--no-extras", "--no-cpu-baseline"]
    r = _run(cmd, env={"SKS_BENCH_ONE_DEVICE": "1"})
    assert r["n_gpus"] == 2 and r["config"]["views_on_rank0"] == 16 and r["strong_scaling"]["ideal_speedup"] == 31 / 16
    assert "gloo" in r["config"]["parallelism"] and r["value"] > 0


def test_sharded_extras_at_world_2_on_one_device(device):
    """The same with the extras the driver's multi-GPU run carries (the loop's dense and sparse steps alone and sharded, frame
    sharding): every rank goes through the same collectives and the line still comes out as one."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", "29580", "bench.py", "--gpus", "2", "--steps", "10", "--warmup", "2", "--full"]
    r = _run(cmd, env={"SKS_BENCH_ONE_DEVICE": "1"})
    assert "loop_error" not in r, r.get("loop_error")
    assert "cpu_baseline" not in r            # the CPU sample belongs to the N = 1 line
    for tag in ("api_step", "loop_dense", "loop_sparse"):
        assert r["strong_scaling"][tag]["ms_per_step"] > 0
    assert r["frame_sharded"]["frames_per_s_all_ranks"] > 0 and r["mean_equals_one_gpu"] == "bit for bit"


def test_dump_outputs_writes_the_last_timed_step(device, tmp_path):
    """--dump-outputs: the timed step's last outputs as float32 .npy files (the colour planes as a seeded sample), at most 64 MB,
    consistent with each other; --steps is the number of timed steps."""
    import numpy as np
    out = tmp_path / "outputs"
    r = _run([sys.executable, "bench.py", "--steps", "7", "--warmup", "2", "--no-extras", "--no-cpu-baseline", "--form", "two",
              "--dump-outputs", str(out)])
    assert r["steps"] == 7 and r["ms_per_step"] > 0 and r["dumped_outputs"]["dir"] == str(out)
    names = set(r["dumped_outputs"]["arrays"])
    assert {"color", "invdepth", "radii", "dL_dmeans3D", "dL_dmeans3D_mean"} <= names
    assert {p.name for p in out.iterdir()} == {n + ".npy" for n in names}
    a = {n: np.load(out / (n + ".npy")) for n in names}
    assert all(x.dtype == np.float32 and np.isfinite(x).all() for x in a.values())
    assert sum(x.nbytes for x in a.values()) <= 64 << 20
    assert a["invdepth"].shape == (4, 1, 1000, 1000) and a["radii"].shape == (4, 17) and a["dL_dmeans3D"].shape == (4, 17, 3)
    assert a["color"].shape == (1 << 22,) and r["dumped_outputs"]["arrays"]["color"].startswith("sample of")
    assert (a["radii"] >= 0).all() and np.array_equal(a["radii"], np.round(a["radii"])) and a["radii"].max() > 0
    # the step's result is the mean of the per-view joint gradients the same call handed back
    mean = a["dL_dmeans3D"].astype(np.float64).mean(0)
    assert np.allclose(a["dL_dmeans3D_mean"], mean, rtol=1e-5, atol=1e-6 * np.abs(mean).max())


def test_plain_run_is_the_headline_alone_and_computes_what_full_computes(device, tmp_path):
    """Without --full the line carries the headline and the `roofline` of the timed steps' own event pairs, nothing measured
    behind them; the timed step's outputs are bit for bit those of a --full run with the same arguments."""
    import numpy as np
    base = [sys.executable, "bench.py", "--gpus", "1", "--steps", "9", "--warmup", "2"]
    r = _run(base + ["--dump-outputs", str(tmp_path / "plain")])
    f = _run(base + ["--full", "--no-extras", "--no-cpu-baseline", "--dump-outputs", str(tmp_path / "full")])
    for k in ("metric", "unit", "higher_is_better", "dtype", "steps", "warmup"):
        assert r[k] == f[k], k
    assert r["n_gpus"] == 1 and abs(r["value"] - 4 / r["ms_per_step"] * 1e3) < 1e-6 * r["value"]
    assert r["config"]["form"] == "two calls" and r["config"]["autotuned"] is not None
    assert not {"one_call_step", "cpu_baseline", "same_buffer_plain_stores", "bwd_kernel_avg_us", "panoptic", "stress"} & set(r)
    assert "one_call_step" in f
    roof = r["roofline"]
    assert roof["timed_in"].startswith("the timed region") and "rotating_output_sets" not in roof and 0 < roof["launches_timed"] <= 9
    assert r["dumped_outputs"]["arrays"] == f["dumped_outputs"]["arrays"]
    for n in r["dumped_outputs"]["arrays"]:
        assert np.array_equal(np.load(tmp_path / "plain" / (n + ".npy")), np.load(tmp_path / "full" / (n + ".npy"))), n
