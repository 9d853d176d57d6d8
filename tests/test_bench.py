"""The headline harness contract (``bench.py``): ``--gpus N`` starts N rank processes by itself
(no torchrun needed), the rank count must agree with a torchrun environment, and rank 0 prints
one JSON line whose ``value`` is the whole-job aggregate.  CPU: gloo ranks on the tiny model."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env_extra=None, timeout=300):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env.update(env_extra or {})
    env["CUDA_VISIBLE_DEVICES"] = ""          # CPU ranks (gloo) even where a GPU is visible
    env["HIP_VISIBLE_DEVICES"] = ""
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True,
                          text=True, timeout=timeout, env=env, cwd=ROOT)


def _json_lines(out):
    return [json.loads(l) for l in out.splitlines() if l.startswith("{")]


def test_bench_gpus2_spawns_two_ranks():
    r = _run(["--gpus", "2", "--model", "tiny", "--steps", "1", "--warmup", "0", "--no-score"])
    assert r.returncode == 0, r.stderr[-3000:]
    lines = _json_lines(r.stdout)
    assert len(lines) == 1, r.stdout                 # rank 0 only
    out = lines[0]
    assert out["n_gpus"] == 2
    assert out["comm"] == {"backend": "gloo", "world_size": 2, "oversubscribed": False}
    assert out["finite"] in (True, None)
    assert [p["rank"] for p in out["per_rank"]] == [0, 1]
    assert out["config"]["global_batch"] == 8
    # whole-job aggregate: 2 ranks x 4 images x 1 step over the slowest rank's time
    assert abs(out["value"] - 8 / (out["ms_per_step"] / 1e3)) / out["value"] < 0.01


def test_bench_plain_run_is_lean_and_dumps_reproducible_outputs(tmp_path):
    """A plain run measures the headline only (no scorer / batch-1 / extras: those need ``--full``);
    ``--dump-outputs`` writes the last timed step's images as float32, identical from run to run."""
    import numpy as np
    arrs = []
    for d in ("a", "b"):
        r = _run(["--gpus", "1", "--model", "tiny", "--steps", "2", "--warmup", "1",
                  "--dump-outputs", str(tmp_path / d)])
        assert r.returncode == 0, r.stderr[-3000:]
        lines = _json_lines(r.stdout)
        assert len(lines) == 1, r.stdout
        out = lines[0]
        assert out["steps"] == 2 and out["ms_per_step"] > 0 and out["full"] is False
        assert abs(out["value"] - 4 / (out["ms_per_step"] / 1e3)) / out["value"] < 0.01
        for k in ("p50_score_ms", "cpu_minilm_1pair_p50_ms", "sdxl_fp8_s_per_image", "live_images_per_s"):
            assert k not in out
        assert out["batch1_s_per_image"] is None
        assert sorted(os.listdir(tmp_path / d)) == ["images.npy"]
        a = np.load(tmp_path / d / "images.npy")
        assert a.dtype == np.float32 and a.shape == (4, 16, 16, 3) and out["dumped"]["shapes"]["images"] == [4, 16, 16, 3]
        assert a.min() >= 0 and a.max() <= 255 and np.array_equal(a, np.round(a))
        arrs.append(a)
    assert np.array_equal(arrs[0], arrs[1])


def test_dump_outputs_samples_above_the_size_budget(tmp_path, monkeypatch):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import bench
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 2 * 4 * 100)       # 100 float32 per file
    big = torch.arange(1000, dtype=torch.float32).reshape(10, 100)
    small = torch.arange(12, dtype=torch.uint8).reshape(3, 4)
    shapes = bench.dump_outputs(str(tmp_path), {"big": big, "small": small})
    assert shapes == {"big": [100], "small": [3, 4]}
    b = np.load(tmp_path / "big.npy")
    assert b.dtype == np.float32 and len(set(b.tolist())) == 100 and np.all(np.diff(b) > 0)
    bench.dump_outputs(str(tmp_path / "again"), {"big": big, "small": small})
    assert np.array_equal(b, np.load(tmp_path / "again" / "big.npy"))       # the same sample every time
    s = np.load(tmp_path / "small.npy")
    assert s.dtype == np.float32 and np.array_equal(s, small.numpy())


def test_bench_world_size_mismatch_fails():
    r = _run(["--gpus", "2", "--model", "tiny", "--steps", "1", "--warmup", "0", "--no-score"],
             env_extra={"WORLD_SIZE": "1", "RANK": "0"}, timeout=120)
    assert r.returncode == 2
    assert "disagrees" in r.stderr


def test_bench_failing_rank_fails_the_job():
    # an unknown model raises in every rank: the launcher must exit non-zero, not hang, and
    # print ONE failure record (value null) naming the ranks' errors
    r = _run(["--gpus", "2", "--model", "nope", "--steps", "1", "--warmup", "0", "--no-score"], timeout=120)
    assert r.returncode != 0
    lines = _json_lines(r.stdout)
    assert len(lines) == 1 and lines[0]["value"] is None, r.stdout
    assert "KeyError" in lines[0]["error"] and "comm" not in lines[0]


def test_launcher_never_touches_hip():
    """verdict r5 item 5: the launcher counts GPUs without HIP (visibility variables / KFD sysfs).
    With every torch device-count entry point made to raise, ``--gpus 2`` still launches."""
    code = ("import sys, torch\n"
            "def boom(*a, **k):\n    raise AssertionError('launcher touched the GPU runtime')\n"
            "torch.cuda.device_count = boom\ntorch.cuda.is_available = boom\n"
            "torch._C._cuda_getDeviceCount = boom\n"
            f"sys.path.insert(0, {ROOT!r})\n"
            "import bench\n"
            "sys.argv = ['bench.py', '--gpus', '2', '--model', 'tiny', '--steps', '1', '--warmup', '0', '--no-score']\n"
            "sys.exit(bench.main())\n")
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env["CUDA_VISIBLE_DEVICES"] = ""
    env["HIP_VISIBLE_DEVICES"] = ""
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    out = _json_lines(r.stdout)
    assert len(out) == 1 and out[0]["n_gpus"] == 2 and out[0]["value"] > 0


def test_visible_gpu_count_from_env(monkeypatch):
    sys.path.insert(0, ROOT)
    import bench
    for v in ("HIP_VISIBLE_DEVICES", "ROCR_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"):
        monkeypatch.delenv(v, raising=False)
    monkeypatch.setenv("ROCR_VISIBLE_DEVICES", "0,1,2,3")
    assert bench._visible_gpus() == 4
    monkeypatch.setenv("HIP_VISIBLE_DEVICES", "")
    assert bench._visible_gpus() == 0


@pytest.mark.parametrize("mode,extra", [("raise", []), ("hang", ["--comm-timeout-s", "5"])])
def test_injected_process_group_init_failure_is_bounded(mode, extra):
    """verdict r5 item 5: a rank whose process-group init fails (or wedges) ends the job with a
    non-zero exit and ONE JSON line carrying ``comm.error``, within 60 s."""
    import time
    t0 = time.monotonic()
    r = _run(["--gpus", "2", "--model", "tiny", "--steps", "1", "--warmup", "0", "--no-score", *extra],
             env_extra={"CASSMANTLE_FAULT_DIST_INIT": mode, "CASSMANTLE_FAULT_DIST_RANKS": "1"}, timeout=120)
    took = time.monotonic() - t0
    assert r.returncode != 0 and took < 60, (r.returncode, took, r.stderr[-2000:])
    lines = _json_lines(r.stdout)
    assert len(lines) == 1 and lines[0]["value"] is None, r.stdout
    rec = lines[0]
    assert rec["comm"]["world_size"] == 2 and rec["comm"]["backend"] == "gloo"
    if mode == "raise":
        assert "injected process-group init failure on rank 1" in rec["comm"]["error"], rec
    else:                                       # a rank's init bound fired (both ranks arm it:
        # the wedged rank 1 and rank 0 waiting on it expire ~together; the first report wins)
        assert "comm-init" in rec["error"], rec
        assert any(f"rank {r}: comm-init" in rec["comm"]["error"] for r in (0, 1)), rec


def test_bench_live_supervised_topology():
    """tools/bench_live.py --gpus 2: front-end + 2 supervised workers (gloo on the CPU), both
    rooms drawn every round while the front-end scores"""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env["CUDA_VISIBLE_DEVICES"] = ""
    env["HIP_VISIBLE_DEVICES"] = ""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bench_live.py"), "--gpus", "2", "--model", "tiny",
                        "--players", "4", "--seconds", "3", "--idle-s", "1"], capture_output=True, text=True,
                       timeout=400, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    out = _json_lines(r.stdout)[-1]
    assert out["topology"] == "supervised" and out["n_gpus"] == 2
    assert out["devices"] == ["cpu:0", "cpu:1"] and not out["retired"]
    assert out["rounds"] >= 1 and out["images_per_s"] > 0 and out["requests"] > 0


def test_bench_oversubscribe_forces_gloo_and_refuses_nccl():
    r = _run(["--gpus", "2", "--oversubscribe", "--model", "tiny", "--steps", "1", "--warmup", "0", "--no-score"])
    assert r.returncode == 0, r.stderr[-3000:]
    out = _json_lines(r.stdout)[0]
    assert out["comm"] == {"backend": "gloo", "world_size": 2, "oversubscribed": True}
    assert len(out["per_rank"]) == 2
    r = _run(["--gpus", "2", "--oversubscribe", "--model", "tiny", "--steps", "1", "--warmup", "0", "--no-score"],
             env_extra={"CASSMANTLE_DIST_BACKEND": "nccl"}, timeout=120)
    assert r.returncode == 2 and "refused" in r.stderr


def test_bench_under_torchrun_four_ranks():
    """The driver's multi-GPU launch shape (torch.distributed.run, 127.0.0.1 rendezvous, one rank
    per device, bench.py reading RANK / WORLD_SIZE from the env): 4 gloo ranks on the CPU, one
    JSON line from rank 0 with the whole-job aggregate."""
    from cassmantle_amd.parallel.supervisor import free_port
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env["CUDA_VISIBLE_DEVICES"] = ""
    env["HIP_VISIBLE_DEVICES"] = ""
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "4",
                        "--master-addr", "127.0.0.1", "--master-port", str(free_port()), os.path.join(ROOT, "bench.py"),
                        "--gpus", "4", "--model", "tiny", "--steps", "1", "--warmup", "1", "--no-score"],
                       capture_output=True, text=True, timeout=400, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = _json_lines(r.stdout)
    assert len(lines) == 1, r.stdout
    out = lines[0]
    assert out["n_gpus"] == 4 and out["steps"] == 1 and out["warmup"] == 1
    assert out["comm"]["world_size"] == 4 and out["comm"]["backend"] == "gloo"
    assert out["config"]["parallelism"] == "dp4 (rooms)" and out["config"]["global_batch"] == 16
    assert [p["rank"] for p in out["per_rank"]] == [0, 1, 2, 3]
    assert abs(out["value"] - 16 / (out["ms_per_step"] / 1e3)) / out["value"] < 0.01
