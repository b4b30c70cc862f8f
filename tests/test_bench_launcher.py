"""CPU: `bench.py --gpus N` starts its own one-rank-per-GPU launcher (torch.distributed.run as a
child process) when no launcher is around it, and refuses a world that differs from --gpus.
The rehearsal mode (--launch-check) rendezvous over gloo and all-reduces once, touching no GPU."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _env(**kw):
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(kw)
    return env


def test_self_launch_two_ranks_gloo():
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "2", "--launch-check"], cwd=ROOT,
                       env=_env(STARK_BENCH_BACKEND="gloo"), capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout            # rank 0 alone prints
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["ranks_in_all_reduce"] == 2


def test_world_mismatch_is_refused():
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "4", "--launch-check"], cwd=ROOT,
                       env=_env(WORLD_SIZE="2", RANK="0"), capture_output=True, text=True, timeout=120)
    assert r.returncode != 0
    assert "WORLD_SIZE=2 but --gpus 4" in r.stderr


def test_single_gpu_runs_in_process():
    r = subprocess.run([sys.executable, "bench.py", "--launch-check"], cwd=ROOT, env=_env(),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert json.loads(r.stdout.strip().splitlines()[-1])["n_gpus"] == 1


def test_plain_run_leaves_everything_else_to_full(monkeypatch):
    """A plain run times the headline steps alone; --full turns the extras and the CPU baselines on,
    and --no-extras / --no-cpu-baseline still take them out of a --full run."""
    sys.path.insert(0, ROOT)
    import bench

    def parsed(*argv):
        monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
        return bench.parse()
    a = parsed("--gpus", "1", "--steps", "7", "--warmup", "2")
    assert (a.steps, a.warmup, a.full, a.no_extras, a.no_cpu_baseline) == (7, 2, False, True, True)
    assert a.dump_outputs is None
    a = parsed("--full")
    assert a.full and not a.no_extras and not a.no_cpu_baseline
    a = parsed("--full", "--no-cpu-baseline", "--dump-outputs", "d")
    assert a.full and not a.no_extras and a.no_cpu_baseline and a.dump_outputs == "d"


def test_dump_outputs_fixed_sample_exact_in_float64(tmp_path):
    """--dump-outputs: the same rows every time, each row's eight 32-bit limbs exact in float64,
    well under 64 MB; a small output is written whole."""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench
    n = 2 * bench.DUMP_ROWS
    a = np.random.default_rng(7).integers(-2**63, 2**63 - 1, (n, 4), dtype=np.int64)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), torch.from_numpy(a), n)
    rows = np.load(tmp_path / "a" / "ntt_output_rows.npy")
    limbs = np.load(tmp_path / "a" / "ntt_output_u32_limbs.npy")
    assert rows.dtype == limbs.dtype == np.float64
    assert rows.shape == (bench.DUMP_ROWS,) and limbs.shape == (bench.DUMP_ROWS, 8)
    assert rows.nbytes + limbs.nbytes <= 64 << 20
    assert np.all(np.diff(rows) >= 0) and rows[0] >= 0 and rows[-1] < n
    assert np.array_equal(rows, np.load(tmp_path / "b" / "ntt_output_rows.npy"))
    assert np.array_equal(limbs, np.load(tmp_path / "b" / "ntt_output_u32_limbs.npy"))
    back = np.ascontiguousarray(limbs.astype(np.uint32)).view(np.int64)
    assert np.array_equal(back, a[rows.astype(np.int64)])
    bench.dump_outputs(str(tmp_path / "c"), torch.from_numpy(a[:5].copy()), 5)
    assert np.array_equal(np.load(tmp_path / "c" / "ntt_output_rows.npy"), np.arange(5.0))
    small = np.load(tmp_path / "c" / "ntt_output_u32_limbs.npy")
    assert np.array_equal(small.astype(np.uint32).view(np.int64), a[:5])


def test_distributed_roofline_fields():
    """The N > 1 line's roofline (bench.py distributed_roofline): the local kernels' 2 x 64 B per shard
    element against HBM and the all-to-all's (G-1)/G x 32 B per element against G-1 xGMI links, from
    the phase times; nothing taken from the 1-GPU profiles."""
    sys.path.insert(0, ROOT)
    import bench
    n, world = 1 << 24, 8
    ph = {"local_ms": 1.5, "exchange_ms": 0.5, "finish_ms": 0.25}
    r = bench.distributed_roofline(ph, n, world, 24, [8, 8, 8], on_gloo=False)
    assert r["bound"] == "hbm" and r["traffic"] is None and r["phases_ms"] == ph
    assert abs(r["achieved"] - 128.0 * n / 1.75e-3 / 1e9) < 0.01
    x = r["exchange"]
    assert x["bytes_per_rank"] == 7 / 8 * n * 32 and x["peak"] == 7 * bench.XGMI_LINK_GBS
    assert abs(x["achieved"] - x["bytes_per_rank"] / 0.5e-3 / 1e9) < 0.01
    assert "xGMI" in x["bound"]
    assert "not an xGMI figure" in bench.distributed_roofline(ph, n, 2, 24, [8, 8, 8], on_gloo=True)["exchange"]["bound"]
