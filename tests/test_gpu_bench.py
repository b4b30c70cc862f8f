"""GPU: a plain `bench.py` run times exactly --steps steps, carries no extras, and --dump-outputs
writes the last timed step's transform (checked against the oracle)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_run_line_and_dump(tmp_path, oracle):
    import oracle as O
    log_n, steps = 14, 3
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", "1",
                        "--log-n", str(log_n), "--dump-outputs", str(tmp_path)], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["steps"] == steps and d["warmup"] == 1 and d["full"] is False and d["n_gpus"] == 1
    assert d["unit"] == "field-elems/s" and d["higher_is_better"] is True and d["dtype"] == "u32x8 (BN254 Fr)"
    assert d["ms_per_step"] > 0
    assert abs(d["value"] - (1 << log_n) / (d["ms_per_step"] / 1000.0)) <= 1e-6 * d["value"]
    # nothing beside the headline figure ran
    assert d["cpu_baseline"] is None and "cpu_baselines" not in d
    assert not [k for k in d if k.startswith(("merkle_", "fri_", "prove_", "verify_", "ntt_sweep", "power_"))]
    assert not [k for k in d if "bitexact" in k]
    # the dump: the whole 2^14-point output of the last of `steps` in-place transforms of the input
    n = 1 << log_n
    rows = np.load(tmp_path / "ntt_output_rows.npy")
    limbs = np.load(tmp_path / "ntt_output_u32_limbs.npy")
    assert rows.dtype == limbs.dtype == np.float64 and np.array_equal(rows, np.arange(n, dtype=np.float64))
    want = O.random_elements(n, 0x5EED0000 + log_n)
    w = O.root_of_unity(log_n)
    for _ in range(steps):
        want = oracle.best_fft(want, w, log_n, cpus=4)
    assert np.array_equal(np.ascontiguousarray(limbs.astype(np.uint32)).view(np.uint64), want)
