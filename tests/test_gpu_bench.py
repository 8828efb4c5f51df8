"""A plain bench.py run on a small window: the headline line only (nothing that `--full` adds), `steps` timed steps, and
`--dump-outputs` writing the last timed step's outputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("roofline", "phase_ms", "shard_emulation", "linearize_at_candidate", "host_placement", "cpu_baseline")


def test_plain_bench_line_and_dump(tmp_path):
    K, H, W, CS = 8, 64, 80, 32
    out_dir = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "1",
                        "--keyframes", str(K), "--height", str(H), "--width", str(W), "--cs", str(CS),
                        "--dump-outputs", str(out_dir)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert out["steps"] == 4 and out["warmup"] == 1 and out["n_gpus"] == 1
    assert out["unit"] == "Mresiduals/s" and out["higher_is_better"] is True and out["dtype"] == "f32"
    assert out["ms_per_step"] > 0 and out["value"] > 0
    assert abs(out["lm_iters_per_sec"] * out["ms_per_step"] - 1e3) < 1e-6 * 1e3
    assert not [k for k in FULL_ONLY if k in out]
    files = sorted(os.listdir(out_dir))
    assert files == sorted(f"{n}.npy" for n in ("lm_last_step", "poses", "codes", "scales", "delta", "normal_equations"))
    d = {f[:-4]: np.load(out_dir / f) for f in files}
    assert all(a.dtype in (np.float32, np.float64) and np.all(np.isfinite(a)) for a in d.values())
    assert d["poses"].shape == (K, 12) and d["codes"].shape == (K, CS) and d["scales"].shape == (K,)
    assert d["delta"].shape == (K * (7 + CS),) and d["lm_last_step"].shape == (4,)
    e0, e1, accepted, damp = d["lm_last_step"]
    assert e0 > 0 and accepted in (0.0, 1.0) and damp > 0
    assert d["normal_equations"].ndim == 1 and d["normal_equations"].size > K * (7 + CS) ** 2
