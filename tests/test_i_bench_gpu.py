"""bench.py's plain run (no --full) on one GPU: the headline fields of the one JSON line, --steps as the number of timed steps, and --dump-outputs -- what the last
timed step computed, equal from run to run although the clock conditioning in front of the warm-up runs a wall-clock-dependent number of SGD steps."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_plain_run_line_and_outputs_do_not_depend_on_the_conditioning(tmp_path):
    dumps = []
    for k, condition_ms in enumerate(("0", "60")):
        out = tmp_path / ("dump%d" % k)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2", "--batch", "64", "--pool", "256",
                            "--condition-ms", condition_ms, "--dump-outputs", str(out)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1, r.stdout[-2000:]
        d = json.loads(lines[0])
        assert d["steps"] == 3 and d["unit"] == "frames/s" and d["higher_is_better"] is True and d["dtype"] == "bf16"
        assert d["value"] == pytest.approx(64 * 3 / (d["ms_per_step"] * 3e-3), rel=1e-6)
        assert "roofline" not in d and "cpu_baseline" not in d              # --full only
        dumps.append({f.name: np.load(str(f)) for f in sorted(out.glob("*.npy"))})
    assert dumps[1]["losses.npy"].shape == (2,) and "vae.encoder.conv1.kernel.npy" in dumps[1] and sorted(dumps[0]) == sorted(dumps[1])
    assert sum(a.nbytes for a in dumps[1].values()) <= 64 << 20
    for name, a in dumps[1].items():
        assert a.dtype == np.float32 and np.isfinite(a).all() and np.array_equal(a, dumps[0][name]), name
