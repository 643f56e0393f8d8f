"""bench.py driver contract on the CPU plumbing path: the result line, the
--steps count, --full, and --dump-outputs (same arguments -> same inputs ->
on CPU bit-identical outputs)."""

import json
import subprocess
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
ARGS = ["--gpus", "1", "--device", "cpu", "--model", "gpt2-test",
        "--micro-batch", "2", "--seq", "16", "--steps", "3", "--warmup", "1"]


def _bench(*extra):
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), *ARGS, *extra],
                       cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_bench_result_line_and_dump(tmp_path):
    a = _bench("--dump-outputs", str(tmp_path / "a"))
    b = _bench("--full", "--dump-outputs", str(tmp_path / "b"))
    for res in (a, b):
        assert res["metric"] == "tokens/sec" and res["unit"] == "tokens/s"
        assert res["higher_is_better"] is True and res["dtype"] == "fp32"
        assert res["steps"] == 3 and res["ms_per_step"] > 0
        # value and ms_per_step describe the same timed interval
        tokens = res["config"]["global_batch"] * res["config"]["seq_len"]
        assert abs(res["value"] * res["ms_per_step"] / 1e3 / tokens - 1) < 1e-2
    names = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert names == ["loss.npy", "params_sample.npy"]
    total = 0
    for n in names:
        x, y = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert x.dtype in (np.float32, np.float64) and np.isfinite(x).all()
        assert x.size > 0 and np.array_equal(x, y), n
        total += x.nbytes
    assert total <= 64 << 20
    assert abs(float(np.load(tmp_path / "a" / "loss.npy")[0])
               - a["final_loss"]) < 1e-3
