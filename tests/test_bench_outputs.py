"""bench.py's own contract on the CPU emulator (LVAE_BENCH_EMU=1: the kernel sources compiled for the host, device "cpu"): a plain run
prints the headline fields with `--steps` timed steps, and `--dump-outputs DIR` writes what the last timed step computed -- the same
arrays whether the run is plain or `--full`, so that two builds can be compared output by output."""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _run(tmp_path, name, *extra):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env["LVAE_BENCH_EMU"] = "1"
    out = tmp_path / name
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "2", "--warmup", "1", "--workload", "toy", "--dtype", "f32",
                        "--pool", "4", "--dump-outputs", str(out)] + list(extra), capture_output=True, text=True, env=env, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-1000:]
    return json.loads(lines[0]), out


def test_plain_run_line_and_dumped_outputs_match_the_full_run(tmp_path):
    line, plain = _run(tmp_path, "plain")
    assert line["metric"] == "aggressive-loop seqs/sec" and line["unit"] == "seq/s" and line["higher_is_better"] is True
    assert line["dtype"] == "f32" and line["steps"] == 2 and line["warmup"] == 1
    assert line["value"] > 0 and abs(line["value"] - 16 * 1e3 / line["ms_per_step"]) < 1e-3 * line["value"] + 0.01
    full_line, full = _run(tmp_path, "full", "--full")
    assert full_line["steps"] == 2
    names = sorted(os.listdir(plain))
    assert names == sorted(os.listdir(full))
    assert {"stats.npy", "loss.npy", "rec.npy", "kl.npy", "param.encoder.embed.weight.npy", "grad.decoder.pred_linear.weight.npy"} <= set(names)
    total = 0
    for f in names:
        a, b = np.load(plain / f), np.load(full / f)
        assert a.dtype == (np.float64 if f == "stats.npy" else np.float32), f
        assert np.array_equal(a, b), f
        total += a.nbytes
    assert total <= 64 << 20
    loss = np.load(plain / "loss.npy")
    assert loss.shape == (16,) and np.isfinite(loss).all()
