"""Microbenchmark (measurement tooling): what the free-bits objective costs a fused training step.

    python profiles/microbench/free_bits_bench.py [--steps 20] [--out profiles/free_bits_bench.txt]

Two workloads, bench.py's shapes: the Yahoo-shaped text step (V 20001, ni 512, H 1024, nz 32, B 32, T 200; precision bf16, eager,
noise drawn on the device, encoder-only updates) and the Omniglot step (B 50, f32, eager).  Per workload four trainers in ONE
process -- free_bits None and the three modes at lambda = 0.05 -- each on its own, identically seeded model.  Every configuration
is warmed first; then 3 blocks, and inside a block the configurations alternate for 3 runs each (9 runs per configuration).  A run
is `--steps` steps between two device synchronisations on the host clock.  Reported: median, minimum and maximum of the per-step
time over the 9 runs, and the median's difference from free_bits None.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from vae_lagging_encoder_amd.factory import build_image_vae, build_text_vae, synthetic_batch  # noqa: E402
from vae_lagging_encoder_amd.trainer import AggressiveImageTrainer, AggressiveTextTrainer  # noqa: E402

LAM = 0.05
CONFIGS = [(None, "dim"), (LAM, "dim"), (LAM, "batch_dim"), (LAM, "batch")]
BLOCKS, RUNS = 3, 3


def text_runners(dev):
    V, ni, H, nz, B, T = 20001, 512, 1024, 32, 32, 200
    pool = [synthetic_batch(B, T, V, seed=7000 + i).to(dev) for i in range(16)]
    out = []
    for fb, mode in CONFIGS:
        vae = build_text_vae(V, ni, H, nz, dev, seed=783435)
        tr = AggressiveTextTrainer(vae, lr=1.0, clip=5.0, seed=783435, precision="bf16", free_bits=fb, free_bits_mode=mode)
        tr.prepare_batches(pool)
        rs = np.random.RandomState(783435)

        def run(n, tr=tr, rs=rs):
            for _ in range(n):
                tr.step(pool[int(rs.randint(0, len(pool)))], 0.1)
            tr.commit()
        out.append(run)
    return "text step, Yahoo shape (V 20001, ni 512, H 1024, nz 32, B 32, T 200), bf16, eager", out


def image_runners(dev):
    B = 50
    probs = torch.rand(8, B, 1, 28, 28, generator=torch.Generator().manual_seed(1)).to(dev)
    out = []
    for fb, mode in CONFIGS:
        vae = build_image_vae(dev, 783435)
        tr = AggressiveImageTrainer(vae, lr=1e-3, clip=5.0, seed=783435, precision="f32", free_bits=fb, free_bits_mode=mode)
        rs = np.random.RandomState(783435)

        def run(n, tr=tr, rs=rs):
            for _ in range(n):
                tr.step(tr.binarize(probs[int(rs.randint(0, 8))]), 1.0)
            tr.read_stats()
        out.append(run)
    return "image step, Omniglot (B 50), f32, eager", out


def measure(dev, name, runners, steps, lines):
    for run in runners:                                   # warm-up: code objects, workspaces, allocator
        run(3)
    torch.cuda.synchronize(dev)
    t = [[] for _ in runners]
    for _ in range(BLOCKS):
        for _ in range(RUNS):
            for i, run in enumerate(runners):
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                run(steps)
                torch.cuda.synchronize(dev)
                t[i].append(1e3 * (time.perf_counter() - t0) / steps)
    lines.append(name)
    base = statistics.median(t[0])
    for (fb, mode), ts in zip(CONFIGS, t):
        med = statistics.median(ts)
        label = "free_bits None            " if fb is None else "free_bits %.2f %-10s" % (fb, mode)
        lines.append("  %s %8.4f ms per step (min %.4f max %.4f) | median - None: %+8.1f us (%+.2f %%)"
                     % (label, med, min(ts), max(ts), 1e3 * (med - base), 100 * (med - base) / base))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "free_bits_bench.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "free_bits_bench.py measures on the MI355X"
    dev = torch.device("cuda:0")
    lines = ["# python profiles/microbench/free_bits_bench.py --steps %d   (one MI355X; lambda %.2f; configurations warmed, then "
             "alternating in %d blocks of %d runs of %d steps; host clock between device synchronisations)" % (a.steps, LAM, BLOCKS, RUNS,
                                                                                                               a.steps)]
    for build in (text_runners, image_runners):
        name, runners = build(dev)
        measure(dev, name, runners, a.steps, lines)
        del runners
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
