"""Microbenchmark (measurement tooling): VAE.sample_from_posterior, the fused chain route (lv_mh_chain_f32: the whole chain on
the device, 16 chains of a sentence per workgroup) against the per-iteration route (VAE.fused_mh = False: one
eval_cond_ll + one lv_mh_step_f32 launch per iteration) on the same model.

    python profiles/microbench/mh_chain_bench.py [--reps 5] [--out profiles/mh_chain_bench.txt]

Shapes: the toy shape (V 1004, ni = H = 50, nz 1, T 12, B 16; seeded weights) and mid8 (tests/golden/beam_mid.npz's model:
V 1004, ni = H = 50, nz 8; B 6, T 12).  1 000 iterations (burn-in 100, thin 3, 300 samples), noise drawn by the method itself.
Route "chain" at chains = 1 and 16 and route "step" at chains = 1, alternating; median of hipEvent times.
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from vae_lagging_encoder_amd.factory import build_text_vae, synthetic_batch  # noqa: E402

BURN_IN, THIN, NSAMPLES, STD = 100, 3, 300, 0.3
ITERS = BURN_IN + THIN * NSAMPLES
T = 12


def models(dev):
    toy = build_text_vae(1004, 50, 50, 1, dev, seed=1, model_scale=0.3, emb_scale=0.5)
    mid = np.load(os.path.join(ROOT, "tests", "golden", "beam_mid.npz"))
    dims = [int(mid[k]) for k in ("V", "ni", "H", "nz")]
    params = {k[6:]: torch.from_numpy(mid[k]) for k in mid.files if k.startswith("param/")}
    mid8 = build_text_vae(*dims, dev, params=params)
    return (("toy  (V 1004, ni = H = 50, nz 1, B 16)", toy, 16, 1004), ("mid8 (V 1004, ni = H = 50, nz 8, B 6)", mid8, 6, dims[0]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mh_chain_bench.txt"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = ["# python profiles/microbench/mh_chain_bench.py --reps %d   (one MI355X; T %d, %d iterations: burn-in %d, thin %d, "
             "%d samples, std %.1f; median hipEvent times, configurations alternating)" % (a.reps, T, ITERS, BURN_IN, THIN, NSAMPLES, STD)]
    configs = (("chain", 1), ("chain", 16), ("step", 1))
    for name, vae, B, V in models(dev):
        vae.eval()
        x = synthetic_batch(B, T, V, seed=2).to(dev)

        def timed(route, chains):
            vae.fused_mh = route == "chain"
            gen = torch.Generator(device=dev).manual_seed(3)
            torch.manual_seed(3)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out, info = vae.sample_from_posterior(x, NSAMPLES, chains=chains, burn_in=BURN_IN, thin=THIN, std=STD, generator=gen,
                                                  return_info=True)
            e1.record()
            torch.cuda.synchronize()
            assert info["route"] == route and info["iterations"] == ITERS
            return e0.elapsed_time(e1), float(info["accept_rate"].mean())
        for c in configs:                              # warm-up: code objects, workspaces, allocator
            timed(*c)
        t = {c: [] for c in configs}
        rate = {}
        for _ in range(a.reps):
            for c in configs:
                ms, rate[c] = timed(*c)
                t[c].append(ms)
        lines.append(name)
        base = statistics.median(t[("step", 1)])
        for c in configs:
            ms = statistics.median(t[c])
            lines.append("  route %-5s chains %2d: %9.2f ms (min %.2f max %.2f) | %8.2f us per iteration | %10.0f chain-iterations/s | "
                         "acceptance %.2f | time relative to route step: %.3f"
                         % (c[0], c[1], ms, min(t[c]), max(t[c]), 1e3 * ms / ITERS, B * c[1] * ITERS / (ms * 1e-3), rate[c], ms / base))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
