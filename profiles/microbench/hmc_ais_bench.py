"""Hamiltonian transitions of VAE.nll_ais on one MI355X: what a leapfrog pass costs, and how tight the
estimate is against random-walk transitions at the same number of decoder evaluations.

    python profiles/microbench/hmc_ais_bench.py [--reps 3] [--blocks 3] [--out profiles/hmc_ais_bench.txt]

1. Cost.  Yahoo dims V 20001, ni 512, H 1024, nz 32, T 200; B 8 sentences x 16 chains = 128 decoder rows; both precisions.
   Three configurations alternate in `blocks` blocks of `reps` calls in one process, each warmed up first, host clock between
   two device synchronisations: nll_ais(transition="hmc") on the fused route (temps 3, leapfrog 3: 10 passes of one forward and
   one backward to z), the same on the generic route (fused_hmc = False), and refine_posterior on the same 128 rows (nsamples 16,
   steps 9: 10 forwards, 9 backwards to z) -- the session whose decoder launches a leapfrog pass repeats.
2. Tightness.  The seeded nz = 8 model of tests/golden/beam_mid.npz (V 1004, ni = H = 50), 6 sentences, 16 chains, three noise
   seeds: transition="rw" with 300 temperatures (301 decoder evaluations per chain) against transition="hmc" with 100
   temperatures of 3 leapfrog steps (301), both from the prior on the sigmoid schedule.  Reported, not judged.
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from vae_lagging_encoder_amd.factory import build_text_vae  # noqa: E402


def timed(dev, fn):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) * 1e3


def cost(a, dev, lines):
    V, ni, H, nz, B, C, T, N, L = 20001, 512, 1024, 32, 8, 16, 200, 3, 3
    vae = build_text_vae(V, ni, H, nz, dev, seed=783435)
    g = torch.Generator().manual_seed(20201)
    x = torch.randint(4, V, (B, T), generator=g, dtype=torch.int64)
    x[:, 0], x[:, -1] = 1, 2
    x = x.to(dev)
    noise = (torch.randn(B, C, nz, generator=g).to(dev), torch.randn(N, B, C, nz, generator=g).to(dev), torch.rand(N, B, C, generator=g).to(dev))
    eps = torch.randn(B, C, nz, generator=g).to(dev)
    passes = 1 + N * L

    def hmc(fused):
        vae.fused_hmc = fused
        return vae.nll_ais(x, chains=C, temps=N, noise=noise, transition="hmc", leapfrog=L, step_size=0.05, return_info=True)

    configs = (("hmc fused", lambda: hmc(True)), ("hmc generic", lambda: hmc(False)),
               ("svi_refine", lambda: vae.refine_posterior(x, steps=passes - 1, nsamples=C, noise=eps)))
    lines.append("# cost: V %d ni %d H %d nz %d T %d, B %d x %d chains = %d rows; %d passes per call; %d blocks of %d calls, alternating"
                 % (V, ni, H, nz, T, B, C, B * C, passes, a.blocks, a.reps))
    for prec in ("f32", "bf16"):
        vae.set_precision(prec)
        for _, fn in configs:
            for _ in range(2):
                fn()
        assert hmc(True)[1]["route"] == "hmc-fused" and hmc(False)[1]["route"] == "hmc-generic"
        rate = float(hmc(True)[1]["accept_rate"].mean())
        times = {name: [] for name, _ in configs}
        for _ in range(a.blocks):
            for name, fn in configs:
                for _ in range(a.reps):
                    times[name].append(timed(dev, fn))
        base = statistics.median(times["svi_refine"]) / passes
        lines.append("%s (acceptance of the timed chains %.2f):" % (prec, rate))
        for name, _ in configs:
            t = times[name]
            med = statistics.median(t)
            lines.append("  %-12s median %9.2f ms per call (min %9.2f max %9.2f, %d calls) | %7.2f ms per pass | relative to a svi_refine iteration: %.3f"
                         % (name, med, min(t), max(t), len(t), med / passes, med / passes / base))


def tightness(dev, lines):
    mid = np.load(os.path.join(ROOT, "tests", "golden", "beam_mid.npz"))
    V, ni, H, nz = (int(mid[k]) for k in ("V", "ni", "H", "nz"))
    params = {k[len("param/"):]: torch.from_numpy(mid[k]) for k in mid.files if k.startswith("param/")}
    vae = build_text_vae(V, ni, H, nz, dev, params=params)
    vae.eval()
    B, T, C = 6, 12, 16
    g = torch.Generator().manual_seed(119)
    x = torch.randint(4, V, (B, T), generator=g, dtype=torch.int64).to(dev)
    lines.append("# tightness: beam_mid model (V %d ni %d H %d nz %d), B %d T %d, %d chains, 301 decoder evaluations per chain, from the prior"
                 % (V, ni, H, nz, B, T, C))
    for seed in (1, 2, 3):
        for name, kw in (("rw  temps 300 std 0.3", dict(temps=300, std=0.3)),
                         ("hmc temps 100 L 3 step 0.3 fixed", dict(temps=100, transition="hmc", leapfrog=3, step_size=0.3)),
                         ("hmc temps 100 L 3 step 0.3 adapt (0.65, 0.02)", dict(temps=100, transition="hmc", leapfrog=3, step_size=0.3,
                                                                            adapt=(0.65, 0.02), step_bounds=(1e-3, 2.0)))):
            gen = torch.Generator(device=dev).manual_seed(seed)
            nll, info = vae.nll_ais(x, chains=C, generator=gen, return_info=True, **kw)
            eps = info.get("step_size")
            lines.append("  seed %d %-46s route %-11s mean log p^ %9.4f  mean se %.4f  acceptance %.3f  final step %s"
                         % (seed, name, info["route"], float(-nll.double().mean()), float(info["se"].mean()), float(info["accept_rate"].mean()),
                            "-" if eps is None else "%.3f .. %.3f" % (float(eps.min()), float(eps.max()))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("hmc_ais_bench.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    lines = ["# python profiles/microbench/hmc_ais_bench.py --reps %d --blocks %d   (one MI355X; host clock between device synchronisations)"
             % (a.reps, a.blocks)]
    tightness(dev, lines)
    cost(a, dev, lines)
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
