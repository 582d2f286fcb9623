"""Microbenchmark (measurement tooling): VAE.nll_ais, the fused chain route (lv_ais_chain_f32) and the per-iteration route
(VAE.fused_ais = False: one eval_cond_ll + one lv_ais_step_f32 launch per iteration), next to the baseline an AIS iteration
should cost: VAE.sample_from_posterior's chain route (lv_mh_chain_f32) at the same B, chains and iteration count, in the same
process -- an AIS iteration is the same gp_cond_nll plus O(nz) work.

    python profiles/microbench/ais_bench.py [--reps 5] [--out profiles/ais_bench.txt]

Shapes: the toy shape (V 1004, ni = H = 50, nz 1, T 12, B 16; seeded weights) and mid8 (tests/golden/beam_mid.npz's model:
V 1004, ni = H = 50, nz 8; B 6, T 12).  1 000 iterations (AIS: 1 000 temperatures, sigmoid schedule, prior init; MH: burn-in 100,
thin 3, 300 samples), noise drawn by the methods themselves.  Configurations alternating; median of hipEvent times.

Second part, recorded rather than asserted: on the nz = 1 model of tests/test_ais.py's truth test, log p^ from nll_ais (prior
init), nll_ais (encoder init) and nll_iw at an equal count of decoder evaluations per sentence, each next to the grid truth
(float64 oracle, z in [-8, 8], step 0.01).
"""
import argparse
import math
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import text_vae_oracle as O  # noqa: E402
from vae_lagging_encoder_amd.factory import build_text_vae, synthetic_batch  # noqa: E402

ITERS, STD = 1000, 0.3
BURN_IN, THIN, NSAMPLES = 100, 3, 300
T = 12


def models(dev):
    toy = build_text_vae(1004, 50, 50, 1, dev, seed=1, model_scale=0.3, emb_scale=0.5)
    mid = np.load(os.path.join(ROOT, "tests", "golden", "beam_mid.npz"))
    dims = [int(mid[k]) for k in ("V", "ni", "H", "nz")]
    params = {k[6:]: torch.from_numpy(mid[k]) for k in mid.files if k.startswith("param/")}
    mid8 = build_text_vae(*dims, dev, params=params)
    return (("toy  (V 1004, ni = H = 50, nz 1, B 16)", toy, 16, 1004), ("mid8 (V 1004, ni = H = 50, nz 8, B 6)", mid8, 6, dims[0]))


def speed(dev, reps, lines):
    configs = (("ais", "chain", 1), ("mh", "chain", 1), ("ais", "chain", 16), ("mh", "chain", 16), ("ais", "chain", 64),
               ("mh", "chain", 64), ("ais", "step", 16))
    for name, vae, B, V in models(dev):
        vae.eval()
        x = synthetic_batch(B, T, V, seed=2).to(dev)

        def timed(kind, route, chains):
            gen = torch.Generator(device=dev).manual_seed(3)
            torch.manual_seed(3)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            if kind == "ais":
                vae.fused_ais = route == "chain"
                e0.record()
                _, info = vae.nll_ais(x, chains=chains, temps=ITERS, std=STD, generator=gen, return_info=True)
            else:
                vae.fused_mh = True
                e0.record()
                _, info = vae.sample_from_posterior(x, NSAMPLES, chains=chains, burn_in=BURN_IN, thin=THIN, std=STD, generator=gen,
                                                    return_info=True)
            e1.record()
            torch.cuda.synchronize()
            assert info["route"] == route and info["iterations"] == ITERS
            return e0.elapsed_time(e1), float(info["accept_rate"].mean())
        for c in configs:                              # warm-up: code objects, workspaces, allocator
            timed(*c)
        t = {c: [] for c in configs}
        rate = {}
        for _ in range(reps):
            for c in configs:
                ms, rate[c] = timed(*c)
                t[c].append(ms)
        lines.append(name)
        for c in configs:
            ms = statistics.median(t[c])
            rel = ""
            if c[0] == "ais":
                base = statistics.median(t[("mh", "chain", c[2])])
                rel = " | time relative to sample_from_posterior, route chain, %d chains: %.3f" % (c[2], ms / base)
            lines.append("  %-3s route %-5s chains %2d: %9.2f ms (min %.2f max %.2f) | %8.2f us per iteration | %10.0f chain-iterations/s | "
                         "acceptance %.2f%s" % (c[0], c[1], c[2], ms, min(t[c]), max(t[c]), 1e3 * ms / ITERS,
                                                B * c[2] * ITERS / (ms * 1e-3), rate[c], rel))


def tightness(dev, lines):
    V, ni, H, nz, B, Tt, C, temps, std = 17, 4, 20, 1, 3, 7, 64, 200, 0.5
    Pm = O.random_params(V, ni, H, nz, seed=11, scale=1.0, emb_scale=0.5)
    x = O.synthetic_batch(B, Tt, V, seed=12)
    P64 = {k: v.double() for k, v in Pm.items()}
    grid = (torch.arange(1601, dtype=torch.float64) * 0.01 - 8.0).view(1, -1, 1).expand(B, -1, -1)
    prior = -0.5 * (grid * grid).sum(-1) - 0.5 * math.log(2 * math.pi)
    truth = torch.logsumexp(prior - O.decoder_reconstruct_error(P64, x, grid), dim=1) + math.log(0.01)
    vae = build_text_vae(V, ni, H, nz, dev, params=Pm)
    vae.eval()
    xd = x.to(dev)
    evals = C * (temps + 1)
    lines.append("tightness on the nz = 1 model of tests/test_ais.py (V 17, ni 4, H 20, B 3, T 7): %d decoder evaluations per sentence "
                 "(nll_ais: %d chains x (%d temperatures + z_0), std %.1f, sigmoid schedule; nll_iw: %d samples, 100 at a time); "
                 "3 seeds each" % (evals, C, temps, std, evals // 100 * 100))
    lines.append("  grid truth log p(x):            %s" % "  ".join("%9.4f" % v for v in truth.tolist()))
    for label, fn in (("nll_ais, prior init  ", lambda g: vae.nll_ais(xd, chains=C, temps=temps, std=std, generator=g, return_info=True)),
                      ("nll_ais, encoder init", lambda g: vae.nll_ais(xd, chains=C, temps=temps, std=std, init="encoder", generator=g,
                                                                      return_info=True)),
                      ("nll_iw               ", None)):
        for seed in (1, 2, 3):
            torch.manual_seed(seed)
            if fn is None:
                with torch.no_grad():
                    lp, extra = -vae.nll_iw(xd, nsamples=evals // 100 * 100, ns=100), ""
            else:
                nll, info = fn(torch.Generator(device=dev).manual_seed(seed))
                lp, extra = -nll, " | se %s | acceptance %.2f" % ("  ".join("%.4f" % v for v in info["se"].tolist()),
                                                                  float(info["accept_rate"].mean()))
            lines.append("  %s seed %d log p^: %s | log p^ - truth: %s%s"
                         % (label, seed, "  ".join("%9.4f" % v for v in lp.tolist()),
                            "  ".join("%+8.4f" % (a - b) for a, b in zip(lp.tolist(), truth.tolist())), extra))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ais_bench.txt"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = ["# python profiles/microbench/ais_bench.py --reps %d   (one MI355X; T %d, %d iterations, std %.1f; AIS: sigmoid schedule, "
             "prior init; MH: burn-in %d, thin %d, %d samples; median hipEvent times, configurations alternating)"
             % (a.reps, T, ITERS, STD, BURN_IN, THIN, NSAMPLES)]
    speed(dev, a.reps, lines)
    tightness(dev, lines)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
