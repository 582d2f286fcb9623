"""Microbenchmark (measurement tooling): the model posterior on toy.py's latent grid, fused (lv_grid_posterior.hip) against the
forced generic route (VAE.fused_grid = False: the grid expanded to [B][K][nz], reconstruct_error on B*K rows, the lv_eval.hip
prior / log-sum-exp kernels).

    python profiles/microbench/grid_posterior_bench.py [--reps 9]       # A/B, median hipEvent times, outputs compared
    python profiles/microbench/grid_posterior_bench.py --profile        # fused route only (under rocprofv3 --kernel-trace --stats)
    python profiles/microbench/grid_posterior_bench.py --summarise DB   # per-kernel table of that run's rocpd database (no GPU)

Workloads (toy shape V 1004, ni = H = 50, nz 1; generate_grid(-20, 20, 0.1, ndim=1): K = 400; T = 12 tokens):
  multiple -- calc_model_posterior_mean over 500 sentences in torch.chunk(plot_data, round(500 / 16)) pieces (toy.py:188-214)
  single   -- one call on 50 sentences (toy.py:391-395, 453-462: after every decoder step of epoch 0)
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from vae_lagging_encoder_amd.factory import build_text_vae, synthetic_batch  # noqa: E402

PEAK_F32_MFMA = 157.3e12
V, NI, H, NZ, T = 1004, 50, 50, 1, 12


def flops(n_sent, K):
    """Useful multiply-adds of the decoder per sample-timestep (recurrence, vocabulary projection, z half of the input
    projection), x2; the per-sentence embedding half and the elementwise work are not counted."""
    per = 4 * H * H + V * H + 4 * H * NZ
    return 2.0 * per * n_sent * K * (T - 1)


def summarise(db):
    """Per-kernel totals of a rocprofv3 rocpd database, and the fused kernel's rate on the profile pass's workloads."""
    import collections
    import re
    import sqlite3
    rows = sqlite3.connect(db).cursor().execute("select name, start, end from kernels order by start").fetchall()
    agg = collections.OrderedDict()
    for n, s, e in rows:
        m = re.search(r"(gp_\w+|at::native::\w+|__amd_rocclr_\w+)(<\d+>)?", n)
        k = (m.group(1) + (m.group(2) or "")) if m else n[:60]
        a = agg.setdefault(k, [0, 0.0, 1e30, 0.0])
        d = (e - s) / 1e3
        a[0] += 1
        a[1] += d
        a[2] = min(a[2], d)
        a[3] = max(a[3], d)
    tot = sum(a[1] for a in agg.values())
    print("%-32s %6s %12s %10s %10s %10s %6s" % ("kernel", "calls", "total_us", "avg_us", "min_us", "max_us", "pct"))
    for k, a in sorted(agg.items(), key=lambda kv: -kv[1][1]):
        print("%-32s %6d %12.1f %10.2f %10.2f %10.2f %6.2f" % (k, a[0], a[1], a[1] / a[0], a[2], a[3], 100 * a[1] / tot))
    K = 400
    fl = 3 * (flops(500, K) + flops(50, K))                    # the profile pass: 3 x (multiple + single)
    main_us = sum(a[1] for k, a in agg.items() if k.startswith("gp_cond_ll"))
    all_us = sum(a[1] for k, a in agg.items() if k.startswith("gp_"))
    print("useful FLOP of the pass %.3g: gp_cond_ll_kernel %.1f us -> %.2f TF/s (%.1f%% of %.0f TF); all three gp_ kernels "
          "%.1f us -> %.2f TF/s (%.1f%%)" % (fl, main_us, fl / main_us / 1e6, 100 * fl / (main_us * 1e-6) / PEAK_F32_MFMA,
                                             PEAK_F32_MFMA / 1e12, all_us, fl / all_us / 1e6,
                                             100 * fl / (all_us * 1e-6) / PEAK_F32_MFMA))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--summarise", metavar="DB")
    a = ap.parse_args()
    if a.summarise:
        summarise(a.summarise)
        return
    dev = torch.device("cuda:0")
    vae = build_text_vae(V, NI, H, NZ, dev, seed=1, model_scale=0.3, emb_scale=0.5)
    vae.eval()
    grid = torch.arange(-20, 20, 0.1).unsqueeze(1).to(dev)
    K = grid.shape[0]
    plot500 = synthetic_batch(500, T, V, seed=2).to(dev)
    chunks = torch.chunk(plot500, round(500 / 16))
    plot50 = plot500[:50].contiguous()
    work = {"multiple": lambda: [vae.calc_model_posterior_mean(c, grid) for c in chunks],
            "single": lambda: [vae.calc_model_posterior_mean(plot50, grid)]}
    n_sent = {"multiple": 500, "single": 50}

    if a.profile:
        with torch.no_grad():
            for name in ("multiple", "single"):
                for _ in range(3):
                    work[name]()
        torch.cuda.synchronize()
        print("profile pass: fused route, 3 x each workload")
        return

    def timed(name, fused):
        vae.fused_grid = fused
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = work[name]()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), torch.cat(out)

    print("chunks of the 500-sentence dump: %d (sizes %s)" % (len(chunks), sorted(set(c.shape[0] for c in chunks))))
    with torch.no_grad():
        for name in ("multiple", "single"):
            for fused in (True, False):             # warm-up: code objects, workspaces, allocator
                timed(name, fused)
            t = {True: [], False: []}
            for _ in range(a.reps):                 # alternate A / B
                for fused in (True, False):
                    ms, out = timed(name, fused)
                    t[fused].append(ms)
            _, a_out = timed(name, True)
            _, b_out = timed(name, False)
            mf, mg = statistics.median(t[True]), statistics.median(t[False])
            fl = flops(n_sent[name], K)
            print("%-8s fused %8.3f ms (min %.3f max %.3f) | generic %8.3f ms (min %.3f max %.3f) | speed-up %.2fx | "
                  "max |mean diff| %.2e | useful %.3g FLOP -> fused %.2f TF/s = %.1f%% of the %.0f TF f32 MFMA peak"
                  % (name, mf, min(t[True]), max(t[True]), mg, min(t[False]), max(t[False]), mg / mf,
                     float((a_out - b_out).abs().max()), fl, fl / (mf * 1e-3) / 1e12, 100 * fl / (mf * 1e-3) / PEAK_F32_MFMA,
                     PEAK_F32_MFMA / 1e12))


if __name__ == "__main__":
    main()
