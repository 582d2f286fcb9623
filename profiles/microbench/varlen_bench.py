"""Variable-length batches: the length-aware route (VarLSTMEncoder / VarLSTMDecoder, masked = True) against the by-length route
(masked = False: every group of equal length through the equal-length kernels, which is all there was before) on one MI355X.

    python profiles/microbench/varlen_bench.py [--reps 5] [--blocks 3] [--out profiles/varlen_bench.txt]

Shape: Yahoo dims V 20001, ni 512, H 1024, nz 32, B 32; lengths seeded uniform in [20, 200], sorted in decreasing order as
data_iter yields them; f32, dropout 0.5 / 0.5 drawn on the device.  Timed work: vae.loss((x, lens), 1.0)[0].mean().backward()
between two device synchronisations, host clock.  Both routes are warmed up, then alternate in `blocks` blocks of `reps` steps;
the equal-length T = 200 step (a plain [32][200] tensor through the same modules) is timed in the same blocks for scale.  Before
anything is timed the two routes are run on the same injected noise and must agree at 1e-4 (tests/parity_common.RTOL).
"""
import argparse
import statistics
import sys
import time

import os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import torch  # noqa: E402

from vae_lagging_encoder_amd.factory import build_text_vae  # noqa: E402

RTOL = 1e-4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--V", type=int, default=20001)
    ap.add_argument("--ni", type=int, default=512)
    ap.add_argument("--H", type=int, default=1024)
    ap.add_argument("--nz", type=int, default=32)
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--min-len", type=int, default=20)
    ap.add_argument("--max-len", type=int, default=200)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("varlen_bench.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    V, ni, H, nz, B = a.V, a.ni, a.H, a.nz, a.B
    vae = build_text_vae(V, ni, H, nz, dev, seed=783435, varlen=True)
    g = torch.Generator().manual_seed(20200)
    lens = sorted(torch.randint(a.min_len, a.max_len + 1, (B,), generator=g).tolist(), reverse=True)
    T = max(lens)
    x = torch.randint(4, V, (B, T), generator=g, dtype=torch.int64)
    x[:, 0] = 1
    for b, n in enumerate(lens):
        x[b, n - 1] = 2
        x[b, n:] = 0
    x = x.to(dev)
    lens_t = torch.tensor(lens, dtype=torch.int64)
    x_eq = torch.randint(4, V, (B, a.max_len), generator=g, dtype=torch.int64)
    x_eq[:, 0], x_eq[:, -1] = 1, 2
    x_eq = x_eq.to(dev)
    groups = len(set(lens))

    def set_masked(flag):
        vae.encoder.masked = vae.decoder.masked = flag

    def step(batch, noise=None):
        vae.zero_grad()
        out = vae.loss(batch, 1.0, noise=noise)
        out[0].mean().backward()
        return out

    # correctness first: the same injected noise through both routes
    noise = (torch.randn(B, 1, nz, generator=g).to(dev), (torch.rand(B, T - 1, ni, generator=g) < 0.5).to(torch.uint8).to(dev),
             (torch.rand(B, T - 1, H, generator=g) < 0.5).to(torch.uint8).to(dev))
    res = {}
    for flag in (True, False):
        set_masked(flag)
        loss, rec, kl = step((x, lens_t), noise)
        res[flag] = (loss.detach().cpu().double(), rec.detach().cpu().double(), kl.detach().cpu().double(),
                     {k: p.grad.detach().cpu().double().clone() for k, p in vae.named_parameters()})
    errs = [float((res[True][i] - res[False][i]).abs().max() / res[False][i].abs().max()) for i in range(2)]
    kl_err = float((res[True][2] - res[False][2]).abs().max() / (res[False][2].abs().max() + 1e-6 * (1 + float(res[False][1].abs().max()))))
    gerr = max(float((res[True][3][k] - res[False][3][k]).abs().max() / (res[False][3][k].abs().max() + 1e-30)) for k in res[True][3])
    assert max(errs) < RTOL and kl_err < RTOL, (errs, kl_err)

    routes = [("masked", lambda: (set_masked(True), step((x, lens_t)))), ("by-length", lambda: (set_masked(False), step((x, lens_t)))),
              ("equal T=%d" % a.max_len, lambda: step(x_eq))]
    for _ in range(2):                                   # warm-up: every shape of every route
        for _, fn in routes:
            fn()
    torch.cuda.synchronize(dev)
    times = {name: [] for name, _ in routes}
    for _ in range(a.blocks):
        for name, fn in routes:
            for _ in range(a.reps):
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize(dev)
                times[name].append((time.perf_counter() - t0) * 1e3)
    lines = ["# python profiles/microbench/varlen_bench.py --reps %d --blocks %d   (one MI355X; V %d ni %d H %d nz %d B %d; f32; dropout 0.5 / 0.5 "
             "drawn on the device; host clock between device synchronisations; routes alternating in %d blocks)" % (a.reps, a.blocks, V, ni, H, nz, B, a.blocks),
             "lengths uniform in [%d, %d], sorted: max %d, mean %.1f, %d tokens of %d padded positions, %d distinct lengths = groups of the by-length route"
             % (a.min_len, a.max_len, T, sum(lens) / B, sum(lens), B * T, groups),
             "timed: vae.loss((x, lens), 1.0)[0].mean().backward()",
             "agreement of the two routes on the same injected noise: loss %.1e rec %.1e kl %.1e, largest gradient difference %.1e (relative to the tensor's largest entry)"
             % (errs[0], errs[1], kl_err, gerr)]
    base = statistics.median(times["by-length"])
    for name, _ in routes:
        t = times[name]
        lines.append("  %-12s median %9.2f ms (min %9.2f max %9.2f, %d steps) | time relative to by-length: %.3f"
                     % (name, statistics.median(t), min(t), max(t), len(t), statistics.median(t) / base))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
