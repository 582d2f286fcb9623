"""Posterior refinement (VAE.refine_posterior): the fused route (engine.LSTMDecoderEngine.svi_refine) against the
generic route (fused_svi = False: reconstruct_error + the full autograd backward per iteration, which is all there was before) on
one MI355X.

    python profiles/microbench/svi_refine_bench.py [--reps 3] [--blocks 3] [--out profiles/svi_refine_bench.txt]
    python profiles/microbench/svi_refine_bench.py --trace-run f32      # a few fused iterations only: the program of a kernel-trace run

Shape: Yahoo dims V 20001, ni 512, H 1024, nz 32, B 32, T 200; K = 20 steps, ns = 1, injected noise; both precisions.  Timed
work: one refine_posterior call between two device synchronisations, host clock.  Both routes are warmed up, then alternate in
`blocks` blocks of `reps` calls in one process.  Before anything is timed the two routes must agree on the trace at 1e-4 (f32;
tests/parity_common.RTOL) -- the bf16 agreement is reported, not asserted.
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import torch  # noqa: E402

from vae_lagging_encoder_amd.factory import build_text_vae  # noqa: E402

RTOL = 1e-4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-run", default=None, choices=["f32", "bf16"])
    ap.add_argument("--V", type=int, default=20001)
    ap.add_argument("--ni", type=int, default=512)
    ap.add_argument("--H", type=int, default=1024)
    ap.add_argument("--nz", type=int, default=32)
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--T", type=int, default=200)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("svi_refine_bench.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    V, ni, H, nz, B, T, K = a.V, a.ni, a.H, a.nz, a.B, a.T, a.steps
    vae = build_text_vae(V, ni, H, nz, dev, seed=783435)
    g = torch.Generator().manual_seed(20201)
    x = torch.randint(4, V, (B, T), generator=g, dtype=torch.int64)
    x[:, 0], x[:, -1] = 1, 2
    x = x.to(dev)
    eps = torch.randn(B, 1, nz, generator=g).to(dev)

    def call(fused, steps=K):
        vae.fused_svi = fused
        return vae.refine_posterior(x, steps=steps, noise=eps, return_info=True)

    if a.trace_run:
        vae.set_precision(a.trace_run)
        call(True, 1)                                     # warm-up: workspaces, weight images
        torch.cuda.synchronize(dev)
        call(True, 3)
        torch.cuda.synchronize(dev)
        return
    lines = ["# python profiles/microbench/svi_refine_bench.py --reps %d --blocks %d   (one MI355X; V %d ni %d H %d nz %d B %d T %d; K = %d "
             "steps, ns = 1, injected noise; host clock between device synchronisations; routes alternating in %d blocks of %d calls)"
             % (a.reps, a.blocks, V, ni, H, nz, B, T, K, a.blocks, a.reps),
             "timed: vae.refine_posterior(x, steps=%d, noise=eps, return_info=True): %d decoder forwards, %d backwards to z" % (K, K + 1, K)]
    for prec in ("f32", "bf16"):
        vae.set_precision(prec)
        res = {}
        for fused in (True, False):
            for _ in range(2):                            # warm-up, and the agreement check on the second call's result
                res[fused] = call(fused)
        assert res[True][2]["route"] == "fused" and res[False][2]["route"] == "generic"
        tf, tg = res[True][2]["trace"].double(), res[False][2]["trace"].double()
        err = float((tf - tg).abs().max() / tg.abs().max())
        if prec == "f32":
            assert err < RTOL, err
        gap = float((res[True][2]["loss0"] - res[True][2]["loss"]).mean())
        torch.cuda.synchronize(dev)
        times = {True: [], False: []}
        for _ in range(a.blocks):
            for fused in (True, False):
                for _ in range(a.reps):
                    torch.cuda.synchronize(dev)
                    t0 = time.perf_counter()
                    call(fused)
                    torch.cuda.synchronize(dev)
                    times[fused].append((time.perf_counter() - t0) * 1e3)
        lines.append("%s: agreement of the two routes' traces %.1e (max-norm relative); mean gain of the refinement %.4f nats per sentence"
                     % (prec, err, gap))
        base = statistics.median(times[False])
        for fused, name in ((True, "fused"), (False, "generic")):
            t = times[fused]
            med = statistics.median(t)
            lines.append("  %-8s median %9.2f ms per call (min %9.2f max %9.2f, %d calls) | %7.2f ms per iteration | time relative to generic: %.3f"
                         % (name, med, min(t), max(t), len(t), med / K, med / base))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
