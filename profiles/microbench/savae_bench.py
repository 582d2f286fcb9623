"""Semi-amortized training (VAE.loss_savae): the fused route (engine.LSTMDecoderEngine.savae_forward /
savae_backward) against the generic route (fused_savae = False: reconstruct_error + torch.autograd.grad per pass) on one MI355X,
and beside them the fused trainers' steps: trainer.SemiAmortizedTextTrainer and an ordinary f32 AggressiveTextTrainer step with
update="both".

    python profiles/microbench/savae_bench.py [--reps 2] [--blocks 2] [--out profiles/savae_bench.txt]

Shape: Yahoo dims V 20001, ni 512, H 1024, nz 32, B 32, T 200; f32; K in {5, 20}; ns = 1, injected noise and masks.  Timed work:
zero_grad, loss_savae, loss.mean().backward() between two device synchronisations, host clock.  Both routes are warmed up, then
alternate in `blocks` blocks of `reps` calls in one process.  Before anything is timed the two routes must agree on the loss at
1e-4 (tests/parity_common.RTOL); their agreement on the gradients (worst tensor, max-norm relative) is reported.
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import torch  # noqa: E402

from vae_lagging_encoder_amd.factory import build_text_vae  # noqa: E402
from vae_lagging_encoder_amd.trainer import AggressiveTextTrainer, SemiAmortizedTextTrainer  # noqa: E402

RTOL = 1e-4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--blocks", type=int, default=2)
    ap.add_argument("--steps", type=int, nargs="+", default=[5, 20])
    ap.add_argument("--out", default=None)
    ap.add_argument("--V", type=int, default=20001)
    ap.add_argument("--ni", type=int, default=512)
    ap.add_argument("--H", type=int, default=1024)
    ap.add_argument("--nz", type=int, default=32)
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--T", type=int, default=200)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("savae_bench.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    V, ni, H, nz, B, T = a.V, a.ni, a.H, a.nz, a.B, a.T
    vae = build_text_vae(V, ni, H, nz, dev, seed=783435)
    vae.train()
    g = torch.Generator().manual_seed(20201)
    x = torch.randint(4, V, (B, T), generator=g, dtype=torch.int64)
    x[:, 0], x[:, -1] = 1, 2
    x = x.to(dev)
    noise = (torch.randn(B, 1, nz, generator=g).to(dev), (torch.rand(B, T - 1, ni, generator=g) < 0.5).to(torch.uint8).to(dev),
             (torch.rand(B, T - 1, H, generator=g) < 0.5).to(torch.uint8).to(dev))

    def call(fused, K):
        vae.fused_savae = fused
        vae.zero_grad()
        loss, rec, kl = vae.loss_savae(x, 1.0, svi_steps=K, noise=noise)
        loss.mean().backward()
        return loss.detach()

    def timed(fn):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) * 1e3

    def row(name, t, base, K):
        med = statistics.median(t)
        return ("  %-28s median %9.2f ms per step (min %9.2f max %9.2f, %d calls) | %7.2f ms per refinement step | relative to %s: %.3f"
                % (name, med, min(t), max(t), len(t), med / max(K, 1), base[0], med / base[1]))

    lines = ["# python profiles/microbench/savae_bench.py --reps %d --blocks %d   (one MI355X; f32; V %d ni %d H %d nz %d B %d T %d; ns = 1, "
             "injected noise and masks; host clock between device synchronisations; routes alternating in %d blocks of %d calls)"
             % (a.reps, a.blocks, V, ni, H, nz, B, T, a.blocks, a.reps),
             "timed: zero_grad; loss_savae(x, 1.0, svi_steps=K, noise=noise); loss.mean().backward()"]
    for K in a.steps:
        res = {}
        for fused in (True, False):
            for _ in range(2):                            # warm-up, and the agreement check on the second call's result
                res[fused] = (call(fused, K), {k: p.grad.detach().clone() for k, p in vae.named_parameters()})
        err = float((res[True][0] - res[False][0]).abs().max() / res[False][0].abs().max())
        assert err < RTOL, err
        gerr = max(float((res[True][1][k] - v).abs().max() / v.abs().max()) for k, v in res[False][1].items())
        times = {True: [], False: []}
        for _ in range(a.blocks):
            for fused in (True, False):
                for _ in range(a.reps):
                    times[fused].append(timed(lambda: call(fused, K)))
        lines.append("K = %d: agreement of the two routes: loss %.1e, gradients %.1e (max-norm relative, worst tensor)" % (K, err, gerr))
        base = ("generic", statistics.median(times[False]))
        lines.append(row("loss_savae fused", times[True], base, K))
        lines.append(row("loss_savae generic", times[False], base, K))
    # the fused trainers (weights move; lr tiny so that the workload stays the same)
    del vae.fused_savae
    plain = AggressiveTextTrainer(vae, lr=1e-6, clip=5.0, precision="f32")
    t_plain = [timed(lambda: plain.step(x, 1.0, noise=noise, update="both")) for _ in range(2 + a.reps * a.blocks)][2:]
    plain.commit()
    base = ("the ordinary step", statistics.median(t_plain))
    lines.append("fused trainers, step(x, 1.0, noise, update='both'):")
    lines.append(row("AggressiveTextTrainer f32", t_plain, base, 1))
    for K in a.steps:
        tr = SemiAmortizedTextTrainer(vae, svi_steps=K, lr=1e-6, clip=5.0)
        t = [timed(lambda: tr.step(x, 1.0, noise=noise)) for _ in range(1 + a.reps * a.blocks)][1:]
        st = tr.read_stats()
        n = 1 + a.reps * a.blocks
        lines.append(row("SemiAmortizedTextTrainer K=%d" % K, t, base, K))
        lines.append("      gap closed by the refinement: (loss0_sum - loss_sum) / sentences = %.4f nats" % ((st["loss0_sum"] - st["loss_sum"]) / (n * B)))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
