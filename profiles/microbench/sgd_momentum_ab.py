"""Microbenchmark (measurement tooling): what optim.SGD's momentum (text.py --momentum) costs in the fused text trainer.

    python profiles/microbench/sgd_momentum_ab.py                      # both parts
    python profiles/microbench/sgd_momentum_ab.py --part kernel        # (a) only
    python profiles/microbench/sgd_momentum_ab.py --part trainer --momenta 0 --tree OTHER_CHECKOUT
                                                                       # (b) momentum 0 only, with the package of another checkout
                                                                       # (a commit without the momentum argument: the A of an A/B)

(a) the plain step kernel (lv_sgd_step_txn_f32) and the momentum step kernel (lv_sgd_momentum_step_txn_f32) on a buffer of the Yahoo
    encoder's flat size (16.6 M floats), clip inactive (coefficient 1: no gradient write-back) and active (0.5: the clipped gradient is
    written back), alternating in one process; per case the median over `reps` blocks of `iters` launches between two device events,
    as microseconds per launch and as GB/s over the streams the form touches (plain: p read + written, g read [+ written]; momentum:
    the same plus the velocity read + written).
(b) AggressiveTextTrainer encoder steps at the Yahoo shape (V 20001, ni 512, H 1024, nz 32, B 32, T 200, bf16 configuration, noise
    drawn on the device) with each momentum of --momenta, alternating in one process: `reps` blocks of `steps` steps each with a
    device synchronise either side; median, min and max of the blocks in ms per step.
"""
import argparse
import os
import statistics
import sys
import time

import torch


def kernel_part(a, dev):
    from vae_lagging_encoder_amd import engine as _eng
    from vae_lagging_encoder_amd.engine import P
    lib, s = _eng.backend_for(dev), _eng.stream_ptr(dev)
    n = 20001 * 512 + 4096 * 512 + 4096 * 1024 + 2 * 4096 + 64 * 1024          # the Yahoo encoder: embed, lstm ih / hh / biases, linear
    g = torch.Generator().manual_seed(0)
    p = torch.randn(n, generator=g).to(dev)
    gr0 = (torch.randn(n, generator=g) * 1e-3).to(dev)
    gr = gr0.clone()
    buf = torch.zeros(n, device=dev)
    sc = torch.tensor([1e-3, 1.0, 0.0], device=dev)                            # lr, coef, void flag

    def plain():
        lib.lv_sgd_step_txn_f32(P(p), P(gr), n, P(sc, 0), P(sc, 1), 1, P(sc, 2), s)

    def momentum():
        lib.lv_sgd_momentum_step_txn_f32(P(p), P(gr), P(buf), n, P(sc, 0), P(sc, 1), 0.9, 1, P(sc, 2), s)

    def block(fn):
        gr.copy_(gr0)                                                           # (an active clip scales g in place at every launch)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        e1.synchronize()
        return 1e3 * e0.elapsed_time(e1) / a.iters                              # us per launch
    print("(a) step kernels on %d floats (%.1f MB per stream), %d blocks of %d launches, alternating" % (n, 4e-6 * n, a.reps, a.iters))
    for label, coef in (("clip inactive", 1.0), ("clip active", 0.5)):
        sc[1] = coef
        streams = {"plain": 3 + (coef != 1.0), "momentum": 5 + (coef != 1.0)}
        for fn in (plain, momentum):
            block(fn)                                                           # warm-up
        t = {"plain": [], "momentum": []}
        for _ in range(a.reps):
            t["plain"].append(block(plain))
            t["momentum"].append(block(momentum))
        for k in ("plain", "momentum"):
            med = statistics.median(t[k])
            gbs = lambda us: streams[k] * 4.0 * n / (us * 1e-6) / 1e9
            # (the slowest block gives the lowest rate: GB/s min is from the max time and the other way round)
            print("    %-13s %-8s %7.1f us (min %.1f max %.1f) | %d streams | %6.0f GB/s (min %.0f max %.0f)" % (
                label, k, med, min(t[k]), max(t[k]), streams[k], gbs(med), gbs(max(t[k])), gbs(min(t[k]))), flush=True)
        buf.zero_()


def trainer_part(a, dev):
    from vae_lagging_encoder_amd.factory import build_text_vae, synthetic_batch
    from vae_lagging_encoder_amd.trainer import AggressiveTextTrainer
    V, ni, H, nz, B, T = 20001, 512, 1024, 32, 32, 200
    momenta = [float(v) for v in a.momenta.split(",")]
    batches = [synthetic_batch(B, T, V, seed=40 + i).to(dev) for i in range(4)]
    routes = []
    for mu in momenta:
        vae = build_text_vae(V, ni, H, nz, "cpu", seed=61, model_scale=0.05, emb_scale=0.1)
        with torch.no_grad():
            vae.encoder.linear.weight.uniform_(-0.2, 0.2)
        vae = vae.to(dev)
        vae.train()
        kw = {"momentum": mu} if mu != 0 else {}                                # (momentum 0 runs on a checkout without the argument too)
        tr = AggressiveTextTrainer(vae, lr=0.01, clip=5.0, precision="bf16", **kw)
        tr.prepare_batches(batches)
        routes.append((mu, tr))

    def block(tr, steps):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for i in range(steps):
            tr.step(batches[i % len(batches)], 0.5)
        torch.cuda.synchronize(dev)
        dt = 1e3 * (time.perf_counter() - t0) / steps
        tr.commit()
        return dt
    for _, tr in routes:
        block(tr, 12)                                                           # warm-up: code objects, workspaces, allocator
    t = {mu: [] for mu, _ in routes}
    for _ in range(a.reps):
        for mu, tr in routes:
            t[mu].append(block(tr, a.steps))
    print("(b) encoder steps, Yahoo shape (B %d, T %d, bf16 configuration), %d blocks of %d steps%s, package: %s" % (
        B, T, a.reps, a.steps, ", alternating" if len(routes) > 1 else "", a.tree or "this checkout"))
    rungs = {mu: tr.commit() for mu, tr in routes}                             # one host read each, before anything is formatted
    for mu, tr in routes:
        med = statistics.median(t[mu])
        print("    momentum %-4g %8.3f ms per step (min %.3f max %.3f, spread %.1f%%) | ladder rung %d" % (
            mu, med, min(t[mu]), max(t[mu]), 100.0 * (max(t[mu]) - min(t[mu])) / med, rungs[mu]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["both", "kernel", "trainer"], default="both")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--momenta", default="0,0.9")
    ap.add_argument("--tree", default=None, help="import the package from this checkout instead of the one the script is in")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree) if a.tree else os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    dev = torch.device("cuda:0")
    if a.part in ("both", "kernel"):
        kernel_part(a, dev)
    if a.part in ("both", "trainer"):
        trainer_part(a, dev)


if __name__ == "__main__":
    main()
