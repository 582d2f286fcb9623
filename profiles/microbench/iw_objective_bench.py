"""Microbenchmark (measurement tooling): one fused training step on the importance-weighted bound (AggressiveTextTrainer(objective="iw"))
against the same step on the ELBO (objective="elbo") on the same build -- the two differ in two small launches (loss assembly, encoder
head backward) -- and the measured error delta of a within-sentence difference of log w against the reference run of
tests/golden/text_iw_h1024_b8_t50.npz, exact-f32 and bf16 configuration.

    python profiles/microbench/iw_objective_bench.py [--reps 5] [--steps 10] [--out profiles/iw_objective_bench.txt]
    python profiles/microbench/iw_objective_bench.py --profile       # a few bf16 "iw" steps (under rocprofv3 --kernel-trace --stats)
    python profiles/microbench/iw_objective_bench.py --toy           # tiny dims: argument parsing and shapes only

Workload: Yahoo dims (V 20001, T 200, ni 512, H 1024, nz 32), B = 32, ns = 4; seeded weights (scale 0.05, head 0.2), seeded synthetic
batches, noise drawn on the device.  Every shape is warmed up first; a timed block is `steps` steps with a device synchronise either
side; `reps` blocks per objective, alternating; median (min, max).
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
from vae_lagging_encoder_amd.factory import build_text_vae, synthetic_batch  # noqa: E402
from vae_lagging_encoder_amd.trainer import AggressiveTextTrainer  # noqa: E402


def build(V, ni, H, nz, dev):
    vae = build_text_vae(V, ni, H, nz, "cpu", seed=61, model_scale=0.05, emb_scale=0.1)
    with torch.no_grad():
        vae.encoder.linear.weight.uniform_(-0.2, 0.2)
    vae = vae.to(dev)
    vae.train()
    return vae


def timed(tr, batches, steps, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for i in range(steps):
        tr.step(batches[i % len(batches)], 0.5)
    torch.cuda.synchronize(dev)
    dt = 1e3 * (time.perf_counter() - t0) / steps
    tr.commit()                              # one host read: raises if a step was voided and could not be replayed
    return dt


def measured_delta(dev, precision):
    """One "iw" step on the wide reference fixture -> (delta, cap, loss error): delta = the largest error of a within-sentence
    difference log w_s - log w_s' against the reference run; cap = 1e-4 * max|rec|."""
    fx = np.load(os.path.join(ROOT, "tests", "golden", "text_iw_h1024_b8_t50.npz"))
    V, ni, H, nz, B, T, ns = (int(fx[k]) for k in ("V", "ni", "H", "nz", "B", "T", "ns"))
    vae = build_text_vae(V, ni, H, nz, "cpu", seed=int(fx["model_seed"]), model_scale=float(fx["model_scale"]), emb_scale=float(fx["emb_scale"]))
    with torch.no_grad():                    # the redraws the fixture script applied, in its order
        vae.encoder.linear.weight.uniform_(-float(fx["head_scale"]), float(fx["head_scale"]))
        vae.decoder.pred_linear.weight.uniform_(-float(fx["pred_scale"]), float(fx["pred_scale"]))
    vae = vae.to(dev)
    vae.train()
    unpack = lambda k: torch.from_numpy(np.unpackbits(fx[k + "_bits"])[:int(np.prod(fx[k + "_shape"]))].reshape(tuple(fx[k + "_shape"])))
    noise = (torch.from_numpy(fx["eps"]).to(dev), unpack("mask_in").to(dev), unpack("mask_out").to(dev))
    tr = AggressiveTextTrainer(vae, lr=1.0, clip=5.0, precision=precision, nsamples=ns, objective="iw")
    tr.step(torch.from_numpy(fx["x"]).to(dev), float(fx["kl_weight"]), noise=noise)
    st = tr.read_stats()
    d = tr.static[(B, T)].logw.cpu().double() - torch.from_numpy(fx["logw"]).double()
    delta = float((d.unsqueeze(2) - d.unsqueeze(1)).abs().max())
    return delta, 1e-4 * float(np.abs(fx["rec"]).max()), abs(st["loss_sum"] - float(fx["loss"].sum())) / abs(float(fx["loss"].sum()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--toy", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "iw_objective_bench.txt"))
    a = ap.parse_args()
    V, T, ni, H, nz, B, ns = (211, 9, 16, 32, 8, 6, 4) if a.toy else (20001, 200, 512, 1024, 32, 32, 4)
    if not torch.cuda.is_available():
        if a.toy:
            print("toy pass without a GPU: V %d T %d B %d ns %d: decoder rows %d, nll values per step %d" % (V, T, B, ns, B * ns, B * ns * (T - 1)))
            return
        raise SystemExit("no GPU: this is a measurement, it does not fall back")
    dev = torch.device("cuda:0")
    batches = [synthetic_batch(B, T, V, seed=40 + i).to(dev) for i in range(4)]
    if a.profile:
        tr = AggressiveTextTrainer(build(V, ni, H, nz, dev), lr=0.01, clip=5.0, precision="bf16", nsamples=ns, objective="iw")
        tr.prepare_batches(batches)
        timed(tr, batches, 2, dev)
        print("profile pass: 2 + 5 fused 'iw' steps, B = %d, ns = %d, T = %d: %.3f ms per step" % (B, ns, T, timed(tr, batches, 5, dev)))
        return
    lines = ["python profiles/microbench/iw_objective_bench.py --reps %d --steps %d      (one MI355X, one process, profiler off)" % (a.reps, a.steps),
             "One fused encoder step, V %d T %d ni %d H %d nz %d, B = %d, ns = %d, noise drawn on the device; objective \"iw\" against \"elbo\" on the"
             % (V, T, ni, H, nz, B, ns),
             "same build, alternating blocks of %d steps between two device synchronises, %d blocks each; median (min, max)." % (a.steps, a.reps), ""]
    for precision in ("f32", "bf16"):
        trs = {}
        for objective in ("elbo", "iw"):
            trs[objective] = AggressiveTextTrainer(build(V, ni, H, nz, dev), lr=0.01, clip=5.0, precision=precision, nsamples=ns, objective=objective)
            trs[objective].prepare_batches(batches)
            timed(trs[objective], batches, len(batches) + 1, dev)           # warm-up: code objects, workspaces of every shape, allocator
        t = {"elbo": [], "iw": []}
        for _ in range(a.reps):
            for objective in ("elbo", "iw"):
                t[objective].append(timed(trs[objective], batches, a.steps, dev))
        me, mi = statistics.median(t["elbo"]), statistics.median(t["iw"])
        lines.append("%-4s elbo %8.3f ms (min %.3f max %.3f) | iw %8.3f ms (min %.3f max %.3f) | iw / elbo %.4f | ladder rung %d / %d" % (
            precision, me, min(t["elbo"]), max(t["elbo"]), mi, min(t["iw"]), max(t["iw"]), mi / me, trs["elbo"].commit(), trs["iw"].commit()))
        print(lines[-1], flush=True)
        del trs
        torch.cuda.empty_cache()
    lines += ["", "delta: the largest error of a within-sentence difference log w_s - log w_s' of one \"iw\" step against the reference run",
              "(tests/golden/text_iw_h1024_b8_t50.npz: V 20001 H 1024, B 8, ns 4, T 50); the tests cap it at 1e-4 * max|rec|."]
    for precision in ("f32", "bf16"):
        delta, cap, loss_rel = measured_delta(dev, precision)
        lines.append("%-4s delta %.3e nats (cap %.3e: %s) | loss_sum relative error %.2e" % (precision, delta, cap, "inside" if delta < cap else "BROKEN",
                                                                                            loss_rel))
        print(lines[-1], flush=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
