"""Microbenchmark (measurement tooling): what the importance-weighted objective and its doubly-reparameterised estimator cost in the
fused steps.

    python profiles/microbench/image_iw_bench.py [--reps 5] [--steps 10] [--out profiles/image_iw_bench.txt]
    python profiles/microbench/image_iw_bench.py --toy          # tiny text dims, argument parsing and shapes only (no GPU needed)

Image: one Omniglot step (ResNet encoder, PixelCNN decoder), B = 50, ns = 5, f32, eager and hipGraph; the three settings "elbo", "iw"
and "iw" + "dreg" on the same build.  Text: one step at the Yahoo shape (V 20001, T 200, ni 512, H 1024, nz 32), B = 32, ns = 4, f32
and bf16; "iw" against "iw" + "dreg".  Seeded weights and batches, noise drawn on the device.  Every shape is warmed up first (the
hipGraph route captures there); a timed block is `steps` steps with a device synchronise either side; `reps` blocks per setting, the
settings alternating in one process; median (min, max).  The lines are appended to --out; the bench.py lines of that file come from
runs of bench.py itself.
"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from vae_lagging_encoder_amd.factory import build_image_vae, build_text_vae, synthetic_batch  # noqa: E402
from vae_lagging_encoder_amd.trainer import AggressiveImageTrainer, AggressiveTextTrainer  # noqa: E402

SETTINGS = {"elbo": dict(objective="elbo"), "iw": dict(objective="iw"), "iw+dreg": dict(objective="iw", iw_estimator="dreg")}


def timed(step, batches, steps, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for i in range(steps):
        step(batches[i % len(batches)])
    torch.cuda.synchronize(dev)
    return 1e3 * (time.perf_counter() - t0) / steps


def fmt(ts):
    return "%8.3f ms (min %.3f max %.3f)" % (statistics.median(ts), min(ts), max(ts))


def alternate(steppers, batches, reps, steps, dev, warm):
    for st in steppers.values():
        timed(st, batches, warm, dev)
    t = {k: [] for k in steppers}
    for _ in range(reps):
        for k, st in steppers.items():
            t[k].append(timed(st, batches, steps, dev))
    return t


def image_lines(a, dev):
    B, ns = 50, 5
    g = torch.Generator().manual_seed(7)
    batches = [(torch.rand(B, 1, 28, 28, generator=g) < 0.35).float().to(dev) for _ in range(4)]
    lines = []
    for use_graph in (False, True):
        steppers = {}
        for name, kw in SETTINGS.items():
            tr = AggressiveImageTrainer(build_image_vae(dev, 61), lr=1e-3, clip=5.0, use_graph=use_graph, nsamples=ns, **kw)
            steppers[name] = (lambda tr_: (lambda x: tr_.step(x, 0.5)))(tr)
        t = alternate(steppers, batches, a.reps, a.steps, dev, warm=3)
        me = statistics.median(t["elbo"])
        lines.append("image f32 %-8s B %d ns %d: " % ("hipGraph" if use_graph else "eager", B, ns) + " | ".join(
            "%s %s" % (k, fmt(v)) for k, v in t.items()) + " | iw / elbo %.4f, iw+dreg / elbo %.4f, iw+dreg / iw %.4f" % (
            statistics.median(t["iw"]) / me, statistics.median(t["iw+dreg"]) / me, statistics.median(t["iw+dreg"]) / statistics.median(t["iw"])))
        print(lines[-1], flush=True)
        del steppers
        torch.cuda.empty_cache()
    return lines


def text_lines(a, dev, dims):
    V, T, ni, H, nz, B, ns = dims
    batches = [synthetic_batch(B, T, V, seed=40 + i).to(dev) for i in range(4)]
    lines = []
    for precision in ("f32", "bf16"):
        steppers, trs = {}, {}
        for name in ("iw", "iw+dreg"):
            vae = build_text_vae(V, ni, H, nz, "cpu", seed=61, model_scale=0.05, emb_scale=0.1)
            with torch.no_grad():
                vae.encoder.linear.weight.uniform_(-0.2, 0.2)
            vae = vae.to(dev)
            vae.train()
            tr = trs[name] = AggressiveTextTrainer(vae, lr=0.01, clip=5.0, precision=precision, nsamples=ns, **SETTINGS[name])
            tr.prepare_batches(batches)
            steppers[name] = (lambda tr_: (lambda x: tr_.step(x, 0.5)))(tr)
        t = alternate(steppers, batches, a.reps, a.steps, dev, warm=len(batches) + 1)
        lines.append("text %-4s V %d T %d H %d B %d ns %d: " % (precision, V, T, H, B, ns) + " | ".join("%s %s" % (k, fmt(v)) for k, v in t.items())
                     + " | iw+dreg / iw %.4f | ladder rung %d / %d" % (statistics.median(t["iw+dreg"]) / statistics.median(t["iw"]),
                                                                       trs["iw"].commit(), trs["iw+dreg"].commit()))
        print(lines[-1], flush=True)
        del steppers, trs
        torch.cuda.empty_cache()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--toy", action="store_true")
    ap.add_argument("--only", choices=["image", "text"], default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "image_iw_bench.txt"))
    a = ap.parse_args()
    dims = (211, 9, 16, 32, 8, 6, 4) if a.toy else (20001, 200, 512, 1024, 32, 32, 4)
    if not torch.cuda.is_available():
        if a.toy:
            print("toy pass without a GPU: settings %s; text dims %s" % (sorted(SETTINGS), dims))
            return
        raise SystemExit("no GPU: this is a measurement, it does not fall back")
    dev = torch.device("cuda:0")
    lines = ["python profiles/microbench/image_iw_bench.py --reps %d --steps %d      (one MI355X, one process, profiler off)" % (a.reps, a.steps),
             "alternating blocks of %d steps between two device synchronises, %d blocks per setting; median (min, max)." % (a.steps, a.reps), ""]
    if a.only != "text" and not a.toy:
        lines += image_lines(a, dev)
    if a.only != "image":
        lines += text_lines(a, dev, dims)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as fh:
        fh.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
