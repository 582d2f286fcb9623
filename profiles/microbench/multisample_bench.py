"""Microbenchmark (measurement tooling): one training step with ns samples per sentence (text.py --nsamples), bf16 configuration --
the fused route (AggressiveTextTrainer(nsamples=ns): the word half of the decoder's input projection once per sentence) against
the drop-in route on the same tree (VAE.loss(x, w, nsamples=ns) under autograd: x, the dropout_in mask and z repeated onto the
ns = 1 engine, then optim.clip_grad_norm_ + optim.SGD), which is the only multi-sample route the library had before.

    python profiles/microbench/multisample_bench.py [--reps 3] [--steps 10]      # A/B, both routes alternating in one process
    python profiles/microbench/multisample_bench.py --profile                    # a few fused steps (under rocprofv3 --kernel-trace --stats)
    python profiles/microbench/multisample_bench.py --toy                        # tiny dims: argument parsing and shapes only

Workloads: Yahoo dims (V 20001, T 200) and Yelp dims (V 19997, T 100), ni 512, H 1024, nz 32, B = 32, ns in {1, 2, 4}; seeded
weights (scale 0.05, head 0.2), seeded synthetic batches, noise drawn on the device.  Every shape is warmed up first; a timed
block is `steps` steps with a device synchronise either side; `reps` blocks per route, alternating; min / median / max.
"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from vae_lagging_encoder_amd import optim as lvo  # noqa: E402
from vae_lagging_encoder_amd.factory import build_text_vae, synthetic_batch  # noqa: E402
from vae_lagging_encoder_amd.trainer import AggressiveTextTrainer  # noqa: E402


def build(V, ni, H, nz, dev):
    vae = build_text_vae(V, ni, H, nz, "cpu", seed=61, model_scale=0.05, emb_scale=0.1)
    with torch.no_grad():
        vae.encoder.linear.weight.uniform_(-0.2, 0.2)
    vae = vae.to(dev)
    vae.train()
    return vae


class Fused(object):
    def __init__(self, V, ni, H, nz, dev, ns):
        self.vae = build(V, ni, H, nz, dev)
        self.tr = AggressiveTextTrainer(self.vae, lr=0.01, clip=5.0, precision="bf16", nsamples=ns)

    def prepare(self, batches):
        self.tr.prepare_batches(batches)

    def step(self, x):
        self.tr.step(x, 0.5)

    def finish(self):
        self.tr.commit()                     # one host read: raises if a step was voided and could not be replayed


class DropIn(object):
    def __init__(self, V, ni, H, nz, dev, ns):
        self.vae = build(V, ni, H, nz, dev)
        self.vae.encoder._hip.precision = self.vae.decoder._hip.precision = "bf16"
        self.ns = ns
        self.enc_opt = lvo.SGD(self.vae.encoder.parameters(), lr=0.01, momentum=0)
        self.dec_opt = lvo.SGD(self.vae.decoder.parameters(), lr=0.01, momentum=0)

    def prepare(self, batches):
        pass

    def step(self, x):
        self.enc_opt.zero_grad()
        self.dec_opt.zero_grad()
        loss, _, _ = self.vae.loss(x, 0.5, nsamples=self.ns)
        loss.mean(dim=-1).backward()
        lvo.clip_grad_norm_(self.vae.parameters(), 5.0)
        self.enc_opt.step()

    def finish(self):
        pass


def timed(route, batches, steps, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for i in range(steps):
        route.step(batches[i % len(batches)])
    torch.cuda.synchronize(dev)
    dt = 1e3 * (time.perf_counter() - t0) / steps
    route.finish()
    return dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--toy", action="store_true")
    a = ap.parse_args()
    if a.toy:
        shapes, (ni, H, nz, B) = (("toy", 211, 9),), (16, 32, 8, 6)
    else:
        shapes, (ni, H, nz, B) = (("yahoo", 20001, 200), ("yelp", 19997, 100)), (512, 1024, 32, 32)
    if a.toy and not torch.cuda.is_available():
        print("toy pass without a GPU: shapes only")
        for name, V, T in shapes:
            for ns in (1, 2, 4):
                print("%-5s V %d T %d B %d ns %d: decoder rows %d" % (name, V, T, B, ns, B * ns))
        return
    dev = torch.device("cuda:0")
    for name, V, T in shapes:
        batches = [synthetic_batch(B, T, V, seed=40 + i).to(dev) for i in range(4)]
        for ns in (1, 2, 4):
            if a.profile and (name, ns) != (shapes[0][0], 4):
                continue
            fused = Fused(V, ni, H, nz, dev, ns)
            fused.prepare(batches)
            if a.profile:
                timed(fused, batches, 2, dev)
                ms = timed(fused, batches, 5, dev)
                print("profile pass: 2 + 5 fused steps, %s dims, B = %d, ns = %d: %.3f ms per step" % (name, B, ns, ms))
                continue
            dropin = DropIn(V, ni, H, nz, dev, ns)
            for r in (fused, dropin):                          # warm-up: code objects, workspaces of every shape, allocator
                timed(r, batches, len(batches) + 1, dev)
            t = {"fused": [], "dropin": []}
            for _ in range(a.reps):                            # alternate A / B
                t["fused"].append(timed(fused, batches, a.steps, dev))
                t["dropin"].append(timed(dropin, batches, a.steps, dev))
            mf, md = statistics.median(t["fused"]), statistics.median(t["dropin"])
            print("%-5s B %d ns %d T %d: fused %8.3f ms (min %.3f max %.3f) | drop-in %8.3f ms (min %.3f max %.3f) | drop-in / fused %5.2fx | "
                  "fused: %8.0f sentences/s, %8.0f decoder rows/s | ladder rung %d" % (
                      name, B, ns, T, mf, min(t["fused"]), max(t["fused"]), md, min(t["dropin"]), max(t["dropin"]), md / mf,
                      1e3 * B / mf, 1e3 * B * ns / mf, fused.tr.commit()), flush=True)
            del fused, dropin
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
