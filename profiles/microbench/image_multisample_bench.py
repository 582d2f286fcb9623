"""Microbenchmark (measurement tooling): one Omniglot training step with ns samples per image (image.py --nsamples) -- the fused
route (AggressiveImageTrainer(nsamples=ns), hipGraph on), the same with bn_partial_cap = inf (past 1024 partial rows the BatchNorm
fusions are dropped: what the library did before the finish-then-apply route), and the drop-in route on the same tree
(VAE.loss(x, w, nsamples=ns) under autograd with x.repeat_interleave(ns), torch's clip and torch's Adam).

    python profiles/microbench/image_multisample_bench.py [--reps 5] [--steps 10]      # A/B/C, the routes alternating in one process
    python profiles/microbench/image_multisample_bench.py --profile                    # five fused ns = 4 steps (under rocprofv3 --kernel-trace --stats)
    python profiles/microbench/image_multisample_bench.py --toy                        # the shape table only (no GPU needed)

B = 50 (image.py's batch), ns in {1, 2, 3, 4, 5}, precisions "f32" and "bf16x3"; seeded weights, seeded binarised batches, noise drawn
on the device (the drop-in route draws it with torch).  Every shape is warmed up first (the fused routes capture their graph there); a
timed block is `steps` steps with a device synchronise either side; `reps` blocks per route, alternating; median with min / max.
"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from vae_lagging_encoder_amd import _lib  # noqa: E402
from vae_lagging_encoder_amd.factory import build_image_vae  # noqa: E402
from vae_lagging_encoder_amd.trainer import AggressiveImageTrainer  # noqa: E402

B = 50


class Fused(object):
    def __init__(self, dev, ns, precision, cap=None, use_graph=True):
        self.vae = build_image_vae(dev, 61)
        self.tr = AggressiveImageTrainer(self.vae, lr=1e-3, clip=5.0, precision=precision, use_graph=use_graph, nsamples=ns)
        if cap is not None:
            self.tr.enc.bn_partial_cap = self.tr.dec.bn_partial_cap = cap

    def step(self, x):
        self.tr.step(x, 0.5)


class DropIn(object):
    def __init__(self, dev, ns, precision):
        self.vae = build_image_vae(dev, 61)
        self.vae.encoder._hip.precision = self.vae.decoder._hip.precision = precision
        self.ns = ns
        self.enc_opt = torch.optim.Adam(self.vae.encoder.parameters(), lr=1e-3)
        self.dec_opt = torch.optim.Adam(self.vae.decoder.parameters(), lr=1e-3)

    def step(self, x):
        self.enc_opt.zero_grad()
        self.dec_opt.zero_grad()
        loss, _, _ = self.vae.loss(x, 0.5, nsamples=self.ns)
        loss.mean(dim=-1).backward()
        torch.nn.utils.clip_grad_norm_(self.vae.parameters(), 5.0)
        self.enc_opt.step()


def timed(route, batches, steps, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for i in range(steps):
        route.step(batches[i % len(batches)])
    torch.cuda.synchronize(dev)
    return 1e3 * (time.perf_counter() - t0) / steps


def fmt(ts):
    return "%8.3f ms (min %.3f max %.3f)" % (statistics.median(ts), min(ts), max(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--ns", type=int, nargs="*", default=[1, 2, 3, 4, 5])
    ap.add_argument("--precisions", nargs="*", default=["f32", "bf16x3"])
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--toy", action="store_true")
    a = ap.parse_args()
    lib = _lib.load()
    if a.toy:
        for ns in a.ns:
            n = B * ns
            print("B %d ns %d: %d decoder images, tap split %d, masked-convolution rows %d, pointwise rows %d" % (
                B, ns, n, lib.lv_conv32_tap_split(n), lib.lv_conv32_blocks(n), lib.lv_conv1x1_blocks(784 * n)))
        return
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(7)
    batches = [(torch.rand(B, 1, 28, 28, generator=g) < 0.35).float().to(dev) for _ in range(4)]
    if a.profile:
        r = Fused(dev, 4, "f32", use_graph=False)
        timed(r, batches, 2, dev)
        ms = timed(r, batches, 5, dev)
        print("profile pass: 2 + 5 eager fused steps, B = %d, ns = 4, f32: %.3f ms per step; finish launches %s" % (B, ms, r.tr.dec.launches))
        return
    base = {}
    for precision in a.precisions:
        for ns in a.ns:
            n = B * ns
            rows32, rows1 = lib.lv_conv32_blocks(n), int(lib.lv_conv1x1_blocks(784 * n))
            routes = {"fused": Fused(dev, ns, precision)}
            if max(rows32, rows1) > 1024:                         # the cap only matters where a producer leaves more rows
                routes["fallback"] = Fused(dev, ns, precision, cap=float("inf"))
            routes["dropin"] = DropIn(dev, ns, precision)
            for r in routes.values():                             # warm-up: code objects, workspaces, allocator, graph capture
                timed(r, batches, 3, dev)
            t = {k: [] for k in routes}
            for _ in range(a.reps):                               # alternate the routes
                for k, r in routes.items():
                    t[k].append(timed(r, batches, a.steps, dev))
            mf = statistics.median(t["fused"])
            base.setdefault(precision, mf if ns == 1 else None)
            line = "%-6s B %d ns %d (%3d decoder images, rows %4d / %4d): fused %s" % (precision, B, ns, n, rows32, rows1, fmt(t["fused"]))
            if "fallback" in t:
                line += " | cap=inf %s, cap=inf / fused %5.3fx" % (fmt(t["fallback"]), statistics.median(t["fallback"]) / mf)
            line += " | drop-in %s, drop-in / fused %5.2fx | fused: %7.0f images/s, %7.0f decoder images/s" % (
                fmt(t["dropin"]), statistics.median(t["dropin"]) / mf, 1e3 * B / mf, 1e3 * n / mf)
            if base.get(precision):
                line += " (%.2f of ns = 1 per decoder image)" % ((1e3 * n / mf) / (1e3 * B / base[precision]))
            print(line, flush=True)
            del routes
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
