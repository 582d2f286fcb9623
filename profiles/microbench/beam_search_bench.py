"""Microbenchmark (measurement tooling): LSTMDecoder.beam_search_decode, batched and device-resident (lv_beam.hip through
engine.LSTMBeamSearcher) against the forced sentence-by-sentence route (LSTMDecoder.batched_beam = False: the reference's
procedure, every decision on the host).

    python profiles/microbench/beam_search_bench.py [--reps 3]          # A/B, wall times with a device synchronise either side
    python profiles/microbench/beam_search_bench.py --profile           # one batched call (under rocprofv3 --kernel-trace --stats)
    python profiles/microbench/beam_search_bench.py --summarise DB      # per-kernel table of that run's rocpd database (no GPU)

Workloads: the model of tests/golden/beam_yahoo_seeded.npz (Yahoo shape V 20001, ni 512, H 1024, nz 32; seed 53, weights
U(-0.05, 0.05), embeddings U(-1, 1), the </s> row of pred_linear x 6: sentences end after 12 words on average, one in 32 runs
the full 100 steps) at B = 1, 8, 32, 128 with K = 5, and the same recipe at the Yelp shape (V 19997) at B = 32.  z ~ N(0, I)
from Generator().manual_seed(9).
"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from vae_lagging_encoder_amd.factory import build_text_vae  # noqa: E402

NI, H, NZ, K = 512, 1024, 32, 5


def build(V, dev):
    vae = build_text_vae(V, NI, H, NZ, "cpu", seed=53, model_scale=0.05, emb_scale=1.0)
    with torch.no_grad():
        vae.decoder.pred_linear.weight[2] *= 6.0
    vae = vae.to(dev)
    vae.eval()
    return vae


def summarise(db):
    """Per-kernel totals of a rocprofv3 rocpd database."""
    import collections
    import re
    import sqlite3
    rows = sqlite3.connect(db).cursor().execute("select name, start, end from kernels order by start").fetchall()
    agg = collections.OrderedDict()
    for n, s, e in rows:
        m = re.search(r"(beam_\w+|gemm\w*|lstm\w*|embed\w*|tanh\w*|at::native::\w+|__amd_rocclr_\w+)", n)
        k = m.group(1) if m else n[:60]
        a = agg.setdefault(k, [0, 0.0, 1e30, 0.0])
        d = (e - s) / 1e3
        a[0] += 1
        a[1] += d
        a[2] = min(a[2], d)
        a[3] = max(a[3], d)
    tot = sum(a[1] for a in agg.values())
    print("%-40s %6s %12s %10s %10s %10s %6s" % ("kernel", "calls", "total_us", "avg_us", "min_us", "max_us", "pct"))
    for k, a in sorted(agg.items(), key=lambda kv: -kv[1][1]):
        print("%-40s %6d %12.1f %10.2f %10.2f %10.2f %6.2f" % (k, a[0], a[1], a[1] / a[0], a[2], a[3], 100 * a[1] / tot))
    sel = sum(a[1] for k, a in agg.items() if k.startswith("beam_chunk") or k.startswith("beam_merge"))
    print("selection (beam_chunk + beam_merge) %.1f us, all beam_ kernels %.1f us, everything %.1f us" % (
        sel, sum(a[1] for k, a in agg.items() if k.startswith("beam_")), tot))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--summarise", metavar="DB")
    a = ap.parse_args()
    if a.summarise:
        summarise(a.summarise)
        return
    dev = torch.device("cuda:0")
    z_all = torch.randn(128, NZ, generator=torch.Generator().manual_seed(9)).to(dev)

    def timed(dec, z, batched):
        dec.batched_beam = batched
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = dec.beam_search_decode(z, K)
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0), out

    vae = build(20001, dev)
    if a.profile:
        timed(vae.decoder, z_all[:32], True)
        print("profile pass: one batched call, Yahoo shape, B = 32, K = 5")
        return
    for shape, V, sizes in (("yahoo", 20001, (1, 8, 32, 128)), ("yelp", 19997, (32,))):
        if V != 20001:
            vae = build(V, dev)
        dec = vae.decoder
        for B in sizes:
            z = z_all[:B]
            for batched in (True, False):           # warm-up: code objects, workspaces, allocator
                timed(dec, z, batched)
            t = {True: [], False: []}
            for _ in range(a.reps):                 # alternate A / B
                for batched in (True, False):
                    t[batched].append(timed(dec, z, batched)[0])
            _, new = timed(dec, z, True)
            _, old = timed(dec, z, False)
            dec.batched_beam = True
            inew = dec.beam_search_decode(z, K, return_info=True)[1]              # untimed: the step counts of the workload
            same = sum(x == y for x, y in zip(new, old))
            mn, mo = statistics.median(t[True]), statistics.median(t[False])
            print("%-5s B %3d K %d: batched %9.2f ms (min %.2f max %.2f) | per-sentence %9.2f ms (min %.2f max %.2f) | speed-up "
                  "%6.2fx | same sentences %d / %d | steps: sum %d, max %d" % (
                      shape, B, K, mn, min(t[True]), max(t[True]), mo, min(t[False]), max(t[False]), mo / mn, same, B,
                      int(inew["steps"].sum()), int(inew["steps"].max())))


if __name__ == "__main__":
    main()
