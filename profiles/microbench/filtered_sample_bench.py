"""Microbenchmark (measurement tooling): LSTMDecoder.sample_decode with temperature / top_k / top_p (lv_rollout_pick_filtered_f32, a
256-thread workgroup per row) against the same call with default arguments (lv_rollout_pick_f32's one-wave draw) and against
greedy_decode, all on the device route (engine.LSTMRollout).

    python profiles/microbench/filtered_sample_bench.py [--reps 7]    # host clock around one call (it ends in a device-to-host copy)
    python profiles/microbench/filtered_sample_bench.py --profile [--n 32]   # one call of each kind at one n (under rocprofv3 --kernel-trace --stats)
    python profiles/microbench/filtered_sample_bench.py --summarise DB   # per-kernel table of that run's rocpd database (no GPU)

Workload: rollout_bench.py's `noboost` model (Yahoo dimensions V 20001, ni 512, H 1024, nz 32; seed 53, weights U(-0.05, 0.05),
embeddings U(-1, 1); nothing ends early, so every call queues all 99 steps), z ~ N(0, I) from Generator().manual_seed(9), n = 1, 32,
256.  Every kind of call is warmed at every n, then the kinds alternate; the yardstick of a filtered call is the default
sample_decode of the SAME run.
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from rollout_bench import NZ, build, summarise  # noqa: E402

KINDS = [("sample", {}), ("greedy", None), ("top_k=40", {"top_k": 40}), ("top_p=0.9", {"top_p": 0.9}), ("temperature=0.7", {"temperature": 0.7})]


def summarise_picks(db):
    """rollout_bench's per-kernel table, then the filtered pick by kind: --profile launches the kinds in KINDS' order, 99 steps each."""
    import sqlite3
    summarise(db)
    rows = sqlite3.connect(db).cursor().execute("select name, start, end from kernels order by start").fetchall()
    d = [(e - s) / 1e3 for n, s, e in rows if "rollout_pick_filtered_kernel" in n]
    kinds = [k for k, kw in KINDS if kw]
    assert len(d) == 99 * len(kinds), len(d)
    for i, k in enumerate(kinds):
        part = d[99 * i:99 * (i + 1)]
        print("rollout_pick_filtered_kernel, %-16s: 99 calls, avg %7.2f us, min %7.2f, max %7.2f" % (
            k, sum(part) / 99, min(part), max(part)))
    for name in ("rollout_pick_sample_kernel", "rollout_pick_greedy_kernel"):
        part = [(e - s) / 1e3 for n, s, e in rows if name in n]
        print("%s: %d calls, avg %7.2f us, min %7.2f, max %7.2f" % (name, len(part), sum(part) / len(part), min(part), max(part)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--summarise", metavar="DB")
    ap.add_argument("--n", type=int, default=32, help="sentences of the --profile pass")
    a = ap.parse_args()
    if a.summarise:
        summarise_picks(a.summarise)
        return
    dev = torch.device("cuda:0")
    z_all = torch.randn(256, NZ, generator=torch.Generator().manual_seed(9)).to(dev)
    dec = build(dev, 1.0).decoder

    def call(z, kw):
        if kw is None:
            t0 = time.perf_counter()
            out = dec.greedy_decode(z)
        else:
            gen = torch.Generator(device=dev).manual_seed(3)
            t0 = time.perf_counter()
            out = dec.sample_decode(z, generator=gen, **kw)
        return 1e3 * (time.perf_counter() - t0), out

    if a.profile:
        for _, kw in KINDS:
            call(z_all[:a.n], kw)
        print("profile pass: one call each of %s on the device route, Yahoo shape, n = %d" % (", ".join(k for k, _ in KINDS), a.n))
        return
    assert a.reps >= 7
    for n in (1, 32, 256):
        for _, kw in KINDS:                             # warm-up of every kind at every shape: code objects, workspaces, allocator
            call(z_all[:n], kw)
    for n in (1, 32, 256):
        z = z_all[:n]
        t = {k: [] for k, _ in KINDS}
        words = {}
        for _ in range(a.reps):                         # alternate the kinds
            for k, kw in KINDS:
                ms, out = call(z, kw)
                t[k].append(ms)
                words[k] = max(len(s) for s in out)
        base = statistics.median(t["sample"])
        print("noboost n %3d | " % n + " | ".join(
            "%s %7.2f ms (min %.2f max %.2f)%s, longest %d" % (
                k, statistics.median(t[k]), min(t[k]), max(t[k]),
                "" if k in ("sample", "greedy") else " = %.2fx of sample" % (statistics.median(t[k]) / base), words[k])
            for k, _ in KINDS))


if __name__ == "__main__":
    main()
