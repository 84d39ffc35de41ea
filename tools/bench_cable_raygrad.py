#!/usr/bin/env python3
"""Times the ray-state adjoint of the fibre march (drrt_backtrace_cable_rays_f32, k_backtrace_cable_rays) on the workload
of tools/bench_cable.py -- 257-sample Luneburg-like profile, 4 194 304 rays x ~512 steps, closest approach to a target at
0.75 length -- next to the two kernels it goes with, in one process:

    trace_cable            TracerC.trace_cable            (k_trace_cable)
    backtrace_cable        TracerC.backtrace_cable        (k_backtrace_cable: dL/dn)
    backtrace_cable_rays   TracerC.backtrace_cable_rays   (k_backtrace_cable_rays: dL/dpos, dL/dvel; replay + reverse)

for rays in random order and in source-pixel order.  The three calls are timed alternately (one of each per round) with
device events around the whole call, so that drift of the machine hits all three alike.

usage: bench_cable_raygrad.py [--side 2048] [--rounds 7] [--warmup 2] [--once]
Prints one JSON object: per order and call the median, minimum and maximum ms over the rounds, the iteration counts
(stats.ray_steps), and the ratio of the new call to the sum of the two existing ones.  --once: a single call of each
(for a `rocprofv3 --kernel-trace --stats` run of its own)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from adjointnonlinearraytracing_amd import drrt  # noqa: E402


def rays(order, side, radius, ds, dev):
    n = side * side
    if order == "random":
        g = torch.Generator(device=dev).manual_seed(0)
        ang = torch.rand(n, device=dev, generator=g) * 6.2831853
        rad = 0.9 * radius * torch.sqrt(torch.rand(n, device=dev, generator=g))
        pos = torch.stack([radius + rad * torch.cos(ang), torch.full((n,), 0.37 * ds, device=dev),
                           radius + rad * torch.sin(ang)], -1)
        vel = torch.randn(n, 3, device=dev, generator=g) * 0.05
        vel[:, 1] = 1
        vel /= vel.norm(dim=1, keepdim=True)
        return pos.contiguous(), vel.contiguous()
    i = torch.arange(side, device=dev, dtype=torch.float32)
    X, Z = torch.meshgrid(i, i, indexing="ij")
    px = (X.flatten() + 0.5) / side * 2 * radius
    pz = (Z.flatten() + 0.5) / side * 2 * radius
    pos = torch.stack([px, torch.full((n,), 0.37 * ds, device=dev), pz], -1)
    vel = torch.zeros(n, 3, device=dev)
    vel[:, 1] = 1
    return pos.contiguous(), vel


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=2048, help="rays = side^2")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--once", action="store_true")
    a = ap.parse_args()
    if a.side < 1 or a.rounds < 1 or a.warmup < 0:
        ap.error("--side and --rounds must be positive, --warmup non-negative")
    if not torch.cuda.is_available():
        sys.exit("bench_cable_raygrad: needs a GPU")
    dev = torch.device("cuda:0")
    drrt.options.check_failed = False
    rres, radius = 257, 1.0
    ds = radius / (rres - 1) / 2
    length = 512 * ds
    prof = torch.sqrt(2.0 - torch.linspace(0, 1, rres) ** 2).to(dev)
    n = a.side * a.side
    tg = torch.tensor([[radius, 0.75 * length, radius]], device=dev).expand(n, 3).contiguous()
    T = drrt.TracerC()
    out = dict(rays=n, rres=rres, ds=ds, length=length, rounds=a.rounds)
    for order in ("random", "pixel"):
        pos, vel = rays(order, a.side, radius, ds, dev)
        xt, vt, _ = T.trace_cable(prof, radius, length, pos, vel, tg, ds)
        one = torch.ones_like(xt)
        calls = {
            "trace_cable": lambda: T.trace_cable(prof, radius, length, pos, vel, tg, ds),
            "backtrace_cable": lambda: T.backtrace_cable(prof, radius, length, xt, vt, one, one, ds),
            "backtrace_cable_rays": lambda: T.backtrace_cable_rays(prof, radius, length, pos, vel, tg, one, one, ds),
        }
        if a.once:
            for fn in calls.values():
                fn()
            torch.cuda.synchronize()
            continue
        steps, ms = {}, {k: [] for k in calls}
        for k, fn in calls.items():
            for _ in range(max(a.warmup, 1)):
                fn()
            steps[k] = drrt.read_stats()["ray_steps"]
        torch.cuda.synchronize()
        for _ in range(a.rounds):
            for k, fn in calls.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                ms[k].append(e0.elapsed_time(e1))
        res = {k: dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), ray_steps=steps[k])
               for k, v in ms.items()}
        both = [x + y for x, y in zip(ms["trace_cable"], ms["backtrace_cable"])]
        res["sum_existing_median_ms"] = statistics.median(both)
        res["new_over_sum_existing"] = statistics.median(ms["backtrace_cable_rays"]) / statistics.median(both)
        out[order] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
