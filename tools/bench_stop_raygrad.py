#!/usr/bin/env python3
"""Times the ray-state adjoints of the plane and SDF marches (drrt_backtrace_pln_rays_f32 / drrt_backtrace_sdf_rays_f32,
k_backtrace_stop_rays + k_backtrace_stop_rays_again) next to the calls whose work they do, in one process:

  plane  256^3 Luneburg, 1 048 576 rays of bench.py's plane source, sensor plane behind the volume: every ray's record is its
         last iteration, so the new call does one forward replay plus one backtrace_rays.
             trace_pln            TracerC.trace_pln            (k_trace_flat<.., 1> + k_trace_again)
             backtrace_rays       TracerC.backtrace_rays       (k_backtrace_rays, from trace_pln's exit rays and counts)
             backtrace_pln_rays   TracerC.backtrace_pln_rays   (the new call, in trace_pln's visit order)
  sdf    the trace_sdf case of tools/run_configs.py: the rays of that source moved to the mid-plane that start within 0.4
         of the centre (about 527k), ending on a sphere of radius 0.45 inside the lens.
             trace_sdf            TracerC.trace_sdf            (k_trace<2> + k_trace_again)
             backtrace_rays       TracerC.backtrace_rays       (from a plain trace of the same rays: trace_sdf leaves no
                                                                iteration counts; those rays run on to the box, so this
                                                                yardstick does somewhat MORE reverse iterations)
             backtrace_sdf_rays   TracerC.backtrace_sdf_rays   (the new call, in trace_sdf's visit order)

The three calls of a case are timed alternately (one of each per round) with device events around the whole call, so that
drift of the machine hits all three alike.

usage: bench_stop_raygrad.py [--grid 256] [--rays 1048576] [--rounds 7] [--warmup 2] [--once]
Prints one JSON object: per case and call the median, minimum and maximum ms over the rounds, the iteration counts
(stats.ray_steps), and the ratio of the new call to the sum of the two existing ones.  --once: a single call of each
(for a `rocprofv3 --kernel-trace --stats` run of its own)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import bench  # noqa: E402
from adjointnonlinearraytracing_amd import drrt  # noqa: E402


def plane_case(T, R, n, dev):
    rif, pos, vel, h, ds = bench.make_workload(R, n, dev, seed=0)
    res = tuple(rif.shape)
    ext = (R - 1) * h
    po = torch.tensor([[0.5 * ext, 1.5 * ext, 0.5 * ext]], device=dev).expand(pos.shape[0], 3).contiguous()
    pd = torch.tensor([[0.0, 1.0, 0.0]], device=dev).expand(pos.shape[0], 3).contiguous()
    xt, vt, _ = T.trace_pln(rif, res, pos, vel, po, pd, h, ds)
    steps, order = drrt.keep_steps(drrt.last_steps), drrt.keep_order(drrt.last_order)
    one = torch.ones_like(xt)
    return pos.shape[0], "backtrace_pln_rays", {
        "trace_pln": lambda: T.trace_pln(rif, res, pos, vel, po, pd, h, ds),
        "backtrace_rays": lambda: T.backtrace_rays(rif, res, pos, vel, xt, vt, steps, one, one, h, ds, order=order),
        "backtrace_pln_rays": lambda: T.backtrace_pln_rays(rif, res, pos, vel, po, pd, one, one, h, ds, order=order),
    }


def sdf_case(T, R, n, dev):
    rif, pos, vel, h, ds = bench.make_workload(R, n, dev, seed=1)
    res = tuple(rif.shape)
    g = torch.linspace(0, 1.0, R, device=dev)
    Z, Y, X = torch.meshgrid(g, g, g, indexing="ij")
    sdf = (torch.sqrt((X - .5) ** 2 + (Y - .5) ** 2 + (Z - .5) ** 2) - 0.45).contiguous()
    p2 = pos.clone()
    p2[:, 1] = 0.5
    keep = (p2 - 0.5).norm(dim=1) < 0.4
    p2, v2 = p2[keep].contiguous(), vel[keep].contiguous()
    xt, vt = T.trace(rif, res, p2, v2, h, ds)
    steps = drrt.keep_steps(drrt.last_steps)
    T.trace_sdf(rif, sdf, res, p2, v2, h, ds)
    order = drrt.keep_order(drrt.last_order)
    one = torch.ones_like(xt)
    return p2.shape[0], "backtrace_sdf_rays", {
        "trace_sdf": lambda: T.trace_sdf(rif, sdf, res, p2, v2, h, ds),
        "backtrace_rays": lambda: T.backtrace_rays(rif, res, p2, v2, xt, vt, steps, one, one, h, ds, order=order),
        "backtrace_sdf_rays": lambda: T.backtrace_sdf_rays(rif, sdf, res, p2, v2, one, one, h, ds, order=order),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--rays", type=int, default=1 << 20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--once", action="store_true")
    a = ap.parse_args()
    if a.grid < 4 or a.rays < 1 or a.rounds < 1 or a.warmup < 0:
        ap.error("--grid >= 4, --rays and --rounds positive, --warmup non-negative")
    if not torch.cuda.is_available():
        sys.exit("bench_stop_raygrad: needs a GPU")
    dev = torch.device("cuda:0")
    drrt.options.check_failed = False
    T = drrt.TracerC()
    out = dict(grid=a.grid, rounds=a.rounds)
    for case, build in (("plane", plane_case), ("sdf", sdf_case)):
        n, new, calls = build(T, a.grid, a.rays, dev)
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
        old = [k for k in calls if k != new]
        both = [x + y for x, y in zip(ms[old[0]], ms[old[1]])]
        res["rays"] = n
        res["sum_existing_median_ms"] = statistics.median(both)
        res["new_over_sum_existing"] = statistics.median(ms[new]) / statistics.median(both)
        out[case] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
