#!/usr/bin/env python3
"""Times the radiance splat (csrc/drrt_sensor.hip k_sensor_radiance, k_sensor_radiance_bwd) for 1M rays onto a 512^2
image against the operator it extends, in the two regimes of tools/bench_sensor.py: spread-out rays and Luneburg-focused
rays.  Per regime, forward and forward + backward in one process:

  generate_sensor (per-ray e)  against  splat_radiance at C = 1      the price of the new path
  splat_radiance at C = 3      against  three calls at C = 1         the gain from sharing landing point and weights
  backward at C = 3 with       against  without dL/drad              what the extra output costs

The calls compared are alternated round by round; every figure is the median over the rounds with their range
(min, max): the spread of repeated runs.  One JSON line."""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench                                                   # noqa: E402
from adjointnonlinearraytracing_amd import drrt, sensor        # noqa: E402


def alternate(fns, rounds=9, reps=10):
    """{name: fn} -> {name: [median, min, max] ms per call}, the fns taking turns within every round."""
    for fn in fns.values():
        for _ in range(3):
            fn()
    ms = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(reps):
                fn()
            t1.record()
            torch.cuda.synchronize()
            ms[k].append(t0.elapsed_time(t1) / reps)
    return {k: [round(statistics.median(v), 4), round(min(v), 4), round(max(v), 4)] for k, v in ms.items()}


def main():
    dev = torch.device("cuda:0")
    drrt.options.check_failed = False
    n, res, span = 1 << 20, 512, 1.0
    torch.manual_seed(0)
    x = torch.rand(n, 3, device=dev) * 0.8 + 0.1
    x[:, 1] = span
    v = torch.randn(n, 3, device=dev) * 0.1
    v[:, 1] = 1.0
    nn = torch.tensor([[0.0, 1.0, 0.0]], device=dev)
    tt = torch.tensor([[0.0, 0.0, 1.0]], device=dev)
    rif, pos, vel, h, ds = bench.make_workload(256, 1024 * 1024, dev, seed=0)
    xt, vt = drrt.TracerC().trace(rif, (256, 256, 256), pos, vel, h, ds)
    regimes = {"spread": (x, v, torch.tensor([[0.5, 1.1, 0.5]], device=dev)),
               "focused": (xt, vt, torch.tensor([[0.5, 1.0, 0.5]], device=dev))}
    rad3 = torch.rand(n, 3, device=dev) + 0.5
    cols = [rad3[:, k].contiguous() for k in range(3)]
    gI3 = torch.randn(3, res, res, device=dev)
    out = {"rays": n, "res": res, "ms": "median, min, max over rounds"}
    for tag, (xs, vs, pp) in regimes.items():
        plane = (pp, nn)
        out[tag + "_fwd"] = alternate({
            "generate_sensor": lambda: sensor.generate_sensor((xs, vs), cols[0], plane, res, span, tt),
            "radiance_c1": lambda: sensor.splat_radiance((xs, vs), cols[0], plane, res, span, tt),
            "radiance_c3": lambda: sensor.splat_radiance((xs, vs), rad3, plane, res, span, tt),
            "radiance_c1_x3": lambda: [sensor.splat_radiance((xs, vs), c, plane, res, span, tt) for c in cols],
        })
        xg, vg = xs.clone().requires_grad_(True), vs.clone().requires_grad_(True)
        r1, r3 = cols[0].clone().requires_grad_(True), rad3.clone().requires_grad_(True)

        def step(fn, rad, gI):
            def run():
                xg.grad = None; vg.grad = None; r1.grad = None; r3.grad = None
                (fn((xg, vg), rad, plane, res, span, tt) * gI).sum().backward()
            return run

        out[tag + "_fwd_bwd"] = alternate({
            "generate_sensor": step(sensor.generate_sensor, cols[0], gI3[0]),
            "radiance_c1_rays": step(sensor.splat_radiance, cols[0], gI3[0]),
            "radiance_c1_rays_rad": step(sensor.splat_radiance, r1, gI3[0]),
            "radiance_c3_rays": step(sensor.splat_radiance, rad3, gI3),
            "radiance_c3_rays_rad": step(sensor.splat_radiance, r3, gI3),
        })
    print(json.dumps(out))


if __name__ == "__main__":
    main()
