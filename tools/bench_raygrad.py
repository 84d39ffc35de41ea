#!/usr/bin/env python3
"""Times the ray-state adjoint (drrt_backtrace_rays_f32, k_backtrace_rays) at the metric's configuration -- Luneburg ball
on a 256^3 grid, 1 048 576 rays of bench.py's plane source, ds = h / 2 (~512 iterations per ray) -- next to the calls it
goes with, each with device events around the library's own launches (drrt_profile_*) and as a whole call:

    forward            TracerC.trace                     (sort + pair copy + k_trace_flat)
    backtrace          TracerC.backtrace                 (dL/dn: classification + window kernel)
    backtrace_rays     TracerC.backtrace_rays            (dL/dpos, dL/dvel: k_backtrace_rays)
    backward_both      tracer.ADTracerC backward with rif, x and v requiring grad (both adjoints)
    backward_rif       tracer.BackTracerC backward       (the same without ray gradients)

usage: bench_raygrad.py [--grid 256] [--rays 1048576] [--iters 10] [--warmup 3]
Prints one JSON object: per phase the median whole-call time (ms, device events on the stream) and the median time of
each library launch inside it; the ray-state kernel's ray-steps/s (stats.ray_steps / its kernel time)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import bench  # noqa: E402
from adjointnonlinearraytracing_amd import _lib, drrt, tracer  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--rays", type=int, default=1024 * 1024)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    drrt.options.check_failed = False
    rif, pos, vel, h, ds = bench.make_workload(a.grid, a.rays, dev, seed=0)
    res = tuple(rif.shape)
    gen = torch.Generator(device="cpu").manual_seed(1)
    gx = torch.randn(pos.shape, generator=gen).to(dev)
    gv = torch.randn(pos.shape, generator=gen).to(dev)
    T = drrt.TracerC()
    lib = _lib.load()

    state = {}

    def forward():
        state["xt"], state["vt"] = T.trace(rif, res, pos, vel, h, ds)
        state["steps"] = drrt.keep_steps(drrt.last_steps)
        state["order"] = drrt.keep_order(drrt.last_order)

    def backtrace():
        T.backtrace(rif, res, state["xt"], state["vt"], gx, gv, h, ds, order=state["order"])

    def backtrace_rays():
        T.backtrace_rays(rif, res, pos, vel, state["xt"], state["vt"], state["steps"], gx, gv, h, ds, order=state["order"])
        state["ray_steps"] = drrt.read_stats()["ray_steps"] if "ray_steps" not in state else state["ray_steps"]

    def backward(cls, ray_grad):
        r = rif.detach().requires_grad_(True)
        x = pos.detach().requires_grad_(ray_grad)
        v = vel.detach().requires_grad_(ray_grad)
        xt, vt = cls.apply(r, x, v, h, ds)
        loss = (xt * gx).sum() + (vt * gv).sum()
        torch.cuda.synchronize(dev)
        return loss

    phases = {"forward": forward, "backtrace": backtrace, "backtrace_rays": backtrace_rays}
    out = {"grid": a.grid, "rays": a.rays, "h": h, "ds": ds, "iters": a.iters, "library": lib.drrt_version().decode()}
    forward()
    for name, fn in list(phases.items()) + [("backward_both", None), ("backward_rif", None)]:
        whole, kern = [], {}
        for it in range(a.warmup + a.iters):
            loss = None
            if fn is None:          # autograd backward: the forward is run (untimed) first
                loss = backward(tracer.ADTracerC if name == "backward_both" else tracer.BackTracerC, name == "backward_both")
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            lib.drrt_profile_begin(64)
            e0.record()
            if fn is None:
                loss.backward()
            else:
                fn()
            e1.record()
            torch.cuda.synchronize(dev)
            launches = _lib.profile_collect()
            lib.drrt_profile_end()
            if it < a.warmup:
                continue
            whole.append(e0.elapsed_time(e1))
            per = {}
            for k, ms in launches:
                per[k] = per.get(k, 0.0) + ms
            for k, ms in per.items():
                kern.setdefault(k, []).append(ms)
        out[name] = {"call_ms": statistics.median(whole),
                     "launch_ms": {k: statistics.median(v) for k, v in kern.items()}}
    k_ms = out["backtrace_rays"]["launch_ms"].get("backtrace_rays")
    out["backtrace_rays"]["ray_steps"] = state["ray_steps"]
    if k_ms:
        out["backtrace_rays"]["ray_steps_per_s_kernel"] = state["ray_steps"] / (k_ms * 1e-3)
    out["backward_both_over_backward_rif"] = out["backward_both"]["call_ms"] / out["backward_rif"]["call_ms"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
