#!/usr/bin/env python3
"""Times the ray-state adjoints (dL/dpos, dL/dvel) next to the calls they go with, one workload per sub-command.  Each
prints one JSON object.

cube    drrt_backtrace_rays_f32 (k_backtrace_rays) at the metric's configuration -- Luneburg ball on a 256^3 grid,
        1 048 576 rays of bench.py's plane source, ds = h / 2 (~512 iterations per ray) -- each phase with device events
        around the library's own launches (drrt_profile_*) and as a whole call:
            forward            TracerC.trace                     (sort + pair copy + k_trace_flat)
            backtrace          TracerC.backtrace                 (dL/dn: classification + window kernel)
            backtrace_rays     TracerC.backtrace_rays            (dL/dpos, dL/dvel: k_backtrace_rays)
            backward_both      tracer.ADTracerC backward with rif, x and v requiring grad (both adjoints)
            backward_rif       tracer.BackTracerC backward       (the same without ray gradients)
        usage: bench_raygrad.py cube [--grid 256] [--rays 1048576] [--iters 10] [--warmup 3]
        Output: per phase the median whole-call time (ms, device events on the stream) and the median time of each
        library launch inside it; the ray-state kernel's ray-steps/s (stats.ray_steps / its kernel time).

cable   drrt_backtrace_cable_rays_f32 (k_backtrace_cable_rays) on the workload of tools/bench_cable.py -- 257-sample
        Luneburg-like profile, 4 194 304 rays x ~512 steps, closest approach to a target at 0.75 length -- for rays in
        random order and in source-pixel order:
            trace_cable            TracerC.trace_cable            (k_trace_cable)
            backtrace_cable        TracerC.backtrace_cable        (k_backtrace_cable: dL/dn)
            backtrace_cable_rays   TracerC.backtrace_cable_rays   (k_backtrace_cable_rays: dL/dpos, dL/dvel; replay + reverse)
        usage: bench_raygrad.py cable [--side 2048] [--rounds 7] [--warmup 2] [--once]

stop    drrt_backtrace_pln_rays_f32 / drrt_backtrace_sdf_rays_f32 (k_backtrace_stop_rays + k_backtrace_stop_rays_again)
        next to the calls whose work they do:
          plane  256^3 Luneburg, 1 048 576 rays of bench.py's plane source, sensor plane behind the volume: every ray's
                 record is its last iteration, so the new call does one forward replay plus one backtrace_rays.
                     trace_pln            TracerC.trace_pln            (k_trace_flat<.., 1> + k_trace_again)
                     backtrace_rays       TracerC.backtrace_rays       (k_backtrace_rays, from trace_pln's exit rays and counts)
                     backtrace_pln_rays   TracerC.backtrace_pln_rays   (the new call, in trace_pln's visit order)
          sdf    the trace_sdf case of tools/run_configs.py: the rays of that source moved to the mid-plane that start
                 within 0.4 of the centre (about 527k), ending on a sphere of radius 0.45 inside the lens.
                     trace_sdf            TracerC.trace_sdf            (k_trace<2> + k_trace_again)
                     backtrace_rays       TracerC.backtrace_rays       (from a plain trace of the same rays: trace_sdf leaves
                                                                        no iteration counts; those rays run on to the box, so
                                                                        this yardstick does somewhat MORE reverse iterations)
                     backtrace_sdf_rays   TracerC.backtrace_sdf_rays   (the new call, in trace_sdf's visit order)
        usage: bench_raygrad.py stop [--grid 256] [--rays 1048576] [--rounds 7] [--warmup 2] [--once]

target  drrt_backtrace_target_rays_f32 (k_target_rays_count + k_backtrace_target_rays) next to the calls it goes with: 256^3
        Luneburg ball, 1 048 576 rays of bench.py's plane source, every ray's target the ball's focal point on the far y face.
            trace_target            TracerC.trace_target            (k_target_a_flat + k_target_b)
            backtrace               TracerC.backtrace               (dL/dn from the record, in trace_target's visit order)
            backtrace_target_rays   TracerC.backtrace_target_rays   (the new call, in trace_target's visit order, dist2 seeded)
        usage: bench_raygrad.py target [--grid 256] [--rays 1048576] [--rounds 7] [--warmup 2] [--once] [--out FILE]
        Also writes the JSON, with the library's version string (source digest), to --out (default
        profiles/target_raygrad_bench.json).

opl     drrt_trace_opl_f32 / drrt_backtrace_opl_f32 (k_trace_opl, k_backtrace_opl) next to the calls they go with: 256^3 grid,
        1 048 576 rays of bench.py's plane source, ds = h / 2, through two media: `luneburg` (the ball: every ray passes the
        few voxels around the focus, the worst case for the plain atomics k_backtrace_opl scatters with) and `tomo_weak`
        (bench.make_grid_tomo, n = 1 + 3e-4 U: straight rays, the representative case of a phase measurement).
            trace               TracerC.trace                      (k_trace_flat)
            trace_opl           TracerC.trace_opl                  (k_trace_opl)
            backtrace           TracerC.backtrace                  (dL/dn: classification + window kernel)
            backtrace_rays      TracerC.backtrace_rays             (dL/dpos, dL/dvel)
            backtrace_opl_all   TracerC.backtrace_opl              (dL/dn, dL/dpos, dL/dvel from seeds on xt, vt, opl)
            backtrace_opl_grid  TracerC.backtrace_opl(rays=False)  (dL/dn alone)
        The six calls are timed alternately like the cases below.  Output per medium and call: median, minimum, maximum ms
        and stats.ray_steps, and the ratios trace_opl / trace, backtrace_opl_all / (backtrace + backtrace_rays),
        backtrace_opl_grid / backtrace.
        usage: bench_raygrad.py opl [--grid 256] [--rays 1048576] [--rounds 7] [--warmup 2] [--once] [--out FILE]
        Also writes the JSON, with the library's version string (source digest), to --out (default profiles/opl_bench.json).

field   drrt_trace_field_f32 / drrt_backtrace_field_f32 (k_trace_field, k_backtrace_field) next to the optical-path-length calls
        they are modelled on, on the workloads of `opl` (256^3, 1 048 576 rays, `luneburg` and `tomo_weak`); the second field is
        1 + 0.5 U, seeded.  All adjoints take seeds on all three outputs and return the ray gradients too.
            trace                  TracerC.trace
            trace_opl              TracerC.trace_opl
            trace_field            TracerC.trace_field
            backtrace_opl          TracerC.backtrace_opl                          (dL/dn)
            backtrace_field_rif    TracerC.backtrace_field(field_grid=False)      (dL/dn)
            backtrace_field_field  TracerC.backtrace_field(grid=False)            (dL/dfield)
            backtrace_field_both   TracerC.backtrace_field                        (dL/dn and dL/dfield)
        Timed alternately like `opl`.  Output per medium and call: median, minimum, maximum ms and stats.ray_steps, and the
        ratios trace_field / trace_opl, trace_field / trace and backtrace_field_* / backtrace_opl.
        usage: bench_raygrad.py field [--grid 256] [--rays 1048576] [--rounds 7] [--warmup 2] [--once] [--out FILE]
        Also writes the JSON, with the library's version string (source digest), to --out (default profiles/field_bench.json).

emission  drrt_trace_emission_f32 / drrt_backtrace_emission_f32 (k_trace_emission, k_backtrace_emission) next to the field
        calls they are modelled on, on the workloads of `field`; emission e = 1 + 0.5 U, absorption a = s (1 + 0.5 U) with s
        such that the median tau of the rays is 1 (found with one trace_field per medium), both seeded.  All adjoints take
        seeds on all outputs and return the ray gradients too.
            trace_field               TracerC.trace_field(field = a)
            trace_emission            TracerC.trace_emission
            backtrace_field           TracerC.backtrace_field(grid=False)                            (dL/da)
            backtrace_emission_rif    TracerC.backtrace_emission(emission_grid = absorption_grid = False)   (dL/dn)
            backtrace_emission_e      TracerC.backtrace_emission(grid = absorption_grid = False)     (dL/de)
            backtrace_emission_a      TracerC.backtrace_emission(grid = emission_grid = False)       (dL/da)
            backtrace_emission_all    TracerC.backtrace_emission                                     (all three grids)
        Timed alternately like `field`.  Output per medium and call: median, minimum, maximum ms and stats.ray_steps, the
        median tau, and the ratios trace_emission / trace_field and backtrace_emission_* / backtrace_field.
        usage: bench_raygrad.py emission [--grid 256] [--rays 1048576] [--rounds 7] [--warmup 2] [--once] [--out FILE]
        Also writes the JSON, with the library's version string (source digest), to --out (default profiles/emission_bench.json).

vector  drrt_trace_vector_f32 / drrt_backtrace_vector_f32 (k_trace_vector, k_backtrace_vector) next to the field and emission
        calls, on the workloads of `field`; the vector field is three planes U - 0.5 (seeded), the second fields those of
        `emission`.  All adjoints take the forward's visit order, unit seeds on every output:
            trace_field, trace_emission, backtrace_field (dL/da), backtrace_emission (all three grids)   as in `emission`
            trace_vector             TracerC.trace_vector
            backtrace_vector_rif     TracerC.backtrace_vector(vfield_grid=False)              (dL/dn)
            backtrace_vector_u       TracerC.backtrace_vector(grid=False)                     (the three planes of dL/du)
            backtrace_vector_both    TracerC.backtrace_vector                                 (all four planes)
            backtrace_vector_rays    TracerC.backtrace_vector(grid=False, vfield_grid=False)  (dpos, dvel alone)
        Timed alternately like `field`.  Output per medium and call: median, minimum, maximum ms and stats.ray_steps, and the
        ratios trace_vector / trace_emission, trace_vector / trace_field and backtrace_vector_* / backtrace_field.
        usage: bench_raygrad.py vector [--grid 256] [--rays 1048576] [--rounds 7] [--warmup 2] [--once] [--out FILE]
        Also writes the JSON, with the library's version string (source digest), to --out (default profiles/vector_bench.json).
path    drrt_trace_path_f32 / drrt_backtrace_path_f32 (k_trace_path, k_backtrace_path) next to the opl calls, which run the same
        march without the series, on the Luneburg workload of `opl`: per stride (--strides, default 1 8 64) with
        samples = ceil(max_steps / stride) + 1, in pixel order (sort_rays off) and in sorted order (the forward sorts, the
        adjoints take its order); all eight calls of a combination alternate in one process:
            trace_opl / trace_path                            the forward; trace_path_extra_ms is their difference, next to
                                                              path_bytes = samples n 12 and what writing them at 8 TB/s takes
            backtrace_{opl,path}_{rays,grid,both}             the adjoints, every seed set (dpath: ones)
        usage: bench_raygrad.py path [--grid 256] [--rays 1048576] [--strides 1 8 64] [--rounds 7] [--warmup 2] [--once] [--out FILE]
        Also writes the JSON, with the library's version string, to --out (default profiles/path_bench.json).
phase   drrt_trace_phase_f32 / drrt_backtrace_phase_f32 (k_trace_phase, k_backtrace_phase) next to the path calls, on the
        workload, strides and orders of `path`; all nine calls of a combination alternate in one process:
            trace_opl / trace_path / trace_phase              the forward; trace_path_extra_ms = trace_path - trace_opl and
                                                              trace_phase_extra_ms = trace_phase - trace_path are each the
                                                              cost of writing one series of samples n 12 bytes
            backtrace_{path,phase}_{rays,grid,both}           the adjoints, every seed set (dpath, dvpath: ones)
        usage: bench_raygrad.py phase [--grid 256] [--rays 1048576] [--strides 1 8 64] [--rounds 7] [--warmup 2] [--once] [--out FILE]
        Also writes the JSON, with the library's version string, to --out (default profiles/phase_bench.json).

cable, stop and target time the three calls of a case alternately (one of each per round) with device events around the whole
call, so that drift of the machine hits all three alike.  Output: per case and call the median, minimum and maximum ms
over the rounds, the iteration counts (stats.ray_steps), and the ratio of the new call to the sum of the two existing
ones.  --once: a single call of each (for a `rocprofv3 --kernel-trace --stats` run of its own)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import bench  # noqa: E402
from adjointnonlinearraytracing_amd import _lib, drrt, tracer  # noqa: E402


def time_alternately(calls, new, a):
    """`calls` = {name: fn}, two existing calls and the `new` one -> the JSON of one case; None with --once, which makes
    a single call of each instead."""
    if a.once:
        for fn in calls.values():
            fn()
        torch.cuda.synchronize()
        return None
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
    res["sum_existing_median_ms"] = statistics.median(both)
    res["new_over_sum_existing"] = statistics.median(ms[new]) / statistics.median(both)
    return res


# ---- cube -----------------------------------------------------------------------------------------------------------
def cube(a, dev):
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
    return out


# ---- cable ----------------------------------------------------------------------------------------------------------
def cable_rays(order, side, radius, ds, dev):
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


def cable(a, dev):
    rres, radius = 257, 1.0
    ds = radius / (rres - 1) / 2
    length = 512 * ds
    prof = torch.sqrt(2.0 - torch.linspace(0, 1, rres) ** 2).to(dev)
    n = a.side * a.side
    tg = torch.tensor([[radius, 0.75 * length, radius]], device=dev).expand(n, 3).contiguous()
    T = drrt.TracerC()
    out = dict(rays=n, rres=rres, ds=ds, length=length, rounds=a.rounds)
    for order in ("random", "pixel"):
        pos, vel = cable_rays(order, a.side, radius, ds, dev)
        xt, vt, _ = T.trace_cable(prof, radius, length, pos, vel, tg, ds)
        one = torch.ones_like(xt)
        res = time_alternately({
            "trace_cable": lambda: T.trace_cable(prof, radius, length, pos, vel, tg, ds),
            "backtrace_cable": lambda: T.backtrace_cable(prof, radius, length, xt, vt, one, one, ds),
            "backtrace_cable_rays": lambda: T.backtrace_cable_rays(prof, radius, length, pos, vel, tg, one, one, ds),
        }, "backtrace_cable_rays", a)
        if res is not None:
            out[order] = res
    return out


# ---- stop -----------------------------------------------------------------------------------------------------------
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


def stop(a, dev):
    T = drrt.TracerC()
    out = dict(grid=a.grid, rounds=a.rounds)
    for case, build in (("plane", plane_case), ("sdf", sdf_case)):
        n, new, calls = build(T, a.grid, a.rays, dev)
        res = time_alternately(calls, new, a)
        if res is not None:
            out[case] = dict(res, rays=n)
    return out


# ---- target ---------------------------------------------------------------------------------------------------------
def target(a, dev):
    rif, pos, vel, h, ds = bench.make_workload(a.grid, a.rays, dev, seed=0)
    res = tuple(rif.shape)
    ext = (a.grid - 1) * h
    n = pos.shape[0]
    tg = torch.tensor([[0.5 * ext, ext, 0.5 * ext]], device=dev).expand(n, 3).contiguous()
    T = drrt.TracerC()
    xt, vt, _ = T.trace_target(rif, res, pos, vel, tg, h, ds)
    order = drrt.keep_order(drrt.last_order)
    one, g = torch.ones_like(xt), torch.ones(n, device=dev)
    res_ = time_alternately({
        "trace_target": lambda: T.trace_target(rif, res, pos, vel, tg, h, ds),
        "backtrace": lambda: T.backtrace(rif, res, xt, vt, one, one, h, ds, order=order),
        "backtrace_target_rays": lambda: T.backtrace_target_rays(rif, res, pos, vel, tg, one, one, h, ds, ddist2=g, order=order),
    }, "backtrace_target_rays", a)
    if res_ is None:
        return {}
    out = dict(res_, grid=a.grid, rays=n, h=h, ds=ds, rounds=a.rounds, library=_lib.load().drrt_version().decode())
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return out


# ---- opl, field -----------------------------------------------------------------------------------------------------
def time_each(calls, a):
    """`calls` = {name: fn}, timed alternately (one of each per round, device events around the whole call) -> (per call:
    median, minimum, maximum ms and stats.ray_steps; the medians); (None, None) with --once, which makes a single call of
    each instead."""
    if a.once:
        for fn in calls.values():
            fn()
        torch.cuda.synchronize()
        return None, None
    rsteps, ms = {}, {k: [] for k in calls}
    for k, fn in calls.items():
        for _ in range(max(a.warmup, 1)):
            fn()
        rsteps[k] = drrt.read_stats()["ray_steps"]
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for k, fn in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    med = {k: statistics.median(v) for k, v in ms.items()}
    return {k: dict(median_ms=med[k], min_ms=min(v), max_ms=max(v), ray_steps=rsteps[k]) for k, v in ms.items()}, med


def opl(a, dev):
    pos, vel = (t.to(dev) for t in bench.make_rays(a.rays, seed=0))      # make_workload's rays; the grids are made below
    h = 1.0 / (a.grid - 1)
    ds = h / 2
    n = pos.shape[0]
    T = drrt.TracerC()
    one, g = torch.ones_like(pos), torch.ones(n, device=dev)
    out = dict(grid=a.grid, rays=n, h=h, ds=ds, rounds=a.rounds, library=_lib.load().drrt_version().decode())
    for medium, make in (("luneburg", bench.make_grid), ("tomo_weak", bench.make_grid_tomo)):
        rif = make(a.grid, dev)
        res = tuple(rif.shape)
        xt, vt, _, steps = T.trace_opl(rif, res, pos, vel, h, ds)
        order = drrt.keep_order(drrt.last_order)
        calls = {
            "trace": lambda: T.trace(rif, res, pos, vel, h, ds),
            "trace_opl": lambda: T.trace_opl(rif, res, pos, vel, h, ds),
            "backtrace": lambda: T.backtrace(rif, res, xt, vt, one, one, h, ds, order=order),
            "backtrace_rays": lambda: T.backtrace_rays(rif, res, pos, vel, xt, vt, steps, one, one, h, ds, order=order),
            "backtrace_opl_all": lambda: T.backtrace_opl(rif, res, pos, vel, xt, vt, steps, one, one, g, h, ds, order=order),
            "backtrace_opl_grid": lambda: T.backtrace_opl(rif, res, pos, vel, xt, vt, steps, one, one, g, h, ds, rays=False,
                                                          order=order),
        }
        r, med = time_each(calls, a)
        if r is None:
            continue
        r["trace_opl_over_trace"] = med["trace_opl"] / med["trace"]
        r["backtrace_opl_all_over_backtrace_plus_backtrace_rays"] = med["backtrace_opl_all"] / (med["backtrace"] + med["backtrace_rays"])
        r["backtrace_opl_grid_over_backtrace"] = med["backtrace_opl_grid"] / med["backtrace"]
        out[medium] = r
    if a.once:
        return {}
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return out


def field(a, dev):
    pos, vel = (t.to(dev) for t in bench.make_rays(a.rays, seed=0))      # the rays of `opl`
    h = 1.0 / (a.grid - 1)
    ds = h / 2
    n = pos.shape[0]
    T = drrt.TracerC()
    one, g = torch.ones_like(pos), torch.ones(n, device=dev)
    fld = (1.0 + 0.5 * torch.rand((a.grid,) * 3, generator=torch.Generator(device="cpu").manual_seed(2))).to(dev)
    out = dict(grid=a.grid, rays=n, h=h, ds=ds, rounds=a.rounds, library=_lib.load().drrt_version().decode())
    for medium, make in (("luneburg", bench.make_grid), ("tomo_weak", bench.make_grid_tomo)):
        rif = make(a.grid, dev)
        res = tuple(rif.shape)
        xt, vt, _, steps = T.trace_field(rif, fld, res, pos, vel, h, ds)
        order = drrt.keep_order(drrt.last_order)
        back = lambda **kw: T.backtrace_field(rif, fld, res, pos, vel, xt, vt, steps, one, one, g, h, ds, order=order, **kw)   # noqa: E731
        r, med = time_each({
            "trace": lambda: T.trace(rif, res, pos, vel, h, ds),
            "trace_opl": lambda: T.trace_opl(rif, res, pos, vel, h, ds),
            "trace_field": lambda: T.trace_field(rif, fld, res, pos, vel, h, ds),
            "backtrace_opl": lambda: T.backtrace_opl(rif, res, pos, vel, xt, vt, steps, one, one, g, h, ds, order=order),
            "backtrace_field_rif": lambda: back(field_grid=False),
            "backtrace_field_field": lambda: back(grid=False),
            "backtrace_field_both": back,
        }, a)
        if r is None:
            continue
        r["trace_field_over_trace_opl"] = med["trace_field"] / med["trace_opl"]
        r["trace_field_over_trace"] = med["trace_field"] / med["trace"]
        for k in ("rif", "field", "both"):
            r[f"backtrace_field_{k}_over_backtrace_opl"] = med[f"backtrace_field_{k}"] / med["backtrace_opl"]
        out[medium] = r
    if a.once:
        return {}
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return out


def emission(a, dev):
    pos, vel = (t.to(dev) for t in bench.make_rays(a.rays, seed=0))      # the rays of `opl` and `field`
    h = 1.0 / (a.grid - 1)
    ds = h / 2
    n = pos.shape[0]
    T = drrt.TracerC()
    one, g = torch.ones_like(pos), torch.ones(n, device=dev)
    gen = lambda seed: (1.0 + 0.5 * torch.rand((a.grid,) * 3, generator=torch.Generator(device="cpu").manual_seed(seed))).to(dev)   # noqa: E731
    emis, unit = gen(2), gen(3)
    out = dict(grid=a.grid, rays=n, h=h, ds=ds, rounds=a.rounds, library=_lib.load().drrt_version().decode())
    for medium, make in (("luneburg", bench.make_grid), ("tomo_weak", bench.make_grid_tomo)):
        rif = make(a.grid, dev)
        res = tuple(rif.shape)
        absb = unit / float(T.trace_field(rif, unit, res, pos, vel, h, ds)[2].median())      # median tau = 1
        xt, vt, _, tau, steps = T.trace_emission(rif, emis, absb, res, pos, vel, h, ds)
        order = drrt.keep_order(drrt.last_order)
        back = lambda **kw: T.backtrace_emission(rif, emis, absb, res, pos, vel, xt, vt, steps, tau, one, one, g, g, h, ds,   # noqa: E731
                                                 order=order, **kw)
        r, med = time_each({
            "trace_field": lambda: T.trace_field(rif, absb, res, pos, vel, h, ds),
            "trace_emission": lambda: T.trace_emission(rif, emis, absb, res, pos, vel, h, ds),
            "backtrace_field": lambda: T.backtrace_field(rif, absb, res, pos, vel, xt, vt, steps, one, one, g, h, ds, grid=False,
                                                         order=order),
            "backtrace_emission_rif": lambda: back(emission_grid=False, absorption_grid=False),
            "backtrace_emission_e": lambda: back(grid=False, absorption_grid=False),
            "backtrace_emission_a": lambda: back(grid=False, emission_grid=False),
            "backtrace_emission_all": back,
        }, a)
        if r is None:
            continue
        r["median_tau"] = float(tau.median())
        r["trace_emission_over_trace_field"] = med["trace_emission"] / med["trace_field"]
        for k in ("rif", "e", "a", "all"):
            r[f"backtrace_emission_{k}_over_backtrace_field"] = med[f"backtrace_emission_{k}"] / med["backtrace_field"]
        out[medium] = r
    if a.once:
        return {}
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return out


def vector(a, dev):
    pos, vel = (t.to(dev) for t in bench.make_rays(a.rays, seed=0))      # the rays of `opl`, `field` and `emission`
    h = 1.0 / (a.grid - 1)
    ds = h / 2
    n = pos.shape[0]
    T = drrt.TracerC()
    one, g = torch.ones_like(pos), torch.ones(n, device=dev)
    gen = lambda seed, *lead: torch.rand(lead + (a.grid,) * 3, generator=torch.Generator(device="cpu").manual_seed(seed))   # noqa: E731
    emis, unit = (1.0 + 0.5 * gen(2)).to(dev), (1.0 + 0.5 * gen(3)).to(dev)
    vf = (gen(4, 3) - 0.5).to(dev)
    out = dict(grid=a.grid, rays=n, h=h, ds=ds, rounds=a.rounds, library=_lib.load().drrt_version().decode())
    for medium, make in (("luneburg", bench.make_grid), ("tomo_weak", bench.make_grid_tomo)):
        rif = make(a.grid, dev)
        res = tuple(rif.shape)
        absb = unit / float(T.trace_field(rif, unit, res, pos, vel, h, ds)[2].median())      # median tau = 1
        tau = T.trace_emission(rif, emis, absb, res, pos, vel, h, ds)[3]
        xt, vt, _, steps = T.trace_vector(rif, vf, res, pos, vel, h, ds)
        order = drrt.keep_order(drrt.last_order)
        back = lambda **kw: T.backtrace_vector(rif, vf, res, pos, vel, xt, vt, steps, one, one, g, h, ds, order=order, **kw)   # noqa: E731
        r, med = time_each({
            "trace_field": lambda: T.trace_field(rif, absb, res, pos, vel, h, ds),
            "trace_emission": lambda: T.trace_emission(rif, emis, absb, res, pos, vel, h, ds),
            "trace_vector": lambda: T.trace_vector(rif, vf, res, pos, vel, h, ds),
            "backtrace_field": lambda: T.backtrace_field(rif, absb, res, pos, vel, xt, vt, steps, one, one, g, h, ds, grid=False,
                                                         order=order),
            "backtrace_emission": lambda: T.backtrace_emission(rif, emis, absb, res, pos, vel, xt, vt, steps, tau, one, one, g, g,
                                                               h, ds, order=order),
            "backtrace_vector_rif": lambda: back(vfield_grid=False),
            "backtrace_vector_u": lambda: back(grid=False),
            "backtrace_vector_both": back,
            "backtrace_vector_rays": lambda: back(grid=False, vfield_grid=False),
        }, a)
        if r is None:
            continue
        r["trace_vector_over_trace_emission"] = med["trace_vector"] / med["trace_emission"]
        r["trace_vector_over_trace_field"] = med["trace_vector"] / med["trace_field"]
        for k in ("rif", "u", "both", "rays"):
            r[f"backtrace_vector_{k}_over_backtrace_field"] = med[f"backtrace_vector_{k}"] / med["backtrace_field"]
        r["backtrace_emission_over_backtrace_field"] = med["backtrace_emission"] / med["backtrace_field"]
        out[medium] = r
    if a.once:
        return {}
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return out


def _series(a, dev, velocities, calls, derive):
    """What `path` and `phase` share: the rays of `opl`, and per visit order and stride one trace_path whose outputs feed
    the adjoints, with a seed of ones per series (two with `velocities`).  `calls(T, fwd, back, seeds, stride, m)` -> the
    timed calls of one setting: `fwd` = (rif, res, pos, vel, h, ds), the arguments of every forward, and
    `back(method, *tail, **kw)` calls an adjoint on the setting's forward outputs with seeds of ones on (xt, vt), `tail` being
    what follows them.  `derive(r, med, nbytes)` adds the mode's own figures, `nbytes` the size of one series."""
    pos, vel = (t.to(dev) for t in bench.make_rays(a.rays, seed=0))
    h = 1.0 / (a.grid - 1)
    ds = h / 2
    n = pos.shape[0]
    T = drrt.TracerC()
    one = torch.ones_like(pos)
    rif = bench.make_grid(a.grid, dev)
    res = tuple(rif.shape)
    ms = drrt.path_max_steps(res, h, ds)
    out = dict(grid=a.grid, rays=n, h=h, ds=ds, max_steps=ms, rounds=a.rounds, library=_lib.load().drrt_version().decode())
    for order_name, sort in (("pixel", False), ("sorted", True)):
        for stride in a.strides:
            m = -(-ms // stride) + 1
            with drrt.using(sort_rays=sort):
                xt, vt, pth, count, steps = T.trace_path(rif, res, pos, vel, h, ds, stride, m)
                order = drrt.keep_order(drrt.last_order)
                seeds = [torch.ones_like(pth) for _ in range(2 if velocities else 1)]
                del pth
                back = lambda method, *tail, **kw: method(rif, res, pos, vel, xt, vt, steps, one, one, *tail,   # noqa: E731
                                                          order=order, **kw)
                r, med = time_each(calls(T, (rif, res, pos, vel, h, ds), back, seeds, stride, m), a)
            del seeds
            if r is None:
                continue
            r["samples"], r["mean_count"] = m, float(count.float().mean())
            derive(r, med, m * n * 12)
            out[f"{order_name}_stride{stride}"] = r
    if a.once:
        return {}
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return out


def path(a, dev):
    def calls(T, fwd, back, seeds, stride, m):
        h, ds = fwd[4:]
        g = torch.ones(fwd[2].shape[0], device=dev)
        bo = lambda **kw: back(T.backtrace_opl, g, h, ds, **kw)      # noqa: E731
        bp = lambda **kw: back(T.backtrace_path, seeds[0], h, ds, stride, **kw)      # noqa: E731
        return {
            "trace_opl": lambda: T.trace_opl(*fwd),
            "trace_path": lambda: T.trace_path(*fwd, stride, m),
            "backtrace_opl_rays": lambda: bo(grid=False), "backtrace_path_rays": lambda: bp(grid=False),
            "backtrace_opl_grid": lambda: bo(rays=False), "backtrace_path_grid": lambda: bp(rays=False),
            "backtrace_opl_both": bo, "backtrace_path_both": bp,
        }

    def derive(r, med, nbytes):
        r["path_bytes"] = nbytes
        r["trace_path_extra_ms"] = med["trace_path"] - med["trace_opl"]
        # what the extra time would be if the path were written at the peak HBM rate of the part (8 TB/s)
        r["path_bytes_at_8TBps_ms"] = nbytes / 8e12 * 1e3
        r["trace_path_over_trace_opl"] = med["trace_path"] / med["trace_opl"]
        for k in ("rays", "grid", "both"):
            r[f"backtrace_path_{k}_over_backtrace_opl_{k}"] = med[f"backtrace_path_{k}"] / med[f"backtrace_opl_{k}"]

    return _series(a, dev, False, calls, derive)


def phase(a, dev):
    def calls(T, fwd, back, seeds, stride, m):
        h, ds = fwd[4:]
        bp = lambda **kw: back(T.backtrace_path, seeds[0], h, ds, stride, **kw)      # noqa: E731
        bq = lambda **kw: back(T.backtrace_phase, *seeds, h, ds, stride, **kw)      # noqa: E731
        return {
            "trace_opl": lambda: T.trace_opl(*fwd),
            "trace_path": lambda: T.trace_path(*fwd, stride, m),
            "trace_phase": lambda: T.trace_phase(*fwd, stride, m),
            "backtrace_path_rays": lambda: bp(grid=False), "backtrace_phase_rays": lambda: bq(grid=False),
            "backtrace_path_grid": lambda: bp(rays=False), "backtrace_phase_grid": lambda: bq(rays=False),
            "backtrace_path_both": bp, "backtrace_phase_both": bq,
        }

    def derive(r, med, nbytes):
        r["series_bytes"] = nbytes
        # both differences are the cost of writing one series of samples n 12 bytes
        r["trace_path_extra_ms"] = med["trace_path"] - med["trace_opl"]
        r["trace_phase_extra_ms"] = med["trace_phase"] - med["trace_path"]
        r["series_bytes_at_8TBps_ms"] = nbytes / 8e12 * 1e3
        r["trace_phase_over_trace_path"] = med["trace_phase"] / med["trace_path"]
        for k in ("rays", "grid", "both"):
            r[f"backtrace_phase_{k}_over_backtrace_path_{k}"] = med[f"backtrace_phase_{k}"] / med[f"backtrace_path_{k}"]

    return _series(a, dev, True, calls, derive)


def main():
    ap = argparse.ArgumentParser(description="ray-state adjoint timings; see the module docstring")
    sub = ap.add_subparsers(dest="workload", required=True)
    p_cube = sub.add_parser("cube")
    p_cube.add_argument("--grid", type=int, default=256)
    p_cube.add_argument("--rays", type=int, default=1024 * 1024)
    p_cube.add_argument("--iters", type=int, default=10)
    p_cube.add_argument("--warmup", type=int, default=3)
    p_cube.set_defaults(run=cube)
    p_cable = sub.add_parser("cable")
    p_cable.add_argument("--side", type=int, default=2048, help="rays = side^2")
    p_cable.set_defaults(run=cable)
    p_stop = sub.add_parser("stop")
    p_stop.add_argument("--grid", type=int, default=256)
    p_stop.add_argument("--rays", type=int, default=1 << 20)
    p_stop.set_defaults(run=stop)
    p_target = sub.add_parser("target")
    p_target.add_argument("--grid", type=int, default=256)
    p_target.add_argument("--rays", type=int, default=1 << 20)
    p_target.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles",
                                                        "target_raygrad_bench.json"))
    p_target.set_defaults(run=target)
    p_opl = sub.add_parser("opl")
    p_opl.add_argument("--grid", type=int, default=256)
    p_opl.add_argument("--rays", type=int, default=1 << 20)
    p_opl.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "opl_bench.json"))
    p_opl.set_defaults(run=opl)
    p_field = sub.add_parser("field")
    p_field.add_argument("--grid", type=int, default=256)
    p_field.add_argument("--rays", type=int, default=1 << 20)
    p_field.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "field_bench.json"))
    p_field.set_defaults(run=field)
    p_emis = sub.add_parser("emission")
    p_emis.add_argument("--grid", type=int, default=256)
    p_emis.add_argument("--rays", type=int, default=1 << 20)
    p_emis.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "emission_bench.json"))
    p_emis.set_defaults(run=emission)
    p_vec = sub.add_parser("vector")
    p_vec.add_argument("--grid", type=int, default=256)
    p_vec.add_argument("--rays", type=int, default=1 << 20)
    p_vec.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "vector_bench.json"))
    p_vec.set_defaults(run=vector)
    p_path = sub.add_parser("path")
    p_path.add_argument("--grid", type=int, default=256)
    p_path.add_argument("--rays", type=int, default=1 << 20)
    p_path.add_argument("--strides", type=int, nargs="+", default=[1, 8, 64])
    p_path.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "path_bench.json"))
    p_path.set_defaults(run=path)
    p_phase = sub.add_parser("phase")
    p_phase.add_argument("--grid", type=int, default=256)
    p_phase.add_argument("--rays", type=int, default=1 << 20)
    p_phase.add_argument("--strides", type=int, nargs="+", default=[1, 8, 64])
    p_phase.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "phase_bench.json"))
    p_phase.set_defaults(run=phase)
    for p in (p_cable, p_stop, p_target, p_opl, p_field, p_emis, p_vec, p_path, p_phase):
        p.add_argument("--rounds", type=int, default=7)
        p.add_argument("--warmup", type=int, default=2)
        p.add_argument("--once", action="store_true")
    a = ap.parse_args()
    if a.workload == "cable" and (a.side < 1 or a.rounds < 1 or a.warmup < 0):
        ap.error("--side and --rounds must be positive, --warmup non-negative")
    if a.workload in ("stop", "target", "opl", "field", "emission", "vector", "path", "phase") and (a.grid < 4 or a.rays < 1 or a.rounds < 1 or a.warmup < 0):
        ap.error("--grid >= 4, --rays and --rounds positive, --warmup non-negative")
    if not torch.cuda.is_available():
        sys.exit("bench_raygrad: needs a GPU")
    drrt.options.check_failed = False
    print(json.dumps(a.run(a, torch.device("cuda:0"))))


if __name__ == "__main__":
    main()
