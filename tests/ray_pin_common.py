"""What test_ray_adjoint_pin.py checks and tests/golden/make_golden.py records: the host builds of the grid ray-state adjoints
on their scenes, as built and with non-finite seeds, and the layout of the fixture.  A plain module: no fixtures, no tests."""
import numpy as np

import hostcheck_lib as HC
import integral_common as IC
import integral_host as OH
import raygrad_common as RC
import target_raygrad_host as TH

SCENES = ("lens16_h1_multi", "box7x11x5_h05_multi")
COUNTS = ("steps", "fwd", "jstar", "failed", "again")       # per ray, where the routine has them


def nonfinite_seed(dx):
    dx = dx.copy()
    dx[::7] = np.inf
    dx[3::11] = np.nan
    return dx


def replaced(n):
    """The rays whose seed nonfinite_seed replaces."""
    m = np.zeros(n, bool)
    m[::7] = True
    m[3::11] = True
    return m


def _rays(s):
    k = HC.trace(s["rif"], s["res"], s["pos"], s["vel"], s["h"], s["ds"])
    return HC.backtrace_rays(s["rif"], s["res"], s["pos"], s["vel"], k["xt"], k["vt"], k["steps"], s["dx"], s["dv"],
                             s["h"], s["ds"])


def _opl(s):
    k = OH.trace_opl(s["rif"], s["res"], s["pos"], s["vel"], s["h"], s["ds"])
    return OH.backtrace_opl(s["rif"], s["res"], s["pos"], s["vel"], k["xt"], k["vt"], k["steps"], s["dx"], s["dv"],
                            s["dopl"], s["h"], s["ds"])


def _target(s, dd2):
    return TH.backtrace_target_rays(s["rif"], s["res"], s["pos"], s["vel"], s["tg"], s["dx"], s["dv"], s["h"], s["ds"],
                                    ddist2=s["dd2"] if dd2 else None)


ROUTINES = {
    # name: (scene builder, host build)
    "rays": (RC.scene, _rays),
    "pln": (lambda name: RC.plane_scene(name, "tilted"), RC.host_plane),
    "sdf": (RC.sdf_scene, RC.host_sdf),
    "target": (lambda name: RC.target_scene(name, "nozero"), lambda s: _target(s, True)),
    "target_nodd2": (lambda name: RC.target_scene(name, "nozero"), lambda s: _target(s, False)),
    "opl": (IC.scene, _opl),
}

_runs = {}


def run(name, routine, variant):
    """-> (the routine's result dict, the seeds (n, 6) it was given) on the scene, `variant` = "built" or "nonfinite"; once
    per session."""
    key = (name, routine, variant)
    if key not in _runs:
        scene, host = ROUTINES[routine]
        s = scene(name)
        if variant == "nonfinite":
            s = dict(s, dx=nonfinite_seed(s["dx"]))
        _runs[key] = (host(s), np.concatenate([s["dx"], s["dv"]], 1))
    return _runs[key]


def record(name, routine):
    """-> {fixture key: array}, per recording: `grad` = the bits of (dpos, dvel) XOR those of (dx, dv), (n, 6) uint32;
    `counts` = the fields of COUNTS the routine has, one row each; the call's totals where it has no per-ray count."""
    out = {}
    for variant in ("built", "nonfinite"):
        r, seeds = run(name, routine, variant)
        rows = replaced(len(seeds)) if variant == "nonfinite" else np.ones(len(seeds), bool)
        grad = np.concatenate([r["dpos"], r["dvel"]], 1)
        assert grad.dtype == seeds.dtype == np.float32
        key = f"{name}.{routine}.{variant}."
        out[key + "grad"] = np.ascontiguousarray(grad[rows]).view(np.uint32) ^ np.ascontiguousarray(seeds[rows]).view(np.uint32)
        if "steps" in r:
            out[key + "counts"] = np.stack([r[f][rows].astype(np.uint32) for f in COUNTS if f in r])
        else:
            out[key + "totals"] = np.array([r["ray_steps"], r["n_failed"]], np.int64)
    return out
