"""The host builds of the grid ray-state adjoints against their own past: tests/golden/ray_adjoints_host.npz holds what
backtrace_rays, backtrace_pln_rays, backtrace_sdf_rays, backtrace_target_rays (with and without the seed on dist2) and
backtrace_opl (the term-carrying representative of the integral family) of tests/hostcheck returned when the fixture was
recorded (tests/golden/make_golden.py ray_adjoints_host), and every array must come out byte for byte.  The other referees
compare these routines with float64 autograd within GRAD_TOL and the kernels with the host builds bit for bit; this one is
what a refactor of the reverse march has to keep.  CPU only.

Each case is recorded as its scene builder makes it and once more with dx[::7] = inf, dx[3::11] = nan.  Two things keep the
fixture small, neither loses a bit:
  * the rays of a call do not see each other's seeds, so of the second recording the fixture keeps the rows of the rays
    whose seed was replaced, and the test holds the other rows against the first recording;
  * (dpos, dvel) are stored as their bit pattern XOR that of the seeds (dx, dv), which the builders give: zeros for every
    ray whose gradient is the identity."""
import os

import numpy as np
import pytest

import hostcheck_lib as HC
import integral_host as OH
import target_raygrad_host as TH
import test_opl
import test_raygrad
import test_stop_raygrad as SR
import test_target_raygrad as TR

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ray_adjoints_host.npz")
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
    "rays": (test_raygrad.scene, _rays),
    "pln": (lambda name: SR.plane_scene(name, "tilted"), SR.host_plane),
    "sdf": (SR.sdf_scene, SR.host_sdf),
    "target": (lambda name: TR.target_scene(name, "nozero"), lambda s: _target(s, True)),
    "target_nodd2": (lambda name: TR.target_scene(name, "nozero"), lambda s: _target(s, False)),
    "opl": (test_opl.scene, _opl),
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


@pytest.fixture(scope="module")
def golden():
    with np.load(FIXTURE) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("routine", list(ROUTINES))
@pytest.mark.parametrize("name", SCENES)
def test_host_build_is_the_recorded_one(golden, name, routine):
    got = record(name, routine)
    want = {k: v for k, v in golden.items() if k.startswith(f"{name}.{routine}.")}
    assert sorted(got) == sorted(want) and len(got) == 4
    for k in sorted(got):
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert got[k].tobytes() == want[k].tobytes(), k
    # the rays whose seed stayed: what the first recording holds
    (b, _), (v, seeds) = run(name, routine, "built"), run(name, routine, "nonfinite")
    keep = ~replaced(len(seeds))
    for f in ("dpos", "dvel") + COUNTS:
        if f in b:
            assert v[f][keep].tobytes() == b[f][keep].tobytes(), f
    assert not np.isfinite(v["dpos"][~keep]).all()


def test_fixture_holds_nothing_else(golden):
    assert {k.split(".")[0] for k in golden} == set(SCENES) and {k.split(".")[1] for k in golden} == set(ROUTINES)
