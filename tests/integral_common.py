"""What the integral-operator test files (test_opl.py, test_field_integral.py, test_emission.py, test_vector_integral.py,
test_path.py, their fuzz files, test_ray_adjoint_pin.py) share: the box march's scenes with seeds on all three outputs, the
tie-free reference with its cache, the bars, the second fields and the closed-form case.  A plain module: no fixtures, no
tests.  Everything cached is computed once per key and handed out unchanged."""
import numpy as np
import torch

import cases
import integral_ad
import integral_host as OH
from raygrad_common import GRAD_TOL, SCENES, TIE_TOL, grid, max_steps_fwd, ray_sets

# Relative error of the fp32 opl against float64 on tie-free rays.  A priori: K 2^-24 for the accumulate (K <= 128) plus
# TIE_TOL |grad n| / n for the samples taken TIE_TOL apart: <~ 2e-5.  4 x the largest value measured on the host build
# (4.95e-7, the plane source of test_plane_source_on_host; 4.45e-7 on lens16_h05_half), rounded up to one digit; the margin
# is for another compiler or libm.  May not exceed 1e-4: more would mean the accumulate is wrong.
OPL_TOL = 2e-6
# rel-L2 over the grid of dL/dn against float64 autograd (flag on).  4 x the largest value measured on the host build
# (4.04e-6, box7x11x5_h05_multi without seeds on the rays), rounded up to one digit; may not exceed GRAD_TOL.
GRID_TOL = 2e-5
assert OPL_TOL <= 1e-4 and GRID_TOL <= GRAD_TOL
ATOMIC_TOL = 2e-5       # grid gradient, kernel vs host build: only the order of the sums differs (tests/test_gpu_parity.py's bar)
KINDS = ("plane", "point", "inside", "face", "never", "graze")


# ---- scenes ---------------------------------------------------------------------------------------------------------
_scenes = {}


def scene(name, seed=0):
    """The box march's scene (raygrad_common) with seeds on all three outputs: <= 672 rays, <= 128 iterations."""
    if (name, seed) in _scenes:
        return _scenes[name, seed]
    kind, h, ds = SCENES[name]
    rif = grid(kind)
    D, H, W = rif.shape
    ext = ((W - 1) * h, (H - 1) * h, (D - 1) * h)
    sets = ray_sets(ext, ds, seed)
    pos = np.concatenate([s[0] for s in sets.values()])
    vel = np.concatenate([s[1] for s in sets.values()])
    labels = np.concatenate([[k] * len(s[0]) for k, s in sets.items()])
    rng = np.random.default_rng(seed + 11)
    s = dict(rif=rif, res=(W, H, D), h=h, ds=ds, pos=pos, vel=vel, labels=labels,
             dx=rng.normal(size=pos.shape).astype(np.float32), dv=rng.normal(size=pos.shape).astype(np.float32),
             dopl=rng.normal(size=len(pos)).astype(np.float32))
    assert len(pos) <= 672 and len(pos) % 256 != 0 and max_steps_fwd(s["res"], h, ds) <= 128
    _scenes[name, seed] = s
    return s


_refs = {}


def reference(oracle, s, key):
    """Host fp32 forward, fp64 forward, tie-free mask (tests/test_raygrad.py::reference) and the float64 opl; once per `key`."""
    if key in _refs:
        return _refs[key]
    k = OH.trace_opl(s["rif"], s["res"], s["pos"], s["vel"], s["h"], s["ds"])
    o64 = oracle.trace(s["rif"], s["res"], s["pos"], s["vel"], s["h"], s["ds"], dtype=np.float64)
    ms = max_steps_fwd(s["res"], s["h"], s["ds"])
    ok = k["steps"] < ms
    tie_free = ok & (o64["steps"] == k["steps"]) & \
        (np.abs(o64["xt"] - k["xt"]).max(1) <= TIE_TOL) & (np.abs(o64["vt"] - k["vt"]).max(1) <= TIE_TOL)
    T = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)      # noqa: E731
    with torch.no_grad():
        opl64 = integral_ad.trace_opl(T(s["rif"]), T(s["pos"]), T(s["vel"]), s["h"], s["ds"])[2].numpy()
    _refs[key] = (k, tie_free, opl64, ms)
    return _refs[key]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(got, want):
    got = got.cpu().numpy()
    return np.array_equal(np.isfinite(got), np.isfinite(want)) and np.array_equal(got, want, equal_nan=True)


def _plane_case(h=1.0):
    """A 12^2 plane source outside the y = 0 face of cases.luneburg(16) (tracer.* pass rif.shape as res)."""
    ds = h / 2
    rng = np.random.default_rng(3)
    u = (np.stack(np.meshgrid(np.arange(12), np.arange(12), indexing="ij"), -1).reshape(-1, 2) + rng.random((144, 2))) / 12
    pos = (np.stack([1.0 + 13.0 * u[:, 0], np.full(144, -0.15), 1.0 + 13.0 * u[:, 1]], -1).astype(np.float32) * np.float32(h))
    vel = rng.normal(0, 0.05, (144, 3)); vel[:, 1] = 1.0
    vel = (vel / np.linalg.norm(vel, axis=1, keepdims=True)).astype(np.float32)
    return dict(rif=cases.luneburg(16), res=(16, 16, 16), h=h, ds=ds, pos=pos, vel=vel,
                dx=rng.normal(size=pos.shape).astype(np.float32), dv=rng.normal(size=pos.shape).astype(np.float32),
                dopl=rng.normal(size=144).astype(np.float32))


def make_field(shape, seed):
    """Seeded, fp32, smooth, >= 0.55: 1 + 0.4 (mean of sines of different periods and phases along the three axes) + 0.05
    uniform noise.  Not symmetric under a permutation of the axes."""
    D, H, W = shape
    z, y, x = np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing="ij")
    s = (np.sin(0.9 * x + 0.3) + np.sin(0.5 * y + 1.1) + np.sin(1.3 * z + 2.0)) / 3.0
    return (1.0 + 0.4 * s + 0.05 * np.random.default_rng(seed + 23).random(shape)).astype(np.float32)


# the dyadic rays of tests/test_opl.py::test_uniform_medium_closed_form: the fp32 march is exact
_RES, _H, _DS, _C = (9, 8, 7), 1.0, 0.5, 1.25
_POS = np.array([(3.25, -1.25, 3.5), (0.0, 2.5, 1.125), (4.5, 3.5, 2.75), (-2.0, 3.0, 3.0), (7.875, 6.75, 5.5)], np.float32)
_VEL = np.array([(0.25, 1.0, 0.125), (1.0, 0.0, 0.0), (-0.5, 0.25, 0.75), (1.0, 0.125, -0.25), (0.125, 0.125, 0.0625)], np.float32)
_DTAU = np.array([0.7, -1.3, 0.4, 2.0, -0.6], np.float32)


def _in_box_samples(steps):
    """Per ray, the boolean mask over k < K of the samples x_k = p0 + k ds v0 that fall in the box (float64: exact here)."""
    ext = np.array([_RES[0] - 1, _RES[1] - 1, _RES[2] - 1], np.float64) * _H
    out = []
    for i in range(len(_POS)):
        x = _POS[i].astype(np.float64) + _DS * np.arange(int(steps[i]))[:, None] * _VEL[i].astype(np.float64)
        out.append(((x >= 0) & (x < ext)).all(1))
    return out
