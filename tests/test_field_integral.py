"""Line integral of a second field along bent rays: drrt_trace_field_f32 / drrt_backtrace_field_f32, TracerC.trace_field /
backtrace_field, tracer.FieldIntegralTracerC.

CPU tier: the host build of the product's per-ray routines (tests/hostcheck/integral_rays.hip: trace_field_ray and
field_backtrace_ray of csrc/drrt_device.h) against the product's own trace and trace_opl_ray (bit for bit), against float64
torch.autograd through tests/integral_ad (its one loop with tau += ds n a) on the tie-free rays of
tests/integral_common.py::reference, against closed forms, against opl_backtrace_ray with field = rif, and the C ABI's argument
checks.  GPU tier: the field kernels of drrt_integral.hip against that host build, the autograd class end to end, its launches, and
the demo.  The scenes, ray sets and the plane source are tests/integral_common.py's; the second field of a scene is seeded, smooth,
strictly positive and not symmetric under a permutation of the axes.

On the parent commit every test here fails: tests/hostcheck/integral_rays.hip does not compile (no trace_field_ray), the
library has no such C symbols, TracerC no such methods, tracer no such class and examples/ no such demo.

Mutation checks (tried by hand on field_backtrace_ray, one at a time, each then undone; CPU tier):
  * without the lambda source term (the three fmaf(fv, grad a_k, lambda) dropped): all ten cases of
    test_adjoint_matches_float64_autograd, test_plane_source_on_host, test_linear_field_closed_form,
    test_exit_on_first_iteration_closed_form and all five cases of test_consistent_with_opl fail;
  * dn without dtau a_k (dn = mu . grad n_k): all ten cases of test_adjoint_matches_float64_autograd,
    test_plane_source_on_host, test_uniform_field_closed_form, test_exit_on_first_iteration_closed_form and all five cases
    of test_consistent_with_opl fail."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import cases
import hostcheck_lib as HC
import integral_ad
import integral_common as IC
import integral_host as OH
from integral_common import _C, _DS, _DTAU, _H, _POS, _RES, _VEL, _in_box_samples, make_field
from oracle import torch_ad
from raygrad_common import GRAD_TOL, SCENES, _t, rel_err

# Relative error of the fp32 tau against float64 on tie-free rays.  A priori as for OPL_TOL of tests/test_opl.py: K 2^-24 for
# the accumulate (K <= 128) plus TIE_TOL (|grad n| / n + |grad a| / a) for the samples taken TIE_TOL apart: <~ 3e-5.  4 x
# the largest value measured on the host build (1.015e-6, lens16_h05_half; 4.39e-7 on the plane source of
# test_plane_source_on_host), rounded up to one digit; the margin is for another compiler or libm.  May not exceed 1e-4:
# more would mean the accumulate is wrong.
TAU_TOL = 5e-6
# rel-L2 over the grid of dL/dfield against float64 autograd.  4 x the largest value measured on the host build (4.39e-6,
# lens16_h05_half, with and without seeds on the rays; 3.20e-6 on the plane source), rounded up to one digit; may not
# exceed GRAD_TOL.
FIELD_TOL = 2e-5
GRID_TOL = IC.GRID_TOL  # dL/drif: the bar of tests/test_opl.py (2e-5)
assert TAU_TOL <= 1e-4 and FIELD_TOL <= GRAD_TOL and GRID_TOL == 2e-5
ATOMIC_TOL = 2e-5       # grid gradients, kernel vs host build: only the order of the sums differs (tests/test_gpu_parity.py's bar)
KINDS = IC.KINDS
_bits = IC._bits


# ---- scenes ---------------------------------------------------------------------------------------------------------
_scenes = {}


def scene(name):
    """tests/integral_common.py's scene (<= 672 rays, not a multiple of 256, <= 128 iterations) with its second field; the seed on
    opl serves as the seed on tau."""
    if name not in _scenes:
        s = dict(IC.scene(name))
        s["field"] = make_field(s["rif"].shape, list(SCENES).index(name))
        s["dtau"] = s["dopl"]
        assert s["field"].min() > 0.5 and s["field"].dtype == np.float32
        _scenes[name] = s
    return _scenes[name]


def plane_case(h=1.0):
    s = dict(IC._plane_case(h))
    s["field"] = make_field(s["rif"].shape, 7)
    s["dtau"] = s["dopl"]
    return s


_refs = {}


def reference(oracle, s, key):
    """tests/integral_common.py::reference (host fp32 forward, fp64 forward, its tie-free mask) plus the host trace_field and the
    float64 tau; once per `key`."""
    if key not in _refs:
        _, tie_free, _, ms = IC.reference(oracle, s, key)
        k = OH.trace_field(s["rif"], s["field"], s["res"], s["pos"], s["vel"], s["h"], s["ds"])
        T = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)      # noqa: E731
        with torch.no_grad():
            tau64 = integral_ad.trace_field(T(s["rif"]), T(s["field"]), T(s["pos"]), T(s["vel"]), s["h"], s["ds"])[2].numpy()
        _refs[key] = (k, tie_free, tau64, ms)
    return _refs[key]


_ad = {}


def autograd64(s, dx, dv, dtau, key=None):
    """float64 torch.autograd of L = <dx, xt> + <dv, vt> + <dtau, tau> through integral_ad
    -> (dL/drif, dL/dfield, dL/dpos, dL/dvel); kept under `key` for the tests that share it."""
    if key is not None and key in _ad:
        return _ad[key]
    T = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)      # noqa: E731
    r, f, p, v = (T(s[k]).requires_grad_(True) for k in ("rif", "field", "pos", "vel"))
    xt, vt, tau, _ = integral_ad.trace_field(r, f, p, v, s["h"], s["ds"])
    L = (xt * T(dx)).sum() + (vt * T(dv)).sum() + (tau * T(dtau)).sum()
    gr, gf, gp, gv = torch.autograd.grad(L, (r, f, p, v))
    out = gr.numpy().reshape(-1), gf.numpy().reshape(-1), gp.numpy(), gv.numpy()
    if key is not None:
        _ad[key] = out
    return out


def host_back(s, k, dx, dv, dtau, **kw):
    return OH.backtrace_field(s["rif"], s["field"], s["res"], s["pos"], s["vel"], k["xt"], k["vt"], k["steps"], dx, dv, dtau,
                              s["h"], s["ds"], **kw)


# ---- CPU tier -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SCENES))
def test_forward_is_trace(name):
    """trace_field_ray's (xt, vt, steps, n_failed) == the product's trace_ray<0> (tests/hostcheck), bit for bit."""
    s = scene(name)
    k = OH.trace_field(s["rif"], s["field"], s["res"], s["pos"], s["vel"], s["h"], s["ds"])
    t = HC.trace(s["rif"], s["res"], s["pos"], s["vel"], s["h"], s["ds"])
    assert np.array_equal(_bits(k["xt"]), _bits(t["xt"])) and np.array_equal(_bits(k["vt"]), _bits(t["vt"]))
    assert np.array_equal(k["steps"].astype(np.int64), t["steps"].astype(np.int64)) and k["n_failed"] == t["n_failed"] > 0


@pytest.mark.parametrize("name", list(SCENES))
def test_field_equal_to_rif_is_opl(name):
    """field = rif (the same values): tau == trace_opl_ray's opl, bit for bit."""
    s = scene(name)
    k = OH.trace_field(s["rif"], s["rif"].copy(), s["res"], s["pos"], s["vel"], s["h"], s["ds"])
    o = OH.trace_opl(s["rif"], s["res"], s["pos"], s["vel"], s["h"], s["ds"])
    assert np.array_equal(_bits(k["tau"]), _bits(o["opl"])) and np.abs(o["opl"]).max() > 1.0
    assert np.array_equal(_bits(k["xt"]), _bits(o["xt"])) and np.array_equal(k["steps"], o["steps"])


@pytest.mark.parametrize("name", list(SCENES))
def test_tau_matches_float64(oracle, name):
    s = scene(name)
    k, tie_free, tau64, ms = reference(oracle, s, name)
    lab = s["labels"]
    for kind in KINDS:
        assert tie_free[lab == kind].sum() >= 10, kind
    m = tie_free & (tau64 > 0)
    err = np.abs(k["tau"].astype(np.float64) - tau64)[m] / tau64[m]
    print(f"{name}: {tie_free.sum()} tie-free rays, {m.sum()} with tau > 0 (max {tau64[m].max():.3f}); "
          f"tau rel err max {err.max():.3e} median {np.median(err):.3e}")
    assert m.sum() >= 40 and err.max() <= TAU_TOL
    never = (lab == "never") & (k["steps"] < ms)
    assert never.sum() > 0 and np.array_equal(_bits(k["tau"][never]), np.zeros(never.sum(), np.uint32))
    assert not tau64[never].any()


def _check_adjoint(s, k, tie_free, seeded, label, key):
    z = tie_free[:, None] if seeded else np.zeros((len(tie_free), 1), bool)
    dx, dv, dtau = s["dx"] * z, s["dv"] * z, s["dtau"] * tie_free
    r = host_back(s, k, dx if seeded else None, dv if seeded else None, dtau, corrected_h=True)
    gr, gf, gp, gv = autograd64(s, dx, dv, dtau, key=(key, seeded))
    err = rel_err(r["dpos"], r["dvel"], gp, gv)[tie_free]
    gerr, ferr = cases.rel_l2(r["grad"], gr), cases.rel_l2(r["grad_field"], gf)
    print(f"{label} rays_seeded={seeded}: {tie_free.sum()} tie-free rays, ray grad rel err max {err.max():.3e} median "
          f"{np.median(err):.3e}; dL/drif rel-L2 {gerr:.3e} (|grad| {np.linalg.norm(gr):.3e}); dL/dfield rel-L2 {ferr:.3e} "
          f"(|grad| {np.linalg.norm(gf):.3e})")
    assert np.linalg.norm(gr) > 0.1 and np.linalg.norm(gf) > 0.1 and np.abs(gp[tie_free]).max() > 1e-3
    assert err.max() <= GRAD_TOL
    assert gerr <= GRID_TOL
    assert ferr <= FIELD_TOL
    return r


@pytest.mark.parametrize("rays_seeded", [True, False])
@pytest.mark.parametrize("name", list(SCENES))
def test_adjoint_matches_float64_autograd(oracle, name, rays_seeded):
    """Flag on: (dpos, dvel) per ray, dL/drif and dL/dfield over the grid against float64 autograd of
    L = <dx, xt> + <dv, vt> + <dtau, tau>, and once more with dx = dv = 0; seeds of the rays that are not tie-free zeroed on
    both sides."""
    s = scene(name)
    k, tie_free, _, ms = reference(oracle, s, name)
    r = _check_adjoint(s, k, tie_free, rays_seeded, name, name)
    assert r["n_failed"] == int((k["steps"] >= ms).sum()) == k["n_failed"]


def test_plane_source_on_host(oracle):
    """The scene of the GPU tier's end-to-end test, on the host build: it is part of what TAU_TOL and FIELD_TOL were
    measured on."""
    s = plane_case()
    k, tie_free, tau64, _ = reference(oracle, s, "plane12")
    terr = (np.abs(k["tau"] - tau64) / tau64)[tie_free].max()
    print(f"plane source: tau rel err {terr:.3e}")
    assert tie_free.sum() >= 120 and terr <= TAU_TOL
    for seeded in (True, False):
        _check_adjoint(s, k, tie_free, seeded, "plane source", "plane12")


@pytest.mark.parametrize("name", list(SCENES))
def test_failed_and_never_entered_rays(oracle, name):
    """Failed rays: zeros, counted, no contribution to either grid.  Never-entered rays: (dx, dv) exactly, no contribution."""
    s = scene(name)
    k, _, _, ms = reference(oracle, s, name)
    lab = s["labels"]
    r = host_back(s, k, s["dx"], s["dv"], s["dtau"])
    failed = k["steps"] >= ms
    assert failed[np.where(lab == "zero")[0][:48]].all()
    assert np.array_equal(r["failed"], failed) and r["n_failed"] == int(failed.sum()) == k["n_failed"] > 0
    assert not r["dpos"][failed].any() and not r["dvel"][failed].any() and not r["steps"][failed].any()
    never = (lab == "never") & ~failed
    assert never.sum() >= 10
    assert np.array_equal(_bits(r["dpos"][never]), _bits(s["dx"][never])) and np.array_equal(_bits(r["dvel"][never]), _bits(s["dv"][never]))
    quiet = failed | never
    q = OH.backtrace_field(s["rif"], s["field"], s["res"], s["pos"][quiet], s["vel"][quiet], k["xt"][quiet], k["vt"][quiet],
                           k["steps"][quiet], s["dx"][quiet], s["dv"][quiet], s["dtau"][quiet], s["h"], s["ds"])
    assert not q["grad"].any() and not q["grad_field"].any() and q["ray_steps"] == 0
    assert np.abs(r["grad"]).max() > 0 and np.abs(r["grad_field"]).max() > 0
    assert r["ray_steps"] == int(r["steps"].astype(np.int64).sum()) > 0


def test_uniform_field_closed_form():
    """n = c and a = b everywhere: tau = ds c b (in-box samples), one rounding per term of the sum -- every term ds c * b is
    exact here; with seeds on tau alone the gradients sum to sum_rays dtau ds c m (dL/dfield) and sum_rays dtau ds b m
    (dL/drif: the value weights of a splat sum to its value, the gradient splat to zero), and nothing pulls on the rays."""
    b = 0.75
    rif = np.full((_RES[2], _RES[1], _RES[0]), _C, np.float32)
    fld = np.full_like(rif, b)
    k = OH.trace_field(rif, fld, _RES, _POS, _VEL, _H, _DS)
    m = np.array([int(x.sum()) for x in _in_box_samples(k["steps"])], np.int64)
    assert (k["steps"] < IC.max_steps_fwd(_RES, _H, _DS)).all() and m.min() >= 2 and m.max() >= 12 and len(set(m)) >= 4
    exact = _DS * _C * b * m
    assert (np.abs(k["tau"].astype(np.float64) - exact) <= m * 2.0 ** -24 * exact).all(), (k["tau"], exact)
    r = OH.backtrace_field(rif, fld, _RES, _POS, _VEL, k["xt"], k["vt"], k["steps"], None, None, _DTAU, _H, _DS)
    assert np.array_equal(r["steps"].astype(np.int64), m)
    d = _DTAU.astype(np.float64)
    np.testing.assert_allclose(r["grad_field"].sum(), (d * _DS * _C * m).sum(), rtol=1e-6)
    np.testing.assert_allclose(r["grad"].sum(), (d * _DS * b * m).sum(), rtol=1e-6)
    one = OH.backtrace_field(rif, fld, _RES, _POS[1:2], _VEL[1:2], k["xt"][1:2], k["vt"][1:2], k["steps"][1:2], None, None,
                             _DTAU[1:2], _H, _DS)
    np.testing.assert_allclose(one["grad_field"].sum(), d[1] * _DS * _C * m[1], rtol=1e-6)
    np.testing.assert_allclose(one["grad"].sum(), d[1] * _DS * b * m[1], rtol=1e-6)
    assert not r["dpos"].any() and not r["dvel"].any()


def test_linear_field_closed_form():
    """n = c, a = a0 + g . p (trilinear interpolation is exact for it; a0, g dyadic and h = 1, so the taps and their
    differences are exact in fp32).  The medium bends nothing: x_k = p0 + k ds v0, and for a ray whose in-box samples are
    k = e .. K - 1, tau = sum_k ds c (a0 + g . x_k), so with seeds on tau alone
        dpos = dtau ds c m g,   dvel = dtau ds^2 c (sum_k k) g.
    Only the lambda source term (dtau ds n_k) grad a_k produces these: grad n = 0 here."""
    a0, g = 4.0, np.array([0.5, -0.25, 0.125])
    rif = np.full((_RES[2], _RES[1], _RES[0]), _C, np.float32)
    z, y, x = np.meshgrid(np.arange(_RES[2]), np.arange(_RES[1]), np.arange(_RES[0]), indexing="ij")
    fld = (a0 + g[0] * x + g[1] * y + g[2] * z).astype(np.float32)
    assert fld.min() > 0
    k = OH.trace_field(rif, fld, _RES, _POS, _VEL, _H, _DS)
    masks = _in_box_samples(k["steps"])
    m, ksum, tau = [], [], []
    for i, inb in enumerate(masks):
        idx = np.where(inb)[0]
        assert len(idx) >= 2 and np.array_equal(idx, np.arange(idx[0], int(k["steps"][i])))     # k = e .. K - 1
        xs = _POS[i].astype(np.float64) + _DS * idx[:, None] * _VEL[i].astype(np.float64)
        m.append(len(idx)); ksum.append(int(idx.sum())); tau.append((_DS * _C * (a0 + xs @ g)).sum())
    m, ksum = np.array(m, np.float64), np.array(ksum, np.float64)
    assert (np.array([mm[0] for mm in masks]) == False).sum() >= 2 and ksum.max() > 50          # noqa: E712 (rays that start outside)
    np.testing.assert_allclose(k["tau"], tau, rtol=1e-6)
    r = OH.backtrace_field(rif, fld, _RES, _POS, _VEL, k["xt"], k["vt"], k["steps"], None, None, _DTAU, _H, _DS)
    d = _DTAU.astype(np.float64)
    np.testing.assert_allclose(r["dpos"], (d * _DS * _C * m)[:, None] * g[None, :], rtol=1e-5)
    np.testing.assert_allclose(r["dvel"], (d * _DS * _DS * _C * ksum)[:, None] * g[None, :], rtol=1e-5)
    assert np.abs(r["dpos"]).min() > 1e-2 and np.abs(r["dvel"]).min() > 1e-2
    np.testing.assert_allclose(r["grad_field"].sum(), (d * _DS * _C * m).sum(), rtol=1e-6)


def test_exit_on_first_iteration_closed_form():
    """e = 0, K = 1 (the case of tests/test_opl.py): tau = ds n(x0) a(x0), dvel = mu = dv + ds dx,
    dpos = dx + ds J(x0)^T mu + dtau ds (a grad n + n grad a), J = d(n grad n)/dx at x0."""
    rif = cases.luneburg(16)
    fld = make_field(rif.shape, 5)
    h, ds, res = 1.0, 0.5, (16, 16, 16)
    pos = np.array([[14.8, 7.3, 6.1]], np.float32)          # half a step from the far x face, heading out
    vel = np.array([[1.0, 0.1, -0.05]], np.float32)
    k = OH.trace_field(rif, fld, res, pos, vel, h, ds)
    assert k["steps"][0] == 1
    dx = np.array([[0.3, -1.2, 0.7]], np.float32); dv = np.array([[-0.4, 0.9, 0.2]], np.float32)
    dtau = np.array([1.7], np.float32)
    r = OH.backtrace_field(rif, fld, res, pos, vel, k["xt"], k["vt"], k["steps"], dx, dv, dtau, h, ds)
    R, F = torch.tensor(rif, dtype=torch.float64), torch.tensor(fld, dtype=torch.float64)
    x = torch.tensor(pos[0], dtype=torch.float64)
    inside = torch.tensor([True])
    n, g = (t[0].numpy() for t in torch_ad.eval_grad(R, x[None], h, inside))
    a, ga = (t[0].numpy() for t in torch_ad.eval_grad(F, x[None], h, inside))
    f = lambda y: (lambda nn, gg: (nn[:, None] * gg)[0])(*torch_ad.eval_grad(R, y[None], h, inside))   # noqa: E731
    J = torch.autograd.functional.jacobian(f, x).numpy()
    mu = dv[0].astype(np.float64) + ds * dx[0]
    pull_n, pull_a = float(dtau[0]) * ds * float(a) * g, float(dtau[0]) * ds * float(n) * ga
    assert np.abs(pull_n).max() > 1e-2 and np.abs(pull_a).max() > 1e-2
    np.testing.assert_allclose(k["tau"][0], ds * float(n) * float(a), rtol=1e-6)
    np.testing.assert_allclose(r["dvel"][0], mu, rtol=1e-6)
    np.testing.assert_allclose(r["dpos"][0], dx[0] + ds * J.T @ mu + pull_n + pull_a, rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("name", list(SCENES))
def test_consistent_with_opl(name):
    """field = rif: tau is opl, so (dpos, dvel) are opl_backtrace_ray's and dL/drif + dL/dfield is its grid gradient.  Both
    sides are within one bar (GRAD_TOL, GRID_TOL) of the same float64 result, hence two bars here."""
    s = dict(scene(name))
    s["field"] = s["rif"].copy()
    k = OH.trace_field(s["rif"], s["field"], s["res"], s["pos"], s["vel"], s["h"], s["ds"])
    ok = k["steps"] < IC.max_steps_fwd(s["res"], s["h"], s["ds"])
    r = host_back(s, k, s["dx"], s["dv"], s["dtau"])
    o = OH.backtrace_opl(s["rif"], s["res"], s["pos"], s["vel"], k["xt"], k["vt"], k["steps"], s["dx"], s["dv"], s["dtau"],
                         s["h"], s["ds"])
    err = rel_err(r["dpos"], r["dvel"], o["dpos"].astype(np.float64), o["dvel"].astype(np.float64))[ok]
    gerr = cases.rel_l2(r["grad"] + r["grad_field"], o["grad"])
    print(f"{name}: vs opl_backtrace_ray: ray grad rel err max {err.max():.3e}; grid rel-L2 {gerr:.3e}")
    assert err.max() <= 2 * GRAD_TOL and gerr <= 2 * GRID_TOL
    assert np.linalg.norm(o["grad"]) > 0.1 and np.linalg.norm(r["grad_field"]) > 0.1
    assert np.array_equal(r["steps"], o["steps"]) and np.array_equal(r["failed"], o["failed"])


def test_flag_off_scales_the_gradient_splat(oracle):
    """h = 0.5: without DRRT_FLAG_CORRECTED_H dL/drif is the flag-on run's value part plus h times its gradient-splat part
    (the bound of tests/test_opl.py's test: <= 4 roundings per corner, 1e-6 over the grid with room); dL/dfield, which has
    no gradient splat, and the ray gradients are bit-identical with the flag on and off."""
    name = "lens16_h05_half"
    s = scene(name)
    assert s["h"] == 0.5
    k = reference(oracle, s, name)[0]
    run = lambda **kw: host_back(s, k, s["dx"], s["dv"], s["dtau"], **kw)      # noqa: E731
    off, on = run(corrected_h=False), run(corrected_h=True)
    val, spl = run(corrected_h=True, parts=1), run(corrected_h=True, parts=2)
    assert np.array_equal(spl["grad"] * s["h"], run(corrected_h=False, parts=2)["grad"])
    assert np.array_equal(val["grad"], run(corrected_h=False, parts=1)["grad"])
    assert cases.rel_l2(val["grad"] + spl["grad"], on["grad"]) <= 1e-6
    err = cases.rel_l2(val["grad"] + s["h"] * spl["grad"], off["grad"])
    print(f"flag off vs value + h * splat: rel-L2 {err:.3e}; |value| {np.linalg.norm(val['grad']):.3e} |splat| {np.linalg.norm(spl['grad']):.3e}")
    assert err <= 1e-6
    assert cases.rel_l2(off["grad"], on["grad"]) > 0.1 and np.linalg.norm(val["grad"]) > 0 and np.linalg.norm(spl["grad"]) > 0
    # dL/dfield: value weights only, the same with either setting
    assert np.array_equal(off["grad_field"], on["grad_field"]) and np.linalg.norm(on["grad_field"]) > 0.1
    assert np.array_equal(val["grad_field"], on["grad_field"]) and not spl["grad_field"].any()
    assert np.array_equal(_bits(off["dpos"]), _bits(on["dpos"])) and np.array_equal(_bits(off["dvel"]), _bits(on["dvel"]))


def test_abi_and_python_surface():
    """The C symbols are exported and bound, the profile ids are appended, the methods and the class exist."""
    from adjointnonlinearraytracing_amd import _lib, drrt, tracer
    lib = C.CDLL(_lib.LIB_PATH)
    for name in ("drrt_trace_field_f32", "drrt_backtrace_field_f32"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    assert _lib.PROF_NAMES[13] == "trace_field" and _lib.PROF_NAMES[14] == "backtrace_field" and max(_lib.PROF_NAMES) == 14
    assert _lib.PROF_NAMES[11] == "trace_opl" and _lib.PROF_NAMES[12] == "backtrace_opl"
    assert _lib.PROF_NAMES[10] == "backtrace_target_rays" and _lib.PROF_NAMES[6] == "backtrace_rays" and _lib.PROF_NAMES[1] == "trace"
    assert callable(drrt.TracerC.trace_field) and callable(drrt.TracerC.backtrace_field)
    assert issubclass(tracer.FieldIntegralTracerC, torch.autograd.Function)
    with open(os.path.join(os.path.dirname(_lib.LIB_PATH), "..", "include", "drrt_hip.h")) as f:
        hdr = f.read()
    assert "drrt_trace_field_f32" in hdr and "drrt_backtrace_field_f32" in hdr
    assert "#define DRRT_PROF_TRACE_FIELD 13" in hdr and "#define DRRT_PROF_BACKTRACE_FIELD 14" in hdr
    assert "#define DRRT_PROF_TRACE_OPL 11" in hdr and "#define DRRT_PROF_BACKTRACE_OPL 12" in hdr


def test_abi_argument_checks():
    """Null pointers, all outputs null, too many rays and bad steps are refused before anything is launched; n = 0 is fine."""
    from adjointnonlinearraytracing_amd import _lib
    lib = _lib.load()
    rif = np.ones(8 * 8 * 8, np.float32)
    a = np.zeros((4, 3), np.float32); o = np.zeros(4, np.float32); st = np.zeros(4, np.uint32)
    P = lambda x: C.c_void_p(x.ctypes.data) if x is not None else None    # noqa: E731 (host pointers: never launched)

    def fwd(rif_=rif, field=rif, res=(8, 8, 8), n=4, pos=a, xt=a, tau=o, steps=st, h=1.0, ds=0.5):
        return lib.drrt_trace_field_f32(P(rif_), P(field), rif.size, (C.c_int * 3)(*res), n, P(pos), P(a), h, ds, P(xt), P(a),
                                        P(tau), P(steps), None, None, 0, 0, None)

    def back(rif_=rif, field=rif, res=(8, 8, 8), n=4, pos=a, xt=a, steps=st, dx=a, dtau=o, grad=None, gfield=None, dpos=a,
             dvel=a, h=1.0, ds=0.5):
        return lib.drrt_backtrace_field_f32(P(rif_), P(field), rif.size, (C.c_int * 3)(*res), n, P(pos), P(a), P(xt), P(a),
                                            P(steps), P(dx), P(a), P(dtau), h, ds, P(grad), P(gfield), P(dpos), P(dvel), None,
                                            None, 0, 0, None)
    for call, kw, rc, msg in (
            (fwd, dict(rif_=None), _lib.ERR_ARG, "null rif"), (fwd, dict(res=(8, 8, 7)), _lib.ERR_RES_MISMATCH, "Resolution"),
            (fwd, dict(field=None), _lib.ERR_ARG, "null field"),
            (fwd, dict(pos=None), _lib.ERR_ARG, "null ray"), (fwd, dict(xt=None), _lib.ERR_ARG, "null ray"),
            (fwd, dict(tau=None), _lib.ERR_ARG, "null ray"), (fwd, dict(steps=None), _lib.ERR_ARG, "steps_out"),
            (fwd, dict(n=1 << 33), _lib.ERR_ARG, "uint32"), (fwd, dict(ds=0.0), _lib.ERR_ARG, "positive"),
            (fwd, dict(h=float("nan")), _lib.ERR_ARG, "positive"), (fwd, dict(ds=float("inf")), _lib.ERR_ARG, "positive"),
            (back, dict(rif_=None), _lib.ERR_ARG, "null rif"), (back, dict(res=(1, 8, 64)), _lib.ERR_BAD_RES, "invalid resolution"),
            (back, dict(field=None), _lib.ERR_ARG, "null field"),
            (back, dict(pos=None), _lib.ERR_ARG, "null ray"), (back, dict(xt=None), _lib.ERR_ARG, "null ray"),
            (back, dict(steps=None), _lib.ERR_ARG, "fwd_steps"), (back, dict(dpos=None, dvel=None), _lib.ERR_ARG, "null output"),
            (back, dict(dpos=None), _lib.ERR_ARG, "together"), (back, dict(dvel=None), _lib.ERR_ARG, "together"),
            (back, dict(dpos=None, grad=rif), _lib.ERR_ARG, "together"), (back, dict(dvel=None, gfield=rif), _lib.ERR_ARG, "together"),
            (back, dict(n=1 << 33), _lib.ERR_ARG, "uint32"), (back, dict(ds=-1.0), _lib.ERR_ARG, "positive"),
            (back, dict(h=0.0), _lib.ERR_ARG, "positive"), (back, dict(h=float("nan")), _lib.ERR_ARG, "positive")):
        assert call(**kw) == rc, kw
        assert msg in _lib.last_error(), (kw, _lib.last_error())
    # a valid call clears the message (no state left behind); null seeds are not an error
    assert fwd(n=0) == 0 and _lib.last_error() == ""
    assert back(ds=0.0) == _lib.ERR_ARG and _lib.last_error() != ""
    assert back(n=0, dx=None, dtau=None, pos=None) == 0 and _lib.last_error() == ""


def test_routines_under_sanitizers(tmp_path):
    """tests/hostcheck/integral_rays.hip as a stand-alone program (its own main), compiled for the host with ASan + UBSan and
    run as a child process, nothing preloaded: scene 1 plus rays, seeds and field values with NaN, Inf, huge and denormal
    entries."""
    exe = HC.sanitized_program(tmp_path, OH.SOURCE, "FIELD_MAIN")
    s = scene(list(SCENES)[1])
    rng = np.random.default_rng(0)
    bad = np.array([np.nan, np.inf, -np.inf, 3e38, -3e38, 1e30, 1e-40, 0.0], np.float32)
    arrs = {}
    for key in ("pos", "vel", "dx", "dv"):
        extra = s[key][rng.integers(0, len(s[key]), 96)].copy()
        extra[rng.integers(0, 96, 60), rng.integers(0, 3, 60)] = rng.choice(bad, 60)
        arrs[key] = np.concatenate([s[key], extra])
    dtau = np.concatenate([s["dtau"], rng.choice(bad, 96)])
    fld = s["field"].copy().reshape(-1)
    fld[rng.integers(0, fld.size, 40)] = rng.choice(bad, 40)
    n = len(dtau)
    path = str(tmp_path / "case.bin")
    HC.write_case(path, list(s["res"]) + [n], [s["h"], s["ds"]],
                  [s["rif"], fld] + [arrs[key] for key in ("pos", "vel", "dx", "dv")] + [dtau])
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "finished without reports" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
    assert f"{n} rays" in r.stdout


# ---- GPU tier -------------------------------------------------------------------------------------------------------
_same = IC._same


def _gpu_forward(T, s, dev):
    from adjointnonlinearraytracing_amd import drrt
    xt, vt, tau, steps = T.trace_field(_t(s["rif"], dev), _t(s["field"], dev), s["res"], _t(s["pos"], dev), _t(s["vel"], dev),
                                       s["h"], s["ds"])
    return xt, vt, tau, steps, drrt.read_stats(), drrt.keep_order(drrt.last_order)


def _gpu_back(T, s, dev, fw, order=None, dx="dx", dv="dv", dtau="dtau", **kw):
    from adjointnonlinearraytracing_amd import drrt
    xt, vt, _, steps = fw[:4]
    seed = lambda k: None if k is None else _t(s[k], dev)      # noqa: E731
    out = T.backtrace_field(_t(s["rif"], dev), _t(s["field"], dev), s["res"], _t(s["pos"], dev), _t(s["vel"], dev), xt, vt,
                            steps, seed(dx), seed(dv), seed(dtau), s["h"], s["ds"], order=order, **kw)
    return out, drrt.read_stats()


_hosts = {}


def host(name):
    if name not in _hosts:
        s = scene(name)
        k = OH.trace_field(s["rif"], s["field"], s["res"], s["pos"], s["vel"], s["h"], s["ds"])
        _hosts[name] = (k, host_back(s, k, s["dx"], s["dv"], s["dtau"], corrected_h=True))
    return _hosts[name]


def _grids_close(grad, gfield, r, tol=ATOMIC_TOL):
    return cases.rel_l2(grad.cpu().numpy(), r["grad"]) <= tol and cases.rel_l2(gfield.cpu().numpy(), r["grad_field"]) <= tol


@pytest.mark.gpu
@pytest.mark.parametrize("pair", [False, True])
@pytest.mark.parametrize("name", list(SCENES))
def test_kernels_match_host_build(gpu, name, pair):
    """k_trace_field and k_backtrace_field (plain and pair-copy gathers of rif, in the forward's visit order) == the host
    build: rays and statistics bit for bit, both grid gradients to the order of their atomic sums.  xt, vt, steps are also
    TracerC.trace's."""
    from adjointnonlinearraytracing_amd import drrt
    s = scene(name)
    k, r = host(name)
    T = drrt.TracerC()
    with drrt.using(pair_grid=pair, corrected_h=True):
        fw = _gpu_forward(T, s, gpu)
        xt, vt, tau, steps, st, order = fw
        assert order is not None
        assert _same(xt, k["xt"]) and _same(vt, k["vt"]) and _same(tau, k["tau"])
        assert np.array_equal(steps.cpu().numpy().astype(np.int64), k["steps"].astype(np.int64))
        assert st["n_failed"] == k["n_failed"] > 0 and st["ray_steps"] == int(k["steps"].astype(np.int64).sum())
        (grad, gfield, dpos, dvel), bst = _gpu_back(T, s, gpu, fw, order=order)
        xt0, vt0 = T.trace(_t(s["rif"], gpu), s["res"], _t(s["pos"], gpu), _t(s["vel"], gpu), s["h"], s["ds"])
        steps0 = drrt.keep_steps(drrt.last_steps)
    assert torch.equal(xt0, xt) and torch.equal(vt0, vt) and torch.equal(steps0, steps)
    assert _same(dpos, r["dpos"]) and _same(dvel, r["dvel"])
    assert bst["ray_steps"] == r["ray_steps"] and bst["n_failed"] == r["n_failed"] > 0
    err, ferr = cases.rel_l2(grad.cpu().numpy(), r["grad"]), cases.rel_l2(gfield.cpu().numpy(), r["grad_field"])
    print(f"{name} pair={pair}: dL/drif rel-L2 vs host {err:.3e}; dL/dfield {ferr:.3e}")
    assert err <= ATOMIC_TOL and ferr <= ATOMIC_TOL


@pytest.mark.gpu
def test_kernel_variants(gpu):
    """The adjoint with its own sort, in caller order, accumulating into pre-filled grids (DRRT_FLAG_NO_ZERO: both, and each
    alone with the other zeroed by the wrapper), with each grid switched off, without the ray outputs, and with null seeds:
    what remains is unchanged bit for bit (rays) or to the order of the sums (grids)."""
    from adjointnonlinearraytracing_amd import drrt
    name = "box7x11x5_h05_multi"
    s = scene(name)
    k, r = host(name)
    T = drrt.TracerC()
    rays_ok = lambda dpos, dvel, ref=r: _same(dpos, ref["dpos"]) and _same(dvel, ref["dvel"])      # noqa: E731
    with drrt.using(corrected_h=True, pair_grid=False):
        fw = _gpu_forward(T, s, gpu)
        (grad, gfield, dpos, dvel), st = _gpu_back(T, s, gpu, fw)                          # sorts for itself
        assert rays_ok(dpos, dvel) and _grids_close(grad, gfield, r)
        assert st["ray_steps"] == r["ray_steps"] and st["n_failed"] == r["n_failed"]
        with drrt.using(sort_rays=False):
            (grad, gfield, dpos, dvel), st = _gpu_back(T, s, gpu, fw)                      # caller order
        assert rays_ok(dpos, dvel) and _grids_close(grad, gfield, r)
        nv = s["rif"].size
        fill, ffill = torch.full((nv,), 3.0, device=gpu), torch.full((nv,), -2.0, device=gpu)
        (grad, gfield, dpos, dvel), _ = _gpu_back(T, s, gpu, fw, order=fw[5], into=fill, field_into=ffill)
        assert grad.data_ptr() == fill.data_ptr() and gfield.data_ptr() == ffill.data_ptr() and rays_ok(dpos, dvel)
        assert cases.rel_l2(fill.cpu().numpy().astype(np.float64) - 3.0, r["grad"]) <= ATOMIC_TOL
        assert cases.rel_l2(ffill.cpu().numpy().astype(np.float64) + 2.0, r["grad_field"]) <= ATOMIC_TOL
        fill = torch.full((nv,), 3.0, device=gpu)
        (grad, gfield, dpos, dvel), _ = _gpu_back(T, s, gpu, fw, order=fw[5], into=fill)   # the other grid: zeroed by the wrapper
        assert grad.data_ptr() == fill.data_ptr() and rays_ok(dpos, dvel)
        assert cases.rel_l2(fill.cpu().numpy().astype(np.float64) - 3.0, r["grad"]) <= ATOMIC_TOL
        assert cases.rel_l2(gfield.cpu().numpy(), r["grad_field"]) <= ATOMIC_TOL
        ffill = torch.full((nv,), -2.0, device=gpu)
        (grad, gfield, dpos, dvel), _ = _gpu_back(T, s, gpu, fw, order=fw[5], field_into=ffill)
        assert gfield.data_ptr() == ffill.data_ptr() and cases.rel_l2(grad.cpu().numpy(), r["grad"]) <= ATOMIC_TOL
        assert cases.rel_l2(ffill.cpu().numpy().astype(np.float64) + 2.0, r["grad_field"]) <= ATOMIC_TOL
        (grad, gfield, dpos, dvel), st = _gpu_back(T, s, gpu, fw, order=fw[5], grid=False)
        assert grad is None and rays_ok(dpos, dvel) and cases.rel_l2(gfield.cpu().numpy(), r["grad_field"]) <= ATOMIC_TOL
        assert st["ray_steps"] == r["ray_steps"]
        (grad, gfield, dpos, dvel), st = _gpu_back(T, s, gpu, fw, order=fw[5], field_grid=False)
        assert gfield is None and rays_ok(dpos, dvel) and cases.rel_l2(grad.cpu().numpy(), r["grad"]) <= ATOMIC_TOL
        (grad, gfield, dpos, dvel), st = _gpu_back(T, s, gpu, fw, order=fw[5], grid=False, field_grid=False)
        assert grad is None and gfield is None and rays_ok(dpos, dvel) and st["ray_steps"] == r["ray_steps"]
        (grad, gfield, dpos, dvel), st = _gpu_back(T, s, gpu, fw, order=fw[5], rays=False)
        assert dpos is None and dvel is None and _grids_close(grad, gfield, r)
        assert st["ray_steps"] == r["ray_steps"] and st["n_failed"] == r["n_failed"]
        with pytest.raises(RuntimeError, match="nothing to compute"):
            _gpu_back(T, s, gpu, fw, grid=False, field_grid=False, rays=False)
        # null seeds on the rays == zero seeds
        r0 = host_back(s, k, None, None, s["dtau"], corrected_h=True)
        (grad, gfield, dpos, dvel), _ = _gpu_back(T, s, gpu, fw, order=fw[5], dx=None, dv=None)
        assert rays_ok(dpos, dvel, r0) and _grids_close(grad, gfield, r0)
        assert not np.array_equal(r0["dpos"], r["dpos"])
        # a null seed on tau == a zero seed: nothing reaches the field's gradient
        r1 = host_back(s, k, s["dx"], s["dv"], None, corrected_h=True)
        (grad, gfield, dpos, dvel), _ = _gpu_back(T, s, gpu, fw, order=fw[5], dtau=None)
        assert rays_ok(dpos, dvel, r1) and cases.rel_l2(grad.cpu().numpy(), r1["grad"]) <= ATOMIC_TOL
        assert not r1["grad_field"].any() and not bool(gfield.any())
    # flag off
    roff = host_back(s, k, s["dx"], s["dv"], s["dtau"], corrected_h=False)
    with drrt.using(corrected_h=False, pair_grid=False):
        (grad, gfield, dpos, dvel), _ = _gpu_back(T, s, gpu, fw, order=fw[5])
    assert rays_ok(dpos, dvel) and _grids_close(grad, gfield, roff)
    assert cases.rel_l2(roff["grad"], r["grad"]) > 0.1 and np.array_equal(roff["grad_field"], r["grad_field"])


@pytest.mark.gpu
def test_single_ray_and_no_rays(gpu):
    from adjointnonlinearraytracing_amd import drrt
    name = "lens16_h1_half"
    s = scene(name)
    k, _ = host(name)
    i = int(np.where((s["labels"] == "inside") & (k["steps"] > 4) & (k["steps"] < 100))[0][0])
    T = drrt.TracerC()
    for sl in (slice(i, i + 1), slice(0, 0)):
        one = dict(s, **{key: s[key][sl] for key in ("pos", "vel", "dx", "dv", "dtau")})
        with drrt.using(corrected_h=True):
            fw = _gpu_forward(T, one, gpu)
            (grad, gfield, dpos, dvel), st = _gpu_back(T, one, gpu, fw)
        k1 = OH.trace_field(one["rif"], one["field"], one["res"], one["pos"], one["vel"], one["h"], one["ds"])
        r1 = host_back(one, k1, one["dx"], one["dv"], one["dtau"], corrected_h=True)
        assert _same(fw[0], k1["xt"]) and _same(fw[1], k1["vt"]) and _same(fw[2], k1["tau"])
        assert np.array_equal(fw[3].cpu().numpy().astype(np.int64), k1["steps"].astype(np.int64))
        assert _same(dpos, r1["dpos"]) and _same(dvel, r1["dvel"]) and tuple(dpos.shape) == (sl.stop - sl.start, 3)
        assert st["ray_steps"] == r1["ray_steps"] and st["n_failed"] == 0
        if sl.stop > sl.start:
            assert r1["ray_steps"] > 4 and _grids_close(grad, gfield, r1, tol=1e-6)      # one lane: the host's order
        else:
            assert not bool(grad.any()) and not bool(gfield.any()) and grad.numel() == gfield.numel() == s["rif"].size


def _ad_grads(s, dev, seeds, rif_grad=True, field_grad=True, x_grad=True, v_grad=True, dtype=torch.float32, field=None):
    """FieldIntegralTracerC.apply -> L = <dx, xt> + <dv, vt> + <dtau, tau> -> backward
    -> (rif.grad, field.grad, x.grad, v.grad, outputs)."""
    from adjointnonlinearraytracing_amd import tracer
    rif = _t(s["rif"], dev).requires_grad_(rif_grad)
    fld = _t(s["field"] if field is None else field, dev).requires_grad_(field_grad)
    x = _t(s["pos"], dev).to(dtype).requires_grad_(x_grad)
    v = _t(s["vel"], dev).requires_grad_(v_grad)
    out = tracer.FieldIntegralTracerC.apply(rif, fld, x, v, s["h"], s["ds"])
    loss = sum((o * _t(np.asarray(w, np.float32), dev)).sum() for o, w in zip(out, seeds) if w is not None)
    if loss.requires_grad:
        loss.backward()
    torch.cuda.synchronize()
    return rif.grad, fld.grad, x.grad, v.grad, [o.detach() for o in out]


@pytest.mark.gpu
def test_field_tracer_end_to_end(gpu, oracle):
    """FieldIntegralTracerC.apply -> loss on all three outputs -> backward against float64 autograd on the tie-free rays
    (the seeds of the others zeroed on both sides); the bounds of the CPU tier."""
    from adjointnonlinearraytracing_amd import drrt
    import itertools
    s = plane_case()
    k, tie_free, tau64, _ = reference(oracle, s, "plane12")
    assert tie_free.sum() >= 120
    seeds = (s["dx"] * tie_free[:, None], s["dv"] * tie_free[:, None], s["dtau"] * tie_free)
    gr, gf, gp, gv = autograd64(s, *seeds, key=("plane12", True))
    N = lambda t: t.cpu().numpy()      # noqa: E731
    with drrt.using(corrected_h=True):
        grif, gfld, gx, gvel, out = _ad_grads(s, gpu, seeds)
        assert _same(out[0], k["xt"]) and _same(out[1], k["vt"]) and _same(out[2], k["tau"])
        err = rel_err(N(gx), N(gvel), gp, gv)[tie_free]
        gerr, ferr = cases.rel_l2(N(grif), gr), cases.rel_l2(N(gfld), gf)
        terr = (np.abs(k["tau"] - tau64) / tau64)[tie_free].max()
        print(f"FieldIntegralTracerC: {tie_free.sum()} tie-free rays; tau rel err {terr:.3e}; ray grad rel err max "
              f"{err.max():.3e}; dL/drif rel-L2 {gerr:.3e}; dL/dfield rel-L2 {ferr:.3e}")
        assert tuple(grif.shape) == tuple(gfld.shape) == s["rif"].shape
        assert terr <= TAU_TOL and err.max() <= GRAD_TOL and gerr <= GRID_TOL and ferr <= FIELD_TOL
        # a loss on tau alone (the other two outputs unused: their seeds reach the library as null pointers)
        gr1, gf1, gp1, gv1 = autograd64(s, 0 * seeds[0], 0 * seeds[1], seeds[2], key=("plane12", False))
        grif, gfld, gx, gvel, _ = _ad_grads(s, gpu, (None, None, seeds[2]))
        assert rel_err(N(gx), N(gvel), gp1, gv1)[tie_free].max() <= GRAD_TOL
        assert cases.rel_l2(N(grif), gr1) <= GRID_TOL and cases.rel_l2(N(gfld), gf1) <= FIELD_TOL
        # only what is asked for comes back: every combination of requires_grad
        for want in itertools.product((False, True), repeat=4):
            got = _ad_grads(s, gpu, seeds, *want)[:4]
            assert tuple(g is not None for g in got) == want, want
        with pytest.raises(RuntimeError, match="float32"):
            _ad_grads(s, gpu, seeds, True, True, True, False, dtype=torch.float64)
        with pytest.raises(RuntimeError, match="shape"):
            _ad_grads(s, gpu, seeds, field=s["field"][:, :, :-1])
        with pytest.raises(RuntimeError, match="shape"):
            _ad_grads(s, gpu, seeds, field=s["field"].reshape(16, 8, 32))
    # h = 0.5 (the same rays scaled by a power of two: every fp32 result scales exactly, so the same errors): the options of
    # the forward's thread reach the backward launch, which autograd runs on a thread of its own
    s2 = plane_case(h=0.5)
    assert np.array_equal(s2["pos"], s["pos"] * np.float32(0.5))
    gr2, gf2 = autograd64(s2, *seeds)[:2]
    with drrt.using(corrected_h=True):
        on = _ad_grads(s2, gpu, seeds)
    with drrt.using(corrected_h=False):
        off = _ad_grads(s2, gpu, seeds)
    assert cases.rel_l2(N(on[0]), gr2) <= GRID_TOL and cases.rel_l2(N(off[0]), gr2) > 0.1
    assert cases.rel_l2(N(on[1]), gf2) <= FIELD_TOL and cases.rel_l2(N(off[1]), gf2) <= FIELD_TOL


@pytest.mark.gpu
def test_field_tracer_launches(gpu):
    """Forward: ["trace_field"].  Backward: ONE backtrace_field launch behind one zero-fill per grid gradient asked for;
    none when nothing requires grad.  (The sort belongs to the forward when options.sort_rays is on: the adjoint takes its
    order.)"""
    from adjointnonlinearraytracing_amd import _lib, drrt
    s = plane_case()
    seeds = (s["dx"], s["dv"], s["dtau"])
    lib = _lib.load()

    def launches(**kw):
        lib.drrt_profile_begin(256)
        try:
            _ad_grads(s, gpu, seeds, **kw)
            return [name for name, _ in _lib.profile_collect()]
        finally:
            lib.drrt_profile_end()
    none = dict(rif_grad=False, field_grad=False, x_grad=False, v_grad=False)
    for sort, fwd in ((False, ["trace_field"]), (True, ["sort", "trace_field"])):
        with drrt.using(sort_rays=sort, pair_grid=False):
            assert launches(**none) == fwd
            assert launches() == fwd + ["zero", "zero", "backtrace_field"]
            assert launches(x_grad=False, v_grad=False) == fwd + ["zero", "zero", "backtrace_field"]
            assert launches(**dict(none, rif_grad=True)) == fwd + ["zero", "backtrace_field"]
            assert launches(**dict(none, field_grad=True)) == fwd + ["zero", "backtrace_field"]
            assert launches(field_grad=False) == fwd + ["zero", "backtrace_field"]
            assert launches(rif_grad=False, field_grad=False) == fwd + ["backtrace_field"]
            assert launches(**dict(none, v_grad=True)) == fwd + ["backtrace_field"]


@pytest.mark.gpu
def test_demo(gpu):
    """examples/absorption_demo.py at 17^3, 3 views of 24^2 rays, 20 iterations: the loss is finite and ends below where it
    began."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    try:
        import absorption_demo
    finally:
        sys.path.pop(0)
    _, _, hist, err = absorption_demo.run(res=17, views=3, side=24, iters=20, verbose=False)
    print(f"absorption_demo: loss {hist[0]:.4e} -> {hist[-1]:.4e} (ratio {hist[-1] / hist[0]:.4f}); rms(a - truth) "
          f"{err[0]:.3e} -> {err[-1]:.3e}")
    assert len(hist) == 20 and np.isfinite(hist).all() and hist[-1] < hist[0]
