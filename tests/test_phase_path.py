"""Ray paths with velocities: drrt_trace_phase_f32 / drrt_backtrace_phase_f32, TracerC.trace_phase / backtrace_phase,
tracer.PhasePathTracerC.

CPU tier: the host build of the product's per-ray routines (tests/hostcheck/integral_rays.hip: trace_phase_ray and
phase_backtrace_ray of csrc/drrt_device.h) against the host build of the path routines (their forwards without the velocity
series; bit for bit), against float64 torch.autograd through tests/integral_ad (its one loop, recording (x, v) where the
product does) on the compared rays, against closed forms, and the C ABI's argument checks.  GPU tier:
k_trace_phase / k_backtrace_phase of drrt_integral.hip against that host build, the autograd class end to end, its
launches, and the demo.

The referee (path_common.referee_phase, shared with tests/test_phase_path_fuzz.py): L = <dx, xt> + <dv, vt> + <dpath, path> +
<dvpath, vpath> in float64, and once more in float32 as the yardstick.  Compared rays, bound and caps are test_path.py's
(integral_fuzz_common.bound, FLOOR, MARGIN, CAPS unchanged); a vpath sample's error is the largest absolute difference over
the compared rays and j < M over the largest |v| of the float64 run and stays under CAPS["out"], like a path sample's over
the box's longest edge.  Modes: every seed; no seeds on the rays; dvpath on the prefix samples alone, on the in-box samples
alone, on the padded entries alone; dpath and dvpath together on the in-box samples (the last five without ray seeds).

On the parent commit every test here fails: the host build of the routines does not compile (no trace_phase_ray), the
library has no such C symbols, TracerC no such methods, tracer no such class and examples/ no such demo.

Largest e_prod / max(e_ref, 2.4e-7) on the fixed scenes, host build (8 allowed): ray gradients 4.77 (box7x11x5_h1_half,
stride 1, truncating M, dvpath on the prefix samples alone: 1.27e-6 against 2.65e-7), dL/drif 2.11 (box7x11x5_h05_multi,
stride 1), path samples 1.16, vpath samples 1.32 (lens16_h05_half, stride 1).

Mutation checks (tried by hand on csrc/drrt_device.h, one at a time, each then undone; CPU tier of this file and of
tests/test_phase_path_fuzz.py, 117 tests):
  * the in-box velocity seed added in `pull` (behind the sample) instead of `enter`: 83 fail -- all 20 cases of
    test_referee_on_fixed_scenes, 62 of the 64 of test_phase_path_fuzz.py::test_referee, test_uniform_medium_closed_form;
  * its countdown started one iteration early (the seed on v_k lands in the iteration that arrives at x_k): 91 fail -- the 84
    referee cases, all five of test_adjoint_identities, test_uniform_medium_closed_form,
    test_exit_on_first_iteration_closed_form;
  * the padded velocity seeds dropped: 92 fail -- those 91 and test_never_entering_ray_closed_form."""
import ctypes as C
import inspect
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
from integral_common import ATOMIC_TOL, _same, scene
from integral_fuzz_common import CAPS
import integral_host as OH
from oracle import torch_ad
import path_common as PC
from path_common import STRIDES, _bits, back_phase as back, count_of, dpath_of, dvpath_of, fwd_phase as fwd, pad_m, trunc_m
from raygrad_common import SCENES, TIE_TOL, _t, max_steps_fwd, rel_err


# ---- the compared rays (as tests/test_path.py) ------------------------------------------------------------------------
def tie_free_for_yardstick(c):
    """The rays whose float32 and float64 torch runs leave on the same iteration with exit samples within TIE_TOL
    (tests/integral_fuzz_common.py::masks)."""
    T = lambda a, dt: torch.tensor(np.asarray(a), dtype=dt)      # noqa: E731
    with torch.no_grad():
        lo, hi = (integral_ad.trace_opl(T(c["rif"], dt), T(c["pos"], dt), T(c["vel"], dt), c["h"], c["ds"])
                  for dt in (torch.float32, torch.float64))
    ms_ad = int(4 * c["h"] * max(c["rif"].shape) / c["ds"])
    close = lambda a, b: (a.double() - b).abs().max(1).values <= TIE_TOL      # noqa: E731
    return ((lo[3] < ms_ad) & (lo[3] == hi[3]) & close(lo[0], hi[0]) & close(lo[1], hi[1])).numpy()


_compared = {}


def compared_rays(oracle, name):
    if name not in _compared:
        s = scene(name)
        _compared[name] = IC.reference(oracle, s, name)[1] & tie_free_for_yardstick(s)
    return _compared[name]


def _fp32_sum(start, rows):
    """((start + rows[0]) + rows[1]) + ... in fp32."""
    out = start.copy()
    for r in rows:
        out = (out + r).astype(np.float32)
    return out


# ---- CPU tier -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SCENES))
def test_forward_identities(name):
    """(xt, vt, path, count, steps) == trace_path's; vpath[0] == vel; every padded vpath entry == vt; the stride-s vpath ==
    every s-th row of the stride-1 vpath (s = 1, 2, 7 and one above every K); M = 3 leaves the first three rows unchanged:
    all bit for bit.  At stride 1, path[j+1] == path[j] + ds vpath[j+1] evaluated in float64 to within one fp32 ulp for
    j + 1 < count: x_k is paired with v_k."""
    s = scene(name)
    ms = max_steps_fwd(s["res"], s["h"], s["ds"])
    one = fwd(s, 1, pad_m(ms, 1))
    K = one["steps"].astype(np.int64)
    assert K.max() == ms and (K < ms).sum() > 300
    for stride in (1, 2, 7, ms + 3):
        M = pad_m(ms, stride)
        k = one if stride == 1 else fwd(s, stride, M)
        p = PC.fwd(s, stride, M)
        for key in ("xt", "vt", "path"):
            assert np.array_equal(_bits(k[key]), _bits(p[key])), key
        assert np.array_equal(k["count"], p["count"]) and np.array_equal(k["steps"], p["steps"])
        assert k["n_failed"] == p["n_failed"] > 0
        assert np.array_equal(_bits(k["vpath"][0]), _bits(s["vel"]))
        cnt = count_of(k["steps"], stride, M)
        padded = np.arange(M)[:, None] >= cnt[None, :]
        assert padded[-1].all()
        assert np.array_equal(_bits(k["vpath"])[padded], _bits(np.broadcast_to(k["vt"], k["vpath"].shape))[padded])
        rows = one["vpath"][::stride][:M]
        sample = ~padded[:len(rows)]
        assert np.array_equal(_bits(k["vpath"][:len(rows)])[sample], _bits(rows)[sample])
        if stride > ms:
            assert (cnt == 1).all()
        cut = fwd(s, stride, 3)
        if M >= 3:
            assert np.array_equal(_bits(cut["vpath"]), _bits(k["vpath"][:3])) and np.array_equal(_bits(cut["path"]), _bits(k["path"][:3]))
        assert np.array_equal(cut["count"], np.minimum(cnt, 3)) and np.array_equal(_bits(cut["vt"]), _bits(k["vt"]))
    # the pairing: x_{j+1} = fmaf(ds, v_{j+1}, x_j), one rounding of the float64 value
    M = pad_m(ms, 1)
    live = (np.arange(1, M)[:, None] < one["count"][None, :])
    x64 = one["path"][:-1].astype(np.float64) + np.float64(np.float32(s["ds"])) * one["vpath"][1:].astype(np.float64)
    got = one["path"][1:].astype(np.float64)
    ulp = np.spacing(np.abs(x64).astype(np.float32)).astype(np.float64)
    assert live.sum() > 1000 and (np.abs(got - x64)[live] <= ulp[live]).all()
    # ... and with the velocity of the OTHER end of the step it is not (the medium bends these rays)
    y64 = one["path"][:-1].astype(np.float64) + np.float64(np.float32(s["ds"])) * one["vpath"][:-1].astype(np.float64)
    assert (np.abs(got - y64)[live] > ulp[live]).any()


@pytest.mark.parametrize("name", list(SCENES))
def test_adjoint_identities(name):
    """dvpath null or zeros: backtrace_path's results, bit for bit on the rays, equal on the grid.  Seeds on padded vpath
    entries alone: backtrace_path's with dv plus their ascending fp32 sum.  Seeds on prefix vpath entries alone: dpos and the
    grid unchanged, dvel plus their ascending fp32 sum."""
    s = scene(name)
    ms = max_steps_fwd(s["res"], s["h"], s["ds"])
    n = len(s["pos"])
    for stride in (1, 7):
        M = pad_m(ms, stride)
        k = fwd(s, stride, M)
        g = dpath_of((M, n, 3), stride)
        ref = PC.back(s, k, s["dx"], s["dv"], g, stride, M, corrected_h=True)
        for dvpath in (None, np.zeros((M, n, 3), np.float32)):
            r = back(s, k, s["dx"], s["dv"], g, dvpath, stride, M, corrected_h=True)
            assert np.array_equal(_bits(r["dpos"]), _bits(ref["dpos"])) and np.array_equal(_bits(r["dvel"]), _bits(ref["dvel"]))
            assert np.array_equal(r["grad"], ref["grad"]) and np.array_equal(r["steps"], ref["steps"])
            assert np.array_equal(r["failed"], ref["failed"]) and r["n_failed"] > 0
        pre, box, pad = PC.classes(k, ref, stride, M)
        gv = dvpath_of((M, n, 3), stride)
        # padded entries alone
        dvpath = gv * pad[:, :, None]
        dv = _fp32_sum(s["dv"], dvpath)
        assert pad.sum(0).max() >= 3 and not np.array_equal(dv, s["dv"])
        r = back(s, k, s["dx"], s["dv"], g, dvpath, stride, M, corrected_h=True)
        want = PC.back(s, k, s["dx"], dv, g, stride, M, corrected_h=True)
        assert np.array_equal(_bits(r["dpos"]), _bits(want["dpos"])) and np.array_equal(_bits(r["dvel"]), _bits(want["dvel"]))
        assert np.array_equal(r["grad"], want["grad"])
        # prefix entries alone (a failed ray has no sample: the host adjoint's e is meaningless there, and nothing is read)
        dvpath = gv * (pre & ~ref["failed"][None, :])[:, :, None]
        r = back(s, k, s["dx"], s["dv"], g, dvpath, stride, M, corrected_h=True)
        assert np.array_equal(_bits(r["dpos"]), _bits(ref["dpos"])) and np.array_equal(r["grad"], ref["grad"])
        assert np.array_equal(_bits(r["dvel"]), _bits(_fp32_sum(ref["dvel"], dvpath)))
        assert not np.array_equal(r["dvel"], ref["dvel"])


@pytest.mark.parametrize("kind", ["pad", "trunc"])
@pytest.mark.parametrize("stride", STRIDES)
@pytest.mark.parametrize("name", list(SCENES))
def test_referee_on_fixed_scenes(oracle, name, stride, kind):
    """Forward and adjoint against float64 autograd of L = <dx, xt> + <dv, vt> + <dpath, path> + <dvpath, vpath>, every
    mode."""
    s = scene(name)
    ms = max_steps_fwd(s["res"], s["h"], s["ds"])
    cmp_ = compared_rays(oracle, name)
    assert cmp_.sum() >= 400
    M = pad_m(ms, stride) if kind == "pad" else trunc_m(ms, stride)
    worst, bad, weight = PC.referee_phase(s, cmp_, stride, M, f"{name} stride={stride} M={M}")
    assert bad == []
    assert min(weight[m] for m in ("all", "noray", "vprefix", "vinbox", "inbox")) > 100
    assert weight["vpadded"] > (100 if kind == "pad" else 0)


def _uniform():
    res, h, ds, c = (9, 8, 7), 1.0, 0.5, 1.25
    rif = np.full((res[2], res[1], res[0]), c, np.float32)
    pos = np.array([(3.25, -1.25, 3.5), (0.0, 2.5, 1.125), (4.5, 3.5, 2.75), (-2.0, 3.0, 3.0), (7.875, 6.75, 5.5)], np.float32)
    vel = np.array([(0.25, 1.0, 0.125), (1.0, 0.0, 0.0), (-0.5, 0.25, 0.75), (1.0, 0.125, -0.25), (0.125, 0.125, 0.0625)], np.float32)
    return dict(rif=rif, res=res, h=h, ds=ds, pos=pos, vel=vel), c


def test_uniform_medium_closed_form():
    """n = c everywhere: the rays are straight (tests/test_path.py's case; everything dyadic, so the forward is exact).  Every
    vpath row == vel bit for bit.  With g_j / w_j the seeds on path[j] / vpath[j]:
      dpos = dx + sum_j g_j
      dvel = dv + sum_j w_j + K ds (dx + sum_{padded} g_j) + sum_{j < count} (j stride ds) g_j.
    The grid: grad n = 0, so a contribution has no value weights (the grid sums to 0) and its gradient splat has the first
    moment (n ds / h) mu in voxel indices; the moments of all of them are dL/d(eps) for n = c + eps (ix, iy, iz), under which
    v_k moves by (k - e) ds c / h and x_k by ds times the running sum of that, k = e .. K (e: the first in-box sample)."""
    s, c = _uniform()
    res, h, ds, pos, vel = s["res"], s["h"], s["ds"], s["pos"], s["vel"]
    ms = max_steps_fwd(res, h, ds)
    rng = np.random.default_rng(2)
    dyadic = lambda shape: (rng.integers(-8, 9, shape) / 4.0).astype(np.float32)      # noqa: E731
    dx, dv = dyadic(pos.shape), dyadic(pos.shape)
    iz, iy, ix = np.meshgrid(*(np.arange(r, dtype=np.float64) for r in (res[2], res[1], res[0])), indexing="ij")
    for stride in (1, 3):
        M = pad_m(ms, stride)
        k = fwd(s, stride, M)
        K = k["steps"].astype(np.int64)
        assert (K < ms).all() and K.min() >= 2 and K.max() >= 12
        assert np.array_equal(_bits(k["vpath"]), _bits(np.broadcast_to(vel, k["vpath"].shape)))
        idx = np.arange(M)[:, None] * stride
        sample = idx < K[None, :]
        assert np.array_equal(k["count"], sample.sum(0))
        g, w = dyadic(k["path"].shape), dyadic(k["path"].shape)
        r = back(s, k, dx, dv, g, w, stride, M, corrected_h=True)
        g64, w64 = g.astype(np.float64), w.astype(np.float64)
        want_p = dx + g64.sum(0)
        want_v = dv + w64.sum(0) + (K * ds)[:, None] * (dx + (g64 * ~sample[:, :, None]).sum(0)) + \
            (g64 * (sample * idx * ds)[:, :, None]).sum(0)
        np.testing.assert_allclose(r["dpos"], want_p, rtol=1e-6, atol=1e-6)
        np.testing.assert_allclose(r["dvel"], want_v, rtol=1e-6, atol=1e-6)
        # the grid
        e = K - r["steps"].astype(np.int64)
        assert (e < K).all() and (e > 0).any() and (e == 0).any()
        kk = np.where(sample, idx, K[None, :])                                     # the iteration an entry holds the state of
        m = np.clip(kk - e[None, :], 0, None).astype(np.float64)
        dV = m * (ds * c / h)                                                      # d v_k / d eps, per axis
        dX = ds * (ds * c / h) * m * (m + 1) / 2                                   # d x_k / d eps
        mK = (K - e).astype(np.float64)
        want_m = (g64 * dX[:, :, None] + w64 * dV[:, :, None]).sum((0, 1)) + \
            (dx * (ds * (ds * c / h) * mK * (mK + 1) / 2)[:, None] + dv * (mK * ds * c / h)[:, None]).sum(0)
        G = r["grad"].reshape(res[2], res[1], res[0])
        got_m = np.array([(G * ix).sum(), (G * iy).sum(), (G * iz).sum()])
        np.testing.assert_allclose(got_m, want_m, rtol=1e-5, atol=1e-5)
        assert abs(G.sum()) <= 1e-5 * np.abs(G).sum() and np.abs(G).max() > 0.1


def test_exit_on_first_iteration_closed_form():
    """e = 0, K = 1 (tests/test_path.py's case): count = 1, vpath = (vel, vt, vt, ...).  With dx' / dv' = dx / dv + the padded
    seeds of path / vpath: mu = dv' + ds dx', dvel = mu + w_0, dpos = dx' + ds J(x0)^T mu + g_0, J = d(n grad n)/dx at x0."""
    rif = cases.luneburg(16)
    h, ds, res = 1.0, 0.5, (16, 16, 16)
    pos = np.array([[14.8, 7.3, 6.1]], np.float32)
    vel = np.array([[1.0, 0.1, -0.05]], np.float32)
    s = dict(rif=rif, res=res, h=h, ds=ds, pos=pos, vel=vel)
    k = fwd(s, 1, 4)
    assert k["steps"][0] == 1 and k["count"][0] == 1
    assert np.array_equal(_bits(k["vpath"][:, 0]), _bits(np.stack([vel[0], k["vt"][0], k["vt"][0], k["vt"][0]])))
    assert not np.array_equal(k["vt"][0], vel[0])
    dx = np.array([[0.3, -1.2, 0.7]], np.float32); dv = np.array([[-0.4, 0.9, 0.2]], np.float32)
    g = np.array([[[1.1, -0.6, 0.4]], [[0.2, 0.5, -0.9]], [[-0.3, 0.8, 0.1]], [[0.9, -0.2, 0.7]]], np.float32)
    w = np.array([[[0.6, 0.3, -1.1]], [[-0.7, 0.4, 0.2]], [[0.5, -0.9, 0.8]], [[0.1, 1.2, -0.3]]], np.float32)
    r = back(s, k, dx, dv, g, w, 1, 4)
    R = torch.tensor(rif, dtype=torch.float64)
    x = torch.tensor(pos[0], dtype=torch.float64)
    f = lambda y: (lambda nn, gg: (nn[:, None] * gg)[0])(*torch_ad.eval_grad(R, y[None], h, torch.tensor([True])))   # noqa: E731
    J = torch.autograd.functional.jacobian(f, x).numpy()
    dxp = dx[0].astype(np.float64) + g[1:, 0].astype(np.float64).sum(0)
    dvp = dv[0].astype(np.float64) + w[1:, 0].astype(np.float64).sum(0)
    mu = dvp + ds * dxp
    np.testing.assert_allclose(r["dvel"][0], mu + w[0, 0], rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(r["dpos"][0], dxp + ds * J.T @ mu + g[0, 0], rtol=1e-5, atol=1e-6)
    assert r["steps"][0] == 1 and np.abs(r["grad"]).max() > 0


def test_never_entering_ray_closed_form():
    """A ray outside the box that points away: K = 1, and one that flies past it: K > 1, e = K.  (xt, vt) = (pos, vel), so
    every vpath entry is vel.  The gradient is backtrace_path's -- (dx, dv), the padded seeds on dx, the prefix seeds -- with
    every vpath seed on dvel: the padded ones on dv in front (ascending j, fp32), the samples' behind the position seeds of
    the prefix (ascending j), bit for bit; no grid contribution."""
    rif = cases.luneburg(16)
    h, ds, res = 1.0, 0.5, (16, 16, 16)
    pos = np.array([[-1.0, 7.3, 6.1], [-2.0, -1.5, 3.0]], np.float32)
    vel = np.array([[-1.0, 0.1, 0.0], [1.0, 0.0, 0.25]], np.float32)
    s = dict(rif=rif, res=res, h=h, ds=ds, pos=pos, vel=vel)
    rng = np.random.default_rng(8)
    dx, dv = rng.normal(size=(2, 3)).astype(np.float32), rng.normal(size=(2, 3)).astype(np.float32)
    for stride, M in ((1, 6), (4, 9), (4, 3)):
        k = fwd(s, stride, M)
        K = k["steps"].astype(np.int64)
        assert K[0] == 1 and 6 < K[1] < max_steps_fwd(res, h, ds)
        assert np.array_equal(_bits(k["xt"]), _bits(pos)) and np.array_equal(_bits(k["vt"]), _bits(vel))
        assert np.array_equal(_bits(k["vpath"]), _bits(np.broadcast_to(vel, k["vpath"].shape)))
        cnt = count_of(k["steps"], stride, M)
        assert np.array_equal(k["count"], cnt)
        g, w = rng.normal(size=(M, 2, 3)).astype(np.float32), rng.normal(size=(M, 2, 3)).astype(np.float32)
        r = back(s, k, dx, dv, g, w, stride, M)
        for i in range(2):
            dp, dw = dx[i].copy(), dv[i].copy()
            for j in range(cnt[i], M):
                dp = (dp + g[j, i]).astype(np.float32)
                dw = (dw + w[j, i]).astype(np.float32)
            for j in range(cnt[i]):
                dp = (dp + g[j, i]).astype(np.float32)
                kds = np.float32(np.float32(j * stride) * np.float32(ds))
                dw = (kds.astype(np.float64) * g[j, i].astype(np.float64) + dw.astype(np.float64)).astype(np.float32)
            for j in range(cnt[i]):
                dw = (dw + w[j, i]).astype(np.float32)
            assert np.array_equal(_bits(r["dpos"][i]), _bits(dp)) and np.array_equal(_bits(r["dvel"][i]), _bits(dw)), (stride, M, i)
        assert not r["grad"].any() and r["ray_steps"] == 0 and r["n_failed"] == 0


def test_failed_ray():
    """A ray at rest outside the box never leaves: K = max_steps.  Forward: every vpath entry is vel (the stale v0, Q6).
    Adjoint: zeros, counted, no grid contribution, whatever the seeds -- NaN seeds included: none is read."""
    s = scene("lens16_h1_half")
    ms = max_steps_fwd(s["res"], s["h"], s["ds"])
    i = np.where(s["labels"] == "zero")[0][:8]
    one = dict(s, pos=s["pos"][i], vel=s["vel"][i])
    for stride, M in ((1, pad_m(ms, 1)), (7, pad_m(ms, 7)), (ms, 2), (1, 3)):
        k = fwd(one, stride, M)
        assert (k["steps"] == ms).all() and k["n_failed"] == 8 and np.array_equal(k["count"], count_of(k["steps"], stride, M))
        assert np.array_equal(_bits(k["path"]), _bits(np.broadcast_to(one["pos"], k["path"].shape)))
        assert np.array_equal(_bits(k["vpath"]), _bits(np.broadcast_to(one["vel"], k["vpath"].shape)))
        nan = np.full(k["path"].shape, np.nan, np.float32)
        for g, w in ((dpath_of(k["path"].shape, 1), dvpath_of(k["path"].shape, 1)), (nan, nan)):
            r = back(one, k, s["dx"][i], s["dv"][i], g, w, stride, M)
            assert r["n_failed"] == 8 and r["failed"].all() and not r["dpos"].any() and not r["dvel"].any()
            assert not r["grad"].any() and r["ray_steps"] == 0


def test_abi_and_python_surface(monkeypatch):
    """The C symbols are exported and bound, the two profile ids are named, the methods and the class exist with their
    argument order, `samples` is read off dvpath when dpath is None, and the class refuses CPU tensors as the family's
    classes do (no fallback)."""
    from adjointnonlinearraytracing_amd import _lib, drrt, tracer
    lib = C.CDLL(_lib.LIB_PATH)
    for name in ("drrt_trace_phase_f32", "drrt_backtrace_phase_f32"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    assert len(_lib.SIGNATURES["drrt_trace_phase_f32"][1]) == len(_lib.SIGNATURES["drrt_trace_path_f32"][1]) + 1
    assert len(_lib.SIGNATURES["drrt_backtrace_phase_f32"][1]) == len(_lib.SIGNATURES["drrt_backtrace_path_f32"][1]) + 1
    assert _lib.PROF_NAMES_LATER[25] == "trace_phase" and _lib.PROF_NAMES_LATER[26] == "backtrace_phase"
    assert _lib.PROF_NAMES_LATER[24] == "backtrace_path"
    with open(os.path.join(os.path.dirname(_lib.LIB_PATH), "..", "include", "drrt_hip.h")) as f:
        hdr = f.read()
    assert "drrt_trace_phase_f32" in hdr and "drrt_backtrace_phase_f32" in hdr
    assert "#define DRRT_PROF_TRACE_PHASE 25" in hdr and "#define DRRT_PROF_BACKTRACE_PHASE 26" in hdr
    assert issubclass(tracer.PhasePathTracerC, torch.autograd.Function)
    assert list(inspect.signature(drrt.TracerC.trace_phase).parameters) == \
        ["self", "rif", "res", "pos", "vel", "h", "ds", "stride", "samples"]
    assert list(inspect.signature(drrt.TracerC.backtrace_phase).parameters) == \
        ["self", "rif", "res", "pos", "vel", "xt", "vt", "steps", "dx", "dv", "dpath", "dvpath", "h", "ds", "stride", "grid",
         "rays", "into", "order", "samples"]
    assert list(inspect.signature(drrt.TracerC.backtrace_path).parameters) == \
        ["self", "rif", "res", "pos", "vel", "xt", "vt", "steps", "dx", "dv", "dpath", "h", "ds", "stride", "grid", "rays",
         "into", "order", "samples"]
    seen = []
    monkeypatch.setattr(drrt, "_backtrace_integral", lambda op, *a, **kw: seen.append((op, a, kw)))
    z = torch.zeros(1, 3)
    T = drrt.TracerC()
    for dpath, dvpath, samples, want in ((None, torch.zeros(7, 1, 3), None, 7), (torch.zeros(5, 1, 3), None, None, 5),
                                         (torch.zeros(5, 1, 3), torch.zeros(5, 1, 3), None, 5), (None, None, None, 1),
                                         (None, None, 9, 9)):
        T.backtrace_phase(z, (2, 2, 2), z, z, z, z, z, None, None, dpath, dvpath, 1.0, 0.5, 3, samples=samples)
        op, a, kw = seen[-1]
        assert op == "phase" and kw["scalars"] == (3, want)
        assert [t is None for t, _ in kw["series"]] == [dpath is None, dvpath is None]
        assert all(shape == (want, None, 3) for _, shape in kw["series"])
    monkeypatch.undo()
    rif = torch.ones(8, 8, 8, requires_grad=True)
    x, v = torch.zeros(4, 3), torch.ones(4, 3)
    with pytest.raises(RuntimeError, match="cuda"):
        tracer.PhasePathTracerC.apply(rif, x, v, 1.0, 0.5, 1, None)
    with pytest.raises(RuntimeError, match="cuda"):
        drrt.TracerC().trace_phase(rif.detach(), (8, 8, 8), x, v, 1.0, 0.5, 1)


def test_abi_argument_checks():
    """Null vpath, stride < 1, samples < 1, samples n 3 floats overflowing size_t (the extent of either series), null
    pointers, all outputs null, too many rays and bad steps are refused before anything is launched; n = 0 is fine, and so
    are null seeds."""
    from adjointnonlinearraytracing_amd import _lib
    lib = _lib.load()
    rif = np.ones(8 * 8 * 8, np.float32)
    a = np.zeros((4, 3), np.float32); pth = np.zeros((5, 4, 3), np.float32)
    cnt = np.zeros(4, np.int32); st = np.zeros(4, np.uint32)
    P = lambda x: C.c_void_p(x.ctypes.data) if x is not None else None    # noqa: E731 (host pointers: never launched)

    def fw(rif_=rif, res=(8, 8, 8), n=4, pos=a, xt=a, path=pth, vpath=pth, count=cnt, steps=st, h=1.0, ds=0.5, stride=2,
           samples=5):
        return lib.drrt_trace_phase_f32(P(rif_), rif.size, (C.c_int * 3)(*res), n, P(pos), P(a), h, ds, stride, samples, P(xt),
                                        P(a), P(path), P(vpath), P(count), P(steps), None, None, 0, 0, None)

    def bw(rif_=rif, res=(8, 8, 8), n=4, pos=a, xt=a, steps=st, dx=a, dpath=pth, dvpath=pth, grad=None, dpos=a, dvel=a, h=1.0,
           ds=0.5, stride=2, samples=5):
        return lib.drrt_backtrace_phase_f32(P(rif_), rif.size, (C.c_int * 3)(*res), n, P(pos), P(a), P(xt), P(a), P(steps),
                                            P(dx), P(a), P(dpath), P(dvpath), h, ds, stride, samples, P(grad), P(dpos),
                                            P(dvel), None, None, 0, 0, None)
    big = (1 << 32) - 1
    for call, kw, rc, msg in (
            (fw, dict(vpath=None), _lib.ERR_ARG, "null ray"),
            (fw, dict(stride=0), _lib.ERR_ARG, "stride"), (fw, dict(stride=-3), _lib.ERR_ARG, "stride"),
            (fw, dict(samples=0), _lib.ERR_ARG, "samples"), (fw, dict(samples=-1), _lib.ERR_ARG, "samples"),
            (fw, dict(n=big, samples=(1 << 31) - 1), _lib.ERR_ARG, "overflow"),
            (fw, dict(rif_=None), _lib.ERR_ARG, "null rif"), (fw, dict(res=(8, 8, 7)), _lib.ERR_RES_MISMATCH, "Resolution"),
            (fw, dict(pos=None), _lib.ERR_ARG, "null ray"), (fw, dict(xt=None), _lib.ERR_ARG, "null ray"),
            (fw, dict(path=None), _lib.ERR_ARG, "null ray"), (fw, dict(count=None), _lib.ERR_ARG, "null ray"),
            (fw, dict(steps=None), _lib.ERR_ARG, "steps_out"), (fw, dict(n=1 << 33), _lib.ERR_ARG, "uint32"),
            (fw, dict(ds=0.0), _lib.ERR_ARG, "positive"), (fw, dict(h=float("nan")), _lib.ERR_ARG, "positive"),
            (bw, dict(stride=0), _lib.ERR_ARG, "stride"), (bw, dict(samples=0), _lib.ERR_ARG, "samples"),
            (bw, dict(n=big, samples=(1 << 31) - 1), _lib.ERR_ARG, "overflow"),
            (bw, dict(n=big, samples=(1 << 31) - 1, dpath=None), _lib.ERR_ARG, "overflow"),
            (bw, dict(n=big, samples=(1 << 31) - 1, dvpath=None), _lib.ERR_ARG, "overflow"),
            (bw, dict(rif_=None), _lib.ERR_ARG, "null rif"), (bw, dict(res=(1, 8, 64)), _lib.ERR_BAD_RES, "invalid resolution"),
            (bw, dict(pos=None), _lib.ERR_ARG, "null ray"), (bw, dict(xt=None), _lib.ERR_ARG, "null ray"),
            (bw, dict(steps=None), _lib.ERR_ARG, "fwd_steps"), (bw, dict(dpos=None, dvel=None), _lib.ERR_ARG, "null output"),
            (bw, dict(dpos=None), _lib.ERR_ARG, "together"), (bw, dict(dvel=None), _lib.ERR_ARG, "together"),
            (bw, dict(n=1 << 33), _lib.ERR_ARG, "uint32"), (bw, dict(ds=-1.0), _lib.ERR_ARG, "positive"),
            (bw, dict(h=0.0), _lib.ERR_ARG, "positive")):
        assert call(**kw) == rc, kw
        assert msg in _lib.last_error(), (kw, _lib.last_error())
    assert fw(n=0) == 0 and _lib.last_error() == ""
    assert fw(n=0, vpath=None) == 0 and _lib.last_error() == ""
    assert bw(stride=0) == _lib.ERR_ARG and _lib.last_error() != ""
    assert bw(n=0, dx=None, dpath=None, dvpath=None, pos=None) == 0 and _lib.last_error() == ""


def test_routines_under_sanitizers(tmp_path):
    """tests/hostcheck/integral_rays.hip (-DPHASE_MAIN) as a stand-alone program (its own main), compiled for the host with
    ASan + UBSan and run as a child process, nothing preloaded: scene 1 plus rays and seeds with NaN, Inf, huge and denormal entries, with
    a stride above every K, with M = 1, and with zero rays."""
    exe = HC.sanitized_program(tmp_path, OH.SOURCE, "PHASE_MAIN")
    s = scene(list(SCENES)[1])
    ms = max_steps_fwd(s["res"], s["h"], s["ds"])
    rng = np.random.default_rng(0)
    bad = np.array([np.nan, np.inf, -np.inf, 3e38, -3e38, 1e30, 1e-40, 0.0], np.float32)
    arrs = {}
    for key in ("pos", "vel", "dx", "dv"):
        extra = s[key][rng.integers(0, len(s[key]), 96)].copy()
        extra[rng.integers(0, 96, 60), rng.integers(0, 3, 60)] = rng.choice(bad, 60)
        arrs[key] = np.concatenate([s[key], extra])
    full = len(arrs["pos"])
    for n, stride, M in ((full, 3, pad_m(ms, 3)), (full, ms + 5, 4), (full, 2, 1), (0, 1, 2)):
        series = []
        for _ in range(2):
            d = rng.normal(size=(M, n, 3)).astype(np.float32)
            if n:
                d[rng.integers(0, M, 80), rng.integers(0, n, 80), rng.integers(0, 3, 80)] = rng.choice(bad, 80)
            series.append(d)
        path = str(tmp_path / f"case_{n}_{stride}_{M}.bin")
        HC.write_case(path, list(s["res"]) + [n, stride, M], [s["h"], s["ds"]],
                      [s["rif"]] + [arrs[key][:n] for key in ("pos", "vel", "dx", "dv")] + series)
        r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "finished without reports" in r.stdout, (n, stride, M, r.stdout[-2000:], r.stderr[-4000:])
        assert f"{n} rays" in r.stdout


# ---- GPU tier -------------------------------------------------------------------------------------------------------
_hosts = {}


def host(name, stride, M):
    """(forward, seeds on path and vpath, adjoint with every seed set on every ray and the flag on) of the host build."""
    if (name, stride, M) not in _hosts:
        s = scene(name)
        k = fwd(s, stride, M)
        g, w = dpath_of(k["path"].shape, stride + M), dvpath_of(k["path"].shape, stride + M)
        _hosts[name, stride, M] = (k, g, w, back(s, k, s["dx"], s["dv"], g, w, stride, M, corrected_h=True))
    return _hosts[name, stride, M]


@pytest.mark.gpu
@pytest.mark.parametrize("pair", [False, True])
@pytest.mark.parametrize("name", list(SCENES))
def test_kernels_match_host_build(gpu, name, pair):
    """k_trace_phase and k_backtrace_phase (plain and pair-copy gathers; strides 1 and 7; an M that pads and an M that
    truncates; caller order and the forward's visit order) == the host build: both series, count, xt, vt, steps, dpos, dvel
    and the statistics bit for bit, the grid gradient to the order of its atomic sums."""
    from adjointnonlinearraytracing_amd import drrt
    s = scene(name)
    ms = max_steps_fwd(s["res"], s["h"], s["ds"])
    T = drrt.TracerC()
    for stride in (1, 7):
        for M in (pad_m(ms, stride), trunc_m(ms, stride)):
            k, g, w, r = host(name, stride, M)
            assert k["n_failed"] > 0
            for sort in (False, True):
                with drrt.using(pair_grid=pair, corrected_h=True, sort_rays=sort):
                    out, st, order = PC._gpu_forward_phase(T, s, gpu, stride, M)
                    assert (order is not None) == sort
                    PC._forward_matches(out, st, k)
                    (grad, dpos, dvel), bst = PC._gpu_back_phase(T, s, gpu, out, stride, g, w, order=order)
                assert _same(dpos, r["dpos"]) and _same(dvel, r["dvel"])
                assert bst["ray_steps"] == r["ray_steps"] and bst["n_failed"] == r["n_failed"] > 0
                err = cases.rel_l2(grad.cpu().numpy(), r["grad"])
                print(f"{name} pair={pair} stride={stride} M={M} sorted={sort}: grid rel-L2 vs host {err:.3e}")
                assert err <= ATOMIC_TOL


@pytest.mark.gpu
def test_kernel_variants(gpu):
    """The adjoint with the grid only, the rays only and both; accumulating into a pre-filled grid; with each seed null in
    turn (== the host build with that seed null, and == backtrace_path on the device when it is dvpath): what remains is
    unchanged bit for bit (rays) or to the order of the sums (grid)."""
    from adjointnonlinearraytracing_amd import drrt
    name, stride = "box7x11x5_h05_multi", 7
    s = scene(name)
    M = pad_m(max_steps_fwd(s["res"], s["h"], s["ds"]), stride)
    k, g, w, r = host(name, stride, M)
    T = drrt.TracerC()
    ok = lambda grad, want: cases.rel_l2(grad.cpu().numpy(), want["grad"]) <= ATOMIC_TOL      # noqa: E731
    with drrt.using(corrected_h=True, pair_grid=False):
        out, st, order = PC._gpu_forward_phase(T, s, gpu, stride, M)
        (grad, dpos, dvel), bst = PC._gpu_back_phase(T, s, gpu, out, stride, g, w)                 # sorts for itself
        assert _same(dpos, r["dpos"]) and _same(dvel, r["dvel"]) and ok(grad, r)
        assert bst["ray_steps"] == r["ray_steps"] and bst["n_failed"] == r["n_failed"]
        fill = torch.full((s["rif"].size,), 3.0, device=gpu)
        (grad, dpos, dvel), _ = PC._gpu_back_phase(T, s, gpu, out, stride, g, w, order=order, into=fill)
        assert grad.data_ptr() == fill.data_ptr() and _same(dpos, r["dpos"]) and _same(dvel, r["dvel"])
        assert cases.rel_l2(fill.cpu().numpy().astype(np.float64) - 3.0, r["grad"]) <= ATOMIC_TOL
        (grad, dpos, dvel), bst = PC._gpu_back_phase(T, s, gpu, out, stride, g, w, order=order, grid=False)
        assert grad is None and _same(dpos, r["dpos"]) and _same(dvel, r["dvel"]) and bst["ray_steps"] == r["ray_steps"]
        (grad, dpos, dvel), bst = PC._gpu_back_phase(T, s, gpu, out, stride, g, w, order=order, rays=False)
        assert dpos is None and dvel is None and ok(grad, r)
        assert bst["ray_steps"] == r["ray_steps"] and bst["n_failed"] == r["n_failed"]
        with pytest.raises(RuntimeError, match="nothing to compute"):
            PC._gpu_back_phase(T, s, gpu, out, stride, g, w, grid=False, rays=False)
        # each seed null in turn
        r0 = back(s, k, None, s["dv"], g, w, stride, M, corrected_h=True)
        (grad, dpos, dvel), _ = PC._gpu_back_phase(T, s, gpu, out, stride, g, w, order=order, dx=None)
        assert _same(dpos, r0["dpos"]) and _same(dvel, r0["dvel"]) and ok(grad, r0) and not np.array_equal(r0["dpos"], r["dpos"])
        r0 = back(s, k, s["dx"], None, g, w, stride, M, corrected_h=True)
        (grad, dpos, dvel), _ = PC._gpu_back_phase(T, s, gpu, out, stride, g, w, order=order, dv=None)
        assert _same(dpos, r0["dpos"]) and _same(dvel, r0["dvel"]) and ok(grad, r0) and not np.array_equal(r0["dvel"], r["dvel"])
        r0 = back(s, k, s["dx"], s["dv"], None, w, stride, M, corrected_h=True)
        (grad, dpos, dvel), _ = PC._gpu_back_phase(T, s, gpu, out, stride, None, w, order=order)
        assert _same(dpos, r0["dpos"]) and _same(dvel, r0["dvel"]) and ok(grad, r0) and not np.array_equal(r0["dpos"], r["dpos"])
        r0 = back(s, k, s["dx"], s["dv"], g, None, stride, M, corrected_h=True)
        (grad, dpos, dvel), _ = PC._gpu_back_phase(T, s, gpu, out, stride, g, None, order=order)
        assert _same(dpos, r0["dpos"]) and _same(dvel, r0["dvel"]) and ok(grad, r0) and not np.array_equal(r0["dvel"], r["dvel"])
        (pgrad, ppos, pvel), _ = PC._gpu_back(T, s, gpu, (out[0], out[1], out[2], out[4], out[5]), stride, g, order=order)
        assert torch.equal(ppos, dpos) and torch.equal(pvel, dvel) and ok(pgrad, r0)
        (grad, dpos, dvel), _ = PC._gpu_back_phase(T, s, gpu, out, stride, None, None, order=order, samples=M, grid=False)
        r0 = back(s, k, s["dx"], s["dv"], None, None, stride, M, corrected_h=True)
        assert _same(dpos, r0["dpos"]) and _same(dvel, r0["dvel"])
        # the forward == trace_path's on the device; samples=None is the smallest M that always ends on (xt, vt)
        pout, _, _ = PC._gpu_forward(T, s, gpu, stride, M)
        for a, b in zip((out[0], out[1], out[2], out[4], out[5]), pout):
            assert torch.equal(a, b)
        dflt, _, _ = PC._gpu_forward_phase(T, s, gpu, stride, None)
        assert dflt[3].shape[0] == M and _same(dflt[3], k["vpath"])


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 0, 257])
def test_edge_sizes(gpu, n):
    """n = 1, n = 0 and n = 257 (one ray past a block), each with a stride above every K and with M = 1 beside an ordinary
    series."""
    from adjointnonlinearraytracing_amd import drrt
    name = "lens16_h1_half"
    s = scene(name)
    ms = max_steps_fwd(s["res"], s["h"], s["ds"])
    k = fwd(s, 3, pad_m(ms, 3))
    if n == 1:
        i = int(np.where((s["labels"] == "inside") & (k["steps"] > 4) & (k["steps"] < 100))[0][0])
        sl = slice(i, i + 1)
    else:
        sl = slice(0, n)
    one = dict(s, **{key: s[key][sl] for key in ("pos", "vel", "dx", "dv")})
    assert len(one["pos"]) == n
    T = drrt.TracerC()
    for stride, M in ((3, pad_m(ms, 3)), (ms + 3, 2), (2, 1)):
        k1 = fwd(one, stride, M)
        g, w = dpath_of(k1["path"].shape, 5), dvpath_of(k1["path"].shape, 5)
        r1 = back(one, k1, one["dx"], one["dv"], g, w, stride, M, corrected_h=True)
        with drrt.using(corrected_h=True, check_failed=False):
            out, st, _ = PC._gpu_forward_phase(T, one, gpu, stride, M)
            (grad, dpos, dvel), bst = PC._gpu_back_phase(T, one, gpu, out, stride, g, w)
        PC._forward_matches(out, st, k1)
        assert tuple(out[3].shape) == (M, n, 3) and tuple(dpos.shape) == (n, 3)
        assert _same(dpos, r1["dpos"]) and _same(dvel, r1["dvel"])
        assert bst["ray_steps"] == r1["ray_steps"] and bst["n_failed"] == r1["n_failed"]
        if n == 0:
            assert not bool(grad.any()) and grad.numel() == s["rif"].size
        elif n == 1:
            assert r1["ray_steps"] > 4 and cases.rel_l2(grad.cpu().numpy(), r1["grad"]) <= 1e-6      # one lane: the host's order
        else:
            assert cases.rel_l2(grad.cpu().numpy(), r1["grad"]) <= ATOMIC_TOL


def _ad_grads(s, dev, stride, M, seeds, rif_grad=True, x_grad=True, v_grad=True, dtype=torch.float32):
    """PhasePathTracerC.apply -> L = <dx, xt> + <dv, vt> + <dpath, path> + <dvpath, vpath> -> backward ->
    (rif.grad, x.grad, v.grad, outputs)."""
    from adjointnonlinearraytracing_amd import tracer
    rif = _t(s["rif"], dev).requires_grad_(rif_grad)
    x = _t(s["pos"], dev).to(dtype).requires_grad_(x_grad)
    v = _t(s["vel"], dev).requires_grad_(v_grad)
    out = tracer.PhasePathTracerC.apply(rif, x, v, s["h"], s["ds"], stride, M)
    assert not out[4].requires_grad and out[4].dtype == torch.int32
    loss = sum((o * _t(np.asarray(w, np.float32), dev)).sum() for o, w in zip(out, seeds) if w is not None)
    if torch.is_tensor(loss) and loss.requires_grad:
        loss.backward()
    torch.cuda.synchronize()
    return rif.grad, x.grad, v.grad, [o.detach() for o in out]


@pytest.mark.gpu
def test_phase_tracer_end_to_end(gpu, oracle):
    """PhasePathTracerC.apply -> loss on xt, vt, path and vpath -> backward against float64 autograd on the compared rays of
    the plane source (tests/integral_common.py::_plane_case), under the caps of the CPU tier; a loss on vpath alone; only
    what is asked for comes back; launches: forward ["trace_phase"], backward ONE backtrace_phase plus the zero-fill when rif
    requires grad, none when nothing requires grad."""
    from adjointnonlinearraytracing_amd import _lib, drrt
    s = IC._plane_case()
    stride = 5
    M = pad_m(max_steps_fwd(s["res"], s["h"], s["ds"]), stride)
    cmp_ = IC.reference(oracle, s, "plane12")[1] & tie_free_for_yardstick(s)
    assert cmp_.sum() >= 120
    k = fwd(s, stride, M)
    g = dpath_of(k["path"].shape, 9) * cmp_[None, :, None]
    w = dvpath_of(k["path"].shape, 9) * cmp_[None, :, None]
    seeds = (s["dx"] * cmp_[:, None], s["dv"] * cmp_[:, None], g, w)
    T64 = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)      # noqa: E731
    for sd in (seeds, (None, None, None, w)):
        r_, p_, v_ = (T64(s[q]).requires_grad_(True) for q in ("rif", "pos", "vel"))
        out64 = integral_ad.trace_phase(r_, p_, v_, s["h"], s["ds"], stride, M)
        L = sum((o * T64(a)).sum() for o, a in zip(out64, sd) if a is not None)
        gr, gp, gv = (t.numpy() for t in torch.autograd.grad(L, (r_, p_, v_)))
        r = back(s, k, sd[0], sd[1], sd[2], sd[3], stride, M, corrected_h=True)
        with drrt.using(corrected_h=True):
            grif, gx, gvel, out = _ad_grads(s, gpu, stride, M, sd)
        assert _same(out[0], k["xt"]) and _same(out[1], k["vt"]) and _same(out[2], k["path"]) and _same(out[3], k["vpath"])
        assert np.array_equal(out[4].cpu().numpy(), k["count"])
        assert _same(gx, r["dpos"]) and _same(gvel, r["dvel"]) and tuple(grif.shape) == s["rif"].shape
        err = rel_err(gx.cpu().numpy(), gvel.cpu().numpy(), gp, gv)[cmp_].max()
        gerr = cases.rel_l2(grif.cpu().numpy(), gr.reshape(-1))
        print(f"PhasePathTracerC: {cmp_.sum()} rays compared; ray grad rel err max {err:.3e}; grid rel-L2 {gerr:.3e}")
        assert err <= CAPS["rays"] and gerr <= CAPS["grid"] and np.linalg.norm(gr) > 0.1
    with drrt.using(corrected_h=True):
        for rg, xg, vg in ((True, False, False), (False, True, False), (False, False, True), (True, False, True)):
            a, b, c, _ = _ad_grads(s, gpu, stride, M, seeds, rg, xg, vg)
            assert ((a is not None), (b is not None), (c is not None)) == (rg, xg, vg)
        with pytest.raises(RuntimeError, match="float32"):
            _ad_grads(s, gpu, stride, M, seeds, True, True, False, dtype=torch.float64)
        dflt = _ad_grads(s, gpu, stride, None, (None, None, None, None), False, False, False)[3]
        assert dflt[3].shape[0] == M
    lib = _lib.load()

    def launches(**kw):
        lib.drrt_profile_begin(256)
        try:
            _ad_grads(s, gpu, stride, M, seeds, **kw)
            return [name for name, _ in _lib.profile_collect()]
        finally:
            lib.drrt_profile_end()
    for sort, fw_ in ((False, ["trace_phase"]), (True, ["sort", "trace_phase"])):
        with drrt.using(sort_rays=sort, pair_grid=False):
            assert launches(rif_grad=False, x_grad=False, v_grad=False) == fw_
            assert launches() == fw_ + ["zero", "backtrace_phase"]
            assert launches(x_grad=False, v_grad=False) == fw_ + ["zero", "backtrace_phase"]
            assert launches(rif_grad=False) == fw_ + ["backtrace_phase"]


@pytest.mark.gpu
def test_demo(gpu):
    """examples/phase_path_demo.py at its smallest setting: it finishes, what it prints is finite, and the steering loss
    fell."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    try:
        import phase_path_demo
    finally:
        sys.path.pop(0)
    a = phase_path_demo.direction_integrand(res=17, side=12, verbose=False)
    print(f"phase_path_demo (1): circ from (path, vpath) {a['circ_path']:.6e}, VectorIntegralTracerC {a['circ_grid']:.6e}, "
          f"max difference {a['diff']:.3e}, |dL/drif| {a['grad_norm']:.3e}")
    assert all(np.isfinite(a[key]) for key in ("circ_path", "circ_grid", "diff", "grad_norm"))
    hist = phase_path_demo.steer(res=17, side=6, iters=15, verbose=False)
    print(f"phase_path_demo (2): loss {hist[0]:.4e} -> {hist[-1]:.4e}")
    assert len(hist) == 15 and np.isfinite(hist).all() and hist[-1] < hist[0]
