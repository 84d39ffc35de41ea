"""Ray paths: drrt_trace_path_f32 / drrt_backtrace_path_f32, TracerC.trace_path / backtrace_path, tracer.PathTracerC.

CPU tier: the host build of the product's per-ray routines (tests/hostcheck/integral_rays.hip: trace_path_ray and
path_backtrace_ray of csrc/drrt_device.h) against the product's own trace and opl adjoint (bit for bit), against float64
torch.autograd through tests/integral_ad (its one loop, recording x where the product does) on the compared rays, against
closed forms, and the C ABI's argument checks.  GPU tier: k_trace_path / k_backtrace_path of drrt_integral.hip against that
host build, the autograd class end to end, its launches, and the demo.

The referee (`referee`, shared with tests/test_path_fuzz.py): L = <dx, xt> + <dv, vt> + <dpath, path> through integral_ad in
float64, and once more in float32 as the yardstick.  A ray is compared when it is tie-free for the product and for the
yardstick (tests/integral_fuzz_common.py::masks); the seeds of every other ray are zero on all sides.  With e_prod the host
build against float64 and e_ref the float32 run against float64, measured the same way, the gradients are bounded by
integral_fuzz_common.bound(e_ref, CAPS[...]); a path sample's error is the largest absolute difference over the compared
rays and j < M over the box's longest edge and stays under CAPS["out"].  Modes: every seed; no seeds on the rays; dpath on
the prefix samples alone, on the in-box samples alone, on the padded entries alone (the last three without ray seeds).

On the parent commit every test here fails: the host build of the routines does not compile (no trace_path_ray), the library
has no such C symbols, TracerC no such methods, tracer no such class and examples/ no such demo.

Largest e_prod / max(e_ref, 2.4e-7) on the fixed scenes, host build (8 allowed): ray gradients 2.75 (lens16_h1_multi, stride 1,
prefix seeds alone), dL/drif 2.14 (box7x11x5_h05_multi, stride 5, in-box seeds alone), path samples 1.16.

Mutation checks (tried by hand on csrc/drrt_device.h, one at a time, each then undone; CPU tier of this file and of
tests/test_path_fuzz.py, 117 tests):
  * term.pull called behind adj_recur instead of in front of it: 83 fail;
  * the countdown of PathTerm started one iteration late (every in-box seed lands on x_{k-1}): 83 fail -- all 20 cases of
    test_referee_on_fixed_scenes, 62 of the 64 of test_path_fuzz.py::test_referee, test_uniform_medium_closed_form;
  * the padded seeds dropped: 92 fail -- the 84 referee cases, all five of test_adjoint_identities,
    test_uniform_medium_closed_form, test_exit_on_first_iteration_closed_form, test_never_entering_ray_closed_form."""
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
from integral_common import ATOMIC_TOL, _same, scene
from integral_fuzz_common import CAPS
import integral_host as OH
from oracle import torch_ad
from path_common import (STRIDES, _bits, _forward_matches, _gpu_back, _gpu_forward, back, count_of, dpath_of, fwd, pad_m, referee,
                         trunc_m)
from raygrad_common import SCENES, TIE_TOL, _t, max_steps_fwd, rel_err


# ---- the referee ------------------------------------------------------------------------------------------------------
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
    """The fixed scene's compared rays: tie-free for the product (tests/integral_common.py::reference) and for the yardstick."""
    if name not in _compared:
        s = scene(name)
        _compared[name] = IC.reference(oracle, s, name)[1] & tie_free_for_yardstick(s)
    return _compared[name]


# ---- CPU tier -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SCENES))
def test_forward_identities(name):
    """(xt, vt, steps) == the product's trace_ray<0>; path[0] == pos; every padded entry == xt; count == the formula; the
    stride-s path == every s-th row of the stride-1 path (s = 1, 2, 7 and one above every K); M = 3 leaves the first three
    rows unchanged: all bit for bit."""
    s = scene(name)
    ms = max_steps_fwd(s["res"], s["h"], s["ds"])
    t = HC.trace(s["rif"], s["res"], s["pos"], s["vel"], s["h"], s["ds"])
    one = fwd(s, 1, pad_m(ms, 1))
    K = one["steps"].astype(np.int64)
    assert K.max() == ms and (K < ms).sum() > 300
    for stride in (1, 2, 7, ms + 3):
        M = pad_m(ms, stride)
        k = one if stride == 1 else fwd(s, stride, M)
        assert np.array_equal(_bits(k["xt"]), _bits(t["xt"])) and np.array_equal(_bits(k["vt"]), _bits(t["vt"]))
        assert np.array_equal(k["steps"].astype(np.int64), t["steps"].astype(np.int64)) and k["n_failed"] == t["n_failed"] > 0
        assert np.array_equal(_bits(k["path"][0]), _bits(s["pos"]))
        cnt = count_of(k["steps"], stride, M)
        assert np.array_equal(k["count"], cnt) and cnt.min() >= 1 and cnt.max() < M
        padded = np.arange(M)[:, None] >= cnt[None, :]
        assert padded[-1].all() and np.array_equal(_bits(k["path"])[padded], _bits(np.broadcast_to(k["xt"], k["path"].shape))[padded])
        rows = one["path"][::stride][:M]
        sample = ~padded[:len(rows)]
        assert np.array_equal(_bits(k["path"][:len(rows)])[sample], _bits(rows)[sample])
        if stride > ms:
            assert (cnt == 1).all()
        cut = fwd(s, stride, 3)
        assert np.array_equal(_bits(cut["path"]), _bits(k["path"][:3])) if M >= 3 else True
        assert np.array_equal(cut["count"], np.minimum(cnt, 3)) and np.array_equal(_bits(cut["xt"]), _bits(k["xt"]))
    assert (count_of(one["steps"], 1, 3) == 3).sum() > 300          # M = 3 truncates: no padding on those rays


@pytest.mark.parametrize("name", list(SCENES))
def test_adjoint_identities(name):
    """dpath = 0 (zeros, and a null pointer): backtrace_opl's result with dopl = 0, rays and grid.  Seeds on padded entries
    alone: backtrace_opl's with dx plus their ascending fp32 sum.  Bit for bit on the rays, equal on the grid (both host
    builds sum it in double in the same order)."""
    s = scene(name)
    ms = max_steps_fwd(s["res"], s["h"], s["ds"])
    for stride in (1, 7):
        M = pad_m(ms, stride)
        k = fwd(s, stride, M)
        ref = OH.backtrace_opl(s["rif"], s["res"], s["pos"], s["vel"], k["xt"], k["vt"], k["steps"], s["dx"], s["dv"], None,
                               s["h"], s["ds"], corrected_h=True)
        for dpath in (None, np.zeros((M, len(s["pos"]), 3), np.float32)):
            r = back(s, k, s["dx"], s["dv"], dpath, stride, M, corrected_h=True)
            assert np.array_equal(_bits(r["dpos"]), _bits(ref["dpos"])) and np.array_equal(_bits(r["dvel"]), _bits(ref["dvel"]))
            assert np.array_equal(r["grad"], ref["grad"]) and np.array_equal(r["steps"], ref["steps"])
            assert np.array_equal(r["failed"], ref["failed"]) and r["n_failed"] > 0
        padded = np.arange(M)[:, None] >= k["count"][None, :]
        dpath = dpath_of((M, len(s["pos"]), 3), stride) * padded[:, :, None]
        dx = s["dx"].copy()
        for j in range(M):                                                 # ascending j, fp32
            dx = (dx + dpath[j]).astype(np.float32)
        assert padded.sum(0).max() >= 3 and not np.array_equal(dx, s["dx"])
        r = back(s, k, s["dx"], s["dv"], dpath, stride, M, corrected_h=True)
        ref = OH.backtrace_opl(s["rif"], s["res"], s["pos"], s["vel"], k["xt"], k["vt"], k["steps"], dx, s["dv"], None,
                               s["h"], s["ds"], corrected_h=True)
        assert np.array_equal(_bits(r["dpos"]), _bits(ref["dpos"])) and np.array_equal(_bits(r["dvel"]), _bits(ref["dvel"]))
        assert np.array_equal(r["grad"], ref["grad"])


@pytest.mark.parametrize("kind", ["pad", "trunc"])
@pytest.mark.parametrize("stride", STRIDES)
@pytest.mark.parametrize("name", list(SCENES))
def test_referee_on_fixed_scenes(oracle, name, stride, kind):
    """Forward and adjoint against float64 autograd of L = <dx, xt> + <dv, vt> + <dpath, path>, every mode."""
    s = scene(name)
    ms = max_steps_fwd(s["res"], s["h"], s["ds"])
    cmp_ = compared_rays(oracle, name)
    assert cmp_.sum() >= 400
    M = pad_m(ms, stride) if kind == "pad" else trunc_m(ms, stride)
    worst, bad, weight = referee(s, cmp_, stride, M, f"{name} stride={stride} M={M}")
    assert bad == []
    assert min(weight[m] for m in ("all", "noray", "prefix", "inbox")) > 100 and weight["padded"] > (100 if kind == "pad" else 0)


def test_uniform_medium_closed_form():
    """n = c everywhere: the rays are straight.  Positions, directions and ds are dyadic, so the fma chain x = fmaf(ds, v, x)
    is exact: path[j] == pos + j stride ds vel bit for bit, xt = pos + K ds vel, and with g_j the seed on path[j]
    dpos = dx + sum_j g_j, dvel = dv + K ds (dx + sum_{padded} g_j) + sum_{j < count} (j stride ds) g_j."""
    res, h, ds, c = (9, 8, 7), 1.0, 0.5, 1.25
    rif = np.full((res[2], res[1], res[0]), c, np.float32)
    pos = np.array([(3.25, -1.25, 3.5), (0.0, 2.5, 1.125), (4.5, 3.5, 2.75), (-2.0, 3.0, 3.0), (7.875, 6.75, 5.5)], np.float32)
    vel = np.array([(0.25, 1.0, 0.125), (1.0, 0.0, 0.0), (-0.5, 0.25, 0.75), (1.0, 0.125, -0.25), (0.125, 0.125, 0.0625)], np.float32)
    s = dict(rif=rif, res=res, h=h, ds=ds, pos=pos, vel=vel)
    ms = max_steps_fwd(res, h, ds)
    rng = np.random.default_rng(2)
    dyadic = lambda shape: (rng.integers(-8, 9, shape) / 4.0).astype(np.float32)      # noqa: E731
    dx, dv = dyadic(pos.shape), dyadic(pos.shape)
    for stride in (1, 3):
        M = pad_m(ms, stride)
        k = fwd(s, stride, M)
        K = k["steps"].astype(np.int64)
        assert (K < ms).all() and K.min() >= 2 and K.max() >= 12
        idx = np.arange(M)[:, None] * stride
        sample = idx < K[None, :]
        exact = pos[None].astype(np.float64) + (idx * ds)[:, :, None] * vel[None].astype(np.float64)
        assert np.array_equal(k["path"].astype(np.float64)[sample], exact[sample])
        assert np.array_equal(k["xt"].astype(np.float64), pos + (K * ds)[:, None] * vel.astype(np.float64))
        assert np.array_equal(k["count"], sample.sum(0))
        g = dyadic(k["path"].shape)
        r = back(s, k, dx, dv, g, stride, M)
        g64 = g.astype(np.float64)
        want_p = dx + g64.sum(0)
        want_v = dv + (K * ds)[:, None] * (dx + (g64 * ~sample[:, :, None]).sum(0)) + (g64 * (sample * idx * ds)[:, :, None]).sum(0)
        np.testing.assert_allclose(r["dpos"], want_p, rtol=1e-6, atol=1e-6)
        np.testing.assert_allclose(r["dvel"], want_v, rtol=1e-6, atol=1e-6)


def test_exit_on_first_iteration_closed_form():
    """e = 0, K = 1 (tests/test_opl.py's case): count = 1, path = (pos, xt, xt, ...); with dx' = dx + the padded seeds,
    dvel = mu = dv + ds dx', dpos = dx' + ds J(x0)^T mu + g_0, J = d(n grad n)/dx at x0."""
    rif = cases.luneburg(16)
    h, ds, res = 1.0, 0.5, (16, 16, 16)
    pos = np.array([[14.8, 7.3, 6.1]], np.float32)
    vel = np.array([[1.0, 0.1, -0.05]], np.float32)
    s = dict(rif=rif, res=res, h=h, ds=ds, pos=pos, vel=vel)
    k = fwd(s, 1, 4)
    assert k["steps"][0] == 1 and k["count"][0] == 1
    assert np.array_equal(_bits(k["path"][:, 0]), _bits(np.stack([pos[0], k["xt"][0], k["xt"][0], k["xt"][0]])))
    dx = np.array([[0.3, -1.2, 0.7]], np.float32); dv = np.array([[-0.4, 0.9, 0.2]], np.float32)
    g = np.array([[[1.1, -0.6, 0.4]], [[0.2, 0.5, -0.9]], [[-0.3, 0.8, 0.1]], [[0.9, -0.2, 0.7]]], np.float32)
    r = back(s, k, dx, dv, g, 1, 4)
    R = torch.tensor(rif, dtype=torch.float64)
    x = torch.tensor(pos[0], dtype=torch.float64)
    f = lambda y: (lambda nn, gg: (nn[:, None] * gg)[0])(*torch_ad.eval_grad(R, y[None], h, torch.tensor([True])))   # noqa: E731
    J = torch.autograd.functional.jacobian(f, x).numpy()
    dxp = dx[0].astype(np.float64) + g[1:, 0].astype(np.float64).sum(0)
    mu = dv[0].astype(np.float64) + ds * dxp
    np.testing.assert_allclose(r["dvel"][0], mu, rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(r["dpos"][0], dxp + ds * J.T @ mu + g[0, 0], rtol=1e-5, atol=1e-6)
    assert r["steps"][0] == 1 and np.abs(r["grad"]).max() > 0


def test_never_entering_ray_closed_form():
    """A ray outside the box that points away: K = 1, and one that flies past it: K > 1, e = K.  xt = pos, so the padded
    entries are pos; the samples are the free flight's.  The gradient is (dx, dv) plus the padded seeds (on dx, ascending j,
    fp32) plus the prefix seeds (ascending j: dpos += g, dvel = fmaf((float)k ds, g, dvel)), bit for bit; no grid
    contribution."""
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
        cnt = count_of(k["steps"], stride, M)
        assert np.array_equal(k["count"], cnt)
        g = rng.normal(size=(M, 2, 3)).astype(np.float32)
        r = back(s, k, dx, dv, g, stride, M)
        for i in range(2):
            x = pos[i].copy()
            for j in range(M):
                want = x if j < cnt[i] else pos[i]
                assert np.array_equal(_bits(k["path"][j, i]), _bits(want)), (stride, M, i, j)
                for _ in range(stride):
                    x = (np.float64(ds) * vel[i].astype(np.float64) + x.astype(np.float64)).astype(np.float32)      # fmaf: one rounding
            dp, dw = dx[i].copy(), dv[i].copy()
            for j in range(cnt[i], M):
                dp = (dp + g[j, i]).astype(np.float32)
            for j in range(cnt[i]):
                dp = (dp + g[j, i]).astype(np.float32)
                kds = np.float32(np.float32(j * stride) * np.float32(ds))
                dw = (kds.astype(np.float64) * g[j, i].astype(np.float64) + dw.astype(np.float64)).astype(np.float32)
            assert np.array_equal(_bits(r["dpos"][i]), _bits(dp)) and np.array_equal(_bits(r["dvel"][i]), _bits(dw)), (stride, M, i)
        assert not r["grad"].any() and r["ray_steps"] == 0 and r["n_failed"] == 0


def test_failed_ray():
    """A ray at rest outside the box never leaves: K = max_steps.  Forward: the samples are pos, and so is xt.  Adjoint: zeros,
    counted, no grid contribution, whatever the seeds."""
    s = scene("lens16_h1_half")
    ms = max_steps_fwd(s["res"], s["h"], s["ds"])
    i = np.where(s["labels"] == "zero")[0][:8]
    one = dict(s, pos=s["pos"][i], vel=s["vel"][i])
    for stride, M in ((1, pad_m(ms, 1)), (7, pad_m(ms, 7)), (ms, 2), (1, 3)):
        k = fwd(one, stride, M)
        assert (k["steps"] == ms).all() and k["n_failed"] == 8 and np.array_equal(k["count"], count_of(k["steps"], stride, M))
        assert np.array_equal(_bits(k["path"]), _bits(np.broadcast_to(one["pos"], k["path"].shape)))
        g = dpath_of(k["path"].shape, 1)
        r = back(one, k, s["dx"][i], s["dv"][i], g, stride, M)
        assert r["n_failed"] == 8 and r["failed"].all() and not r["dpos"].any() and not r["dvel"].any()
        assert not r["grad"].any() and r["ray_steps"] == 0


def test_abi_and_python_surface():
    """The C symbols are exported and bound, the two profile ids are named, the methods and the class exist, and the class
    refuses CPU tensors as the family's classes do (no fallback)."""
    from adjointnonlinearraytracing_amd import _lib, drrt, tracer
    lib = C.CDLL(_lib.LIB_PATH)
    for name in ("drrt_trace_path_f32", "drrt_backtrace_path_f32"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    names = {**_lib.PROF_NAMES, **_lib.PROF_NAMES_MORE, **_lib.PROF_NAMES_LATER}
    assert names[23] == "trace_path" and names[24] == "backtrace_path" and names[22] == "backtrace_cable_field"
    assert callable(drrt.TracerC.trace_path) and callable(drrt.TracerC.backtrace_path) and callable(drrt.TracerC._trace_path)
    assert issubclass(tracer.PathTracerC, torch.autograd.Function)
    with open(os.path.join(os.path.dirname(_lib.LIB_PATH), "..", "include", "drrt_hip.h")) as f:
        hdr = f.read()
    assert "drrt_trace_path_f32" in hdr and "drrt_backtrace_path_f32" in hdr
    assert "#define DRRT_PROF_TRACE_PATH 23" in hdr and "#define DRRT_PROF_BACKTRACE_PATH 24" in hdr
    assert drrt.path_max_steps((16, 16, 16), 0.5, 0.25) == max_steps_fwd((16, 16, 16), 0.5, 0.25) == 128
    assert drrt.path_max_steps((7, 11, 5), 0.5, 0.8) == max_steps_fwd((7, 11, 5), 0.5, 0.8)
    rif = torch.ones(8, 8, 8, requires_grad=True)
    x, v = torch.zeros(4, 3), torch.ones(4, 3)
    with pytest.raises(RuntimeError, match="cuda"):
        tracer.PathTracerC.apply(rif, x, v, 1.0, 0.5, 1, None)
    with pytest.raises(RuntimeError, match="cuda"):
        drrt.TracerC().trace_path(rif.detach(), (8, 8, 8), x, v, 1.0, 0.5, 1)


def test_abi_argument_checks():
    """stride < 1, samples < 1, samples n 3 floats overflowing size_t, null pointers, all outputs null, too many rays and bad
    steps are refused before anything is launched; n = 0 is fine."""
    from adjointnonlinearraytracing_amd import _lib
    lib = _lib.load()
    rif = np.ones(8 * 8 * 8, np.float32)
    a = np.zeros((4, 3), np.float32); pth = np.zeros((5, 4, 3), np.float32)
    cnt = np.zeros(4, np.int32); st = np.zeros(4, np.uint32)
    P = lambda x: C.c_void_p(x.ctypes.data) if x is not None else None    # noqa: E731 (host pointers: never launched)

    def fw(rif_=rif, res=(8, 8, 8), n=4, pos=a, xt=a, path=pth, count=cnt, steps=st, h=1.0, ds=0.5, stride=2, samples=5):
        return lib.drrt_trace_path_f32(P(rif_), rif.size, (C.c_int * 3)(*res), n, P(pos), P(a), h, ds, stride, samples, P(xt),
                                       P(a), P(path), P(count), P(steps), None, None, 0, 0, None)

    def bw(rif_=rif, res=(8, 8, 8), n=4, pos=a, xt=a, steps=st, dx=a, dpath=pth, grad=None, dpos=a, dvel=a, h=1.0, ds=0.5,
           stride=2, samples=5):
        return lib.drrt_backtrace_path_f32(P(rif_), rif.size, (C.c_int * 3)(*res), n, P(pos), P(a), P(xt), P(a), P(steps),
                                           P(dx), P(a), P(dpath), h, ds, stride, samples, P(grad), P(dpos), P(dvel), None,
                                           None, 0, 0, None)
    big = (1 << 32) - 1
    for call, kw, rc, msg in (
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
            (bw, dict(rif_=None), _lib.ERR_ARG, "null rif"), (bw, dict(res=(1, 8, 64)), _lib.ERR_BAD_RES, "invalid resolution"),
            (bw, dict(pos=None), _lib.ERR_ARG, "null ray"), (bw, dict(xt=None), _lib.ERR_ARG, "null ray"),
            (bw, dict(steps=None), _lib.ERR_ARG, "fwd_steps"), (bw, dict(dpos=None, dvel=None), _lib.ERR_ARG, "null output"),
            (bw, dict(dpos=None), _lib.ERR_ARG, "together"), (bw, dict(dvel=None), _lib.ERR_ARG, "together"),
            (bw, dict(n=1 << 33), _lib.ERR_ARG, "uint32"), (bw, dict(ds=-1.0), _lib.ERR_ARG, "positive"),
            (bw, dict(h=0.0), _lib.ERR_ARG, "positive")):
        assert call(**kw) == rc, kw
        assert msg in _lib.last_error(), (kw, _lib.last_error())
    assert fw(n=0) == 0 and _lib.last_error() == ""
    assert bw(stride=0) == _lib.ERR_ARG and _lib.last_error() != ""
    assert bw(n=0, dx=None, dpath=None, pos=None) == 0 and _lib.last_error() == ""


def test_routines_under_sanitizers(tmp_path):
    """tests/hostcheck/integral_rays.hip as a stand-alone program (its own main), compiled for the host with ASan + UBSan and run
    as a child process, nothing preloaded: scene 1 plus rays and seeds with NaN, Inf, huge and denormal entries, with a
    stride above every K, with M = 1, and with zero rays."""
    exe = HC.sanitized_program(tmp_path, OH.SOURCE, "PATH_MAIN")
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
        dpath = rng.normal(size=(M, n, 3)).astype(np.float32)
        if n:
            dpath[rng.integers(0, M, 80), rng.integers(0, n, 80), rng.integers(0, 3, 80)] = rng.choice(bad, 80)
        path = str(tmp_path / f"case_{n}_{stride}_{M}.bin")
        HC.write_case(path, list(s["res"]) + [n, stride, M], [s["h"], s["ds"]],
                      [s["rif"]] + [arrs[key][:n] for key in ("pos", "vel", "dx", "dv")] + [dpath])
        r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "finished without reports" in r.stdout, (n, stride, M, r.stdout[-2000:], r.stderr[-4000:])
        assert f"{n} rays" in r.stdout


# ---- GPU tier -------------------------------------------------------------------------------------------------------
_hosts = {}


def host(name, stride, M):
    """(forward, seed on path, adjoint with every seed set on every ray and the flag on) of the host build."""
    if (name, stride, M) not in _hosts:
        s = scene(name)
        k = fwd(s, stride, M)
        g = dpath_of(k["path"].shape, stride + M)
        _hosts[name, stride, M] = (k, g, back(s, k, s["dx"], s["dv"], g, stride, M, corrected_h=True))
    return _hosts[name, stride, M]


@pytest.mark.gpu
@pytest.mark.parametrize("pair", [False, True])
@pytest.mark.parametrize("name", list(SCENES))
def test_kernels_match_host_build(gpu, name, pair):
    """k_trace_path and k_backtrace_path (plain and pair-copy gathers; strides 1 and 7; an M that pads and an M that
    truncates; caller order and the forward's visit order) == the host build: path, count, xt, vt, steps, dpos, dvel and the
    statistics bit for bit, the grid gradient to the order of its atomic sums."""
    from adjointnonlinearraytracing_amd import drrt
    s = scene(name)
    ms = max_steps_fwd(s["res"], s["h"], s["ds"])
    T = drrt.TracerC()
    for stride in (1, 7):
        for M in (pad_m(ms, stride), trunc_m(ms, stride)):
            k, g, r = host(name, stride, M)
            assert k["n_failed"] > 0
            for sort in (False, True):
                with drrt.using(pair_grid=pair, corrected_h=True, sort_rays=sort):
                    out, st, order = _gpu_forward(T, s, gpu, stride, M)
                    assert (order is not None) == sort
                    _forward_matches(out, st, k)
                    (grad, dpos, dvel), bst = _gpu_back(T, s, gpu, out, stride, g, order=order)
                assert _same(dpos, r["dpos"]) and _same(dvel, r["dvel"])
                assert bst["ray_steps"] == r["ray_steps"] and bst["n_failed"] == r["n_failed"] > 0
                err = cases.rel_l2(grad.cpu().numpy(), r["grad"])
                print(f"{name} pair={pair} stride={stride} M={M} sorted={sort}: grid rel-L2 vs host {err:.3e}")
                assert err <= ATOMIC_TOL


@pytest.mark.gpu
def test_kernel_variants(gpu):
    """The adjoint with its own sort, in caller order, accumulating into a pre-filled grid (DRRT_FLAG_NO_ZERO), without the
    grid, without the ray outputs, with null seeds and with the flag off: what remains is unchanged bit for bit (rays) or to
    the order of the sums (grid)."""
    from adjointnonlinearraytracing_amd import drrt
    name, stride = "box7x11x5_h05_multi", 7
    s = scene(name)
    M = pad_m(max_steps_fwd(s["res"], s["h"], s["ds"]), stride)
    k, g, r = host(name, stride, M)
    T = drrt.TracerC()
    ok = lambda grad, want: cases.rel_l2(grad.cpu().numpy(), want["grad"]) <= ATOMIC_TOL      # noqa: E731
    with drrt.using(corrected_h=True, pair_grid=False):
        out, st, order = _gpu_forward(T, s, gpu, stride, M)
        (grad, dpos, dvel), bst = _gpu_back(T, s, gpu, out, stride, g)                       # sorts for itself
        assert _same(dpos, r["dpos"]) and _same(dvel, r["dvel"]) and ok(grad, r)
        assert bst["ray_steps"] == r["ray_steps"] and bst["n_failed"] == r["n_failed"]
        with drrt.using(sort_rays=False):
            (grad, dpos, dvel), bst = _gpu_back(T, s, gpu, out, stride, g)                   # caller order
        assert _same(dpos, r["dpos"]) and _same(dvel, r["dvel"]) and ok(grad, r)
        fill = torch.full((s["rif"].size,), 3.0, device=gpu)
        (grad, dpos, dvel), _ = _gpu_back(T, s, gpu, out, stride, g, order=order, into=fill)
        assert grad.data_ptr() == fill.data_ptr() and _same(dpos, r["dpos"]) and _same(dvel, r["dvel"])
        assert cases.rel_l2(fill.cpu().numpy().astype(np.float64) - 3.0, r["grad"]) <= ATOMIC_TOL
        (grad, dpos, dvel), bst = _gpu_back(T, s, gpu, out, stride, g, order=order, grid=False)
        assert grad is None and _same(dpos, r["dpos"]) and _same(dvel, r["dvel"]) and bst["ray_steps"] == r["ray_steps"]
        (grad, dpos, dvel), bst = _gpu_back(T, s, gpu, out, stride, g, order=order, rays=False)
        assert dpos is None and dvel is None and ok(grad, r)
        assert bst["ray_steps"] == r["ray_steps"] and bst["n_failed"] == r["n_failed"]
        with pytest.raises(RuntimeError, match="nothing to compute"):
            _gpu_back(T, s, gpu, out, stride, g, grid=False, rays=False)
        # null seeds == zero seeds, each kind
        r0 = back(s, k, None, None, g, stride, M, corrected_h=True)
        (grad, dpos, dvel), _ = _gpu_back(T, s, gpu, out, stride, g, order=order, dx=None, dv=None)
        assert _same(dpos, r0["dpos"]) and _same(dvel, r0["dvel"]) and ok(grad, r0) and not np.array_equal(r0["dpos"], r["dpos"])
        r1 = back(s, k, s["dx"], s["dv"], None, stride, M, corrected_h=True)
        (grad, dpos, dvel), _ = _gpu_back(T, s, gpu, out, stride, None, order=order, samples=M)
        assert _same(dpos, r1["dpos"]) and _same(dvel, r1["dvel"]) and ok(grad, r1) and not np.array_equal(r1["dpos"], r["dpos"])
        # samples=None is the smallest M that always ends on xt
        dflt, _, _ = _gpu_forward(T, s, gpu, stride, None)
        assert dflt[2].shape[0] == M and _same(dflt[2], k["path"])
    roff = back(s, k, s["dx"], s["dv"], g, stride, M, corrected_h=False)
    with drrt.using(corrected_h=False, pair_grid=False):
        (grad, dpos, dvel), _ = _gpu_back(T, s, gpu, out, stride, g, order=order)
    assert _same(dpos, r["dpos"]) and ok(grad, roff) and cases.rel_l2(roff["grad"], r["grad"]) > 0.1


@pytest.mark.gpu
def test_single_ray_and_no_rays(gpu):
    from adjointnonlinearraytracing_amd import drrt
    name, stride = "lens16_h1_half", 3
    s = scene(name)
    M = pad_m(max_steps_fwd(s["res"], s["h"], s["ds"]), stride)
    k = fwd(s, stride, M)
    i = int(np.where((s["labels"] == "inside") & (k["steps"] > 4) & (k["steps"] < 100))[0][0])
    T = drrt.TracerC()
    for sl in (slice(i, i + 1), slice(0, 0)):
        one = dict(s, **{key: s[key][sl] for key in ("pos", "vel", "dx", "dv")})
        k1 = fwd(one, stride, M)
        g = dpath_of(k1["path"].shape, 5)
        r1 = back(one, k1, one["dx"], one["dv"], g, stride, M, corrected_h=True)
        with drrt.using(corrected_h=True):
            out, st, _ = _gpu_forward(T, one, gpu, stride, M)
            (grad, dpos, dvel), bst = _gpu_back(T, one, gpu, out, stride, g)
        _forward_matches(out, st, k1)
        assert tuple(out[2].shape) == (M, sl.stop - sl.start, 3) and tuple(dpos.shape) == (sl.stop - sl.start, 3)
        assert _same(dpos, r1["dpos"]) and _same(dvel, r1["dvel"]) and bst["ray_steps"] == r1["ray_steps"] and bst["n_failed"] == 0
        if sl.stop > sl.start:
            assert r1["ray_steps"] > 4 and cases.rel_l2(grad.cpu().numpy(), r1["grad"]) <= 1e-6      # one lane: the host's order
        else:
            assert not bool(grad.any()) and grad.numel() == s["rif"].size


def _ad_grads(s, dev, stride, M, seeds, rif_grad=True, x_grad=True, v_grad=True, dtype=torch.float32):
    """PathTracerC.apply -> L = <dx, xt> + <dv, vt> + <dpath, path> -> backward -> (rif.grad, x.grad, v.grad, outputs)."""
    from adjointnonlinearraytracing_amd import tracer
    rif = _t(s["rif"], dev).requires_grad_(rif_grad)
    x = _t(s["pos"], dev).to(dtype).requires_grad_(x_grad)
    v = _t(s["vel"], dev).requires_grad_(v_grad)
    out = tracer.PathTracerC.apply(rif, x, v, s["h"], s["ds"], stride, M)
    assert not out[3].requires_grad and out[3].dtype == torch.int32
    loss = sum((o * _t(np.asarray(w, np.float32), dev)).sum() for o, w in zip(out, seeds) if w is not None)
    if torch.is_tensor(loss) and loss.requires_grad:
        loss.backward()
    torch.cuda.synchronize()
    return rif.grad, x.grad, v.grad, [o.detach() for o in out]


@pytest.mark.gpu
def test_path_tracer_end_to_end(gpu, oracle):
    """PathTracerC.apply -> loss on xt, vt and path -> backward against float64 autograd on the compared rays of the plane
    source (tests/integral_common.py::_plane_case), under the bound of the CPU tier; a loss on path alone; only what is asked for
    comes back; the forward's options reach the backward launch."""
    from adjointnonlinearraytracing_amd import drrt
    s = IC._plane_case()
    stride = 5
    M = pad_m(max_steps_fwd(s["res"], s["h"], s["ds"]), stride)
    cmp_ = IC.reference(oracle, s, "plane12")[1] & tie_free_for_yardstick(s)
    assert cmp_.sum() >= 120
    k = fwd(s, stride, M)
    g = dpath_of(k["path"].shape, 9) * cmp_[None, :, None]
    seeds = (s["dx"] * cmp_[:, None], s["dv"] * cmp_[:, None], g)
    T64 = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)      # noqa: E731

    def autograd64(c, sd):
        r, p, v = (T64(c[q]).requires_grad_(True) for q in ("rif", "pos", "vel"))
        out = integral_ad.trace_path(r, p, v, c["h"], c["ds"], stride, M)
        L = sum((o * T64(w)).sum() for o, w in zip(out, sd) if w is not None)
        gr, gp, gv = torch.autograd.grad(L, (r, p, v))
        return gr.numpy().reshape(-1), gp.numpy(), gv.numpy()
    for sd in (seeds, (None, None, g)):
        gr, gp, gv = autograd64(s, sd)
        r = back(s, k, sd[0], sd[1], g, stride, M, corrected_h=True)
        with drrt.using(corrected_h=True):
            grif, gx, gvel, out = _ad_grads(s, gpu, stride, M, sd)
        assert _same(out[0], k["xt"]) and _same(out[1], k["vt"]) and _same(out[2], k["path"])
        assert np.array_equal(out[3].cpu().numpy(), k["count"])
        assert _same(gx, r["dpos"]) and _same(gvel, r["dvel"]) and tuple(grif.shape) == s["rif"].shape
        err = rel_err(gx.cpu().numpy(), gvel.cpu().numpy(), gp, gv)[cmp_].max()
        gerr = cases.rel_l2(grif.cpu().numpy(), gr)
        print(f"PathTracerC: {cmp_.sum()} rays compared; ray grad rel err max {err:.3e}; grid rel-L2 {gerr:.3e}")
        assert err <= CAPS["rays"] and gerr <= CAPS["grid"] and np.linalg.norm(gr) > 0.1
    with drrt.using(corrected_h=True):
        for rg, xg, vg in ((True, False, False), (False, True, False), (False, False, True), (True, False, True)):
            a, b, c, _ = _ad_grads(s, gpu, stride, M, seeds, rg, xg, vg)
            assert ((a is not None), (b is not None), (c is not None)) == (rg, xg, vg)
        with pytest.raises(RuntimeError, match="float32"):
            _ad_grads(s, gpu, stride, M, seeds, True, True, False, dtype=torch.float64)
        dflt = _ad_grads(s, gpu, stride, None, (None, None, None), False, False, False)[3]
        assert dflt[2].shape[0] == M
    s2 = IC._plane_case(h=0.5)
    gr2 = autograd64(s2, seeds)[0]
    with drrt.using(corrected_h=True):
        on = _ad_grads(s2, gpu, stride, M, seeds)[0].cpu().numpy()
    with drrt.using(corrected_h=False):
        off = _ad_grads(s2, gpu, stride, M, seeds)[0].cpu().numpy()
    assert cases.rel_l2(on, gr2) <= CAPS["grid"] and cases.rel_l2(off, gr2) > 0.1


@pytest.mark.gpu
def test_path_tracer_launches(gpu):
    """Forward: ["trace_path"].  Backward: ONE backtrace_path launch, plus the zero-fill when rif requires grad; none when
    nothing requires grad."""
    from adjointnonlinearraytracing_amd import _lib, drrt
    s = IC._plane_case()
    stride = 5
    M = pad_m(max_steps_fwd(s["res"], s["h"], s["ds"]), stride)
    seeds = (s["dx"], s["dv"], dpath_of((M, len(s["pos"]), 3), 3))
    lib = _lib.load()

    def launches(**kw):
        lib.drrt_profile_begin(256)
        try:
            _ad_grads(s, gpu, stride, M, seeds, **kw)
            return [name for name, _ in _lib.profile_collect()]
        finally:
            lib.drrt_profile_end()
    for sort, fw_ in ((False, ["trace_path"]), (True, ["sort", "trace_path"])):
        with drrt.using(sort_rays=sort, pair_grid=False):
            assert launches(rif_grad=False, x_grad=False, v_grad=False) == fw_
            assert launches() == fw_ + ["zero", "backtrace_path"]
            assert launches(x_grad=False, v_grad=False) == fw_ + ["zero", "backtrace_path"]
            assert launches(rif_grad=False) == fw_ + ["backtrace_path"]


@pytest.mark.gpu
def test_demo(gpu):
    """examples/path_demo.py at a reduced size: (a) the two optical depths agree to the quadrature error it prints and the
    gradient to rif is not zero; (b) the loss ends below where it began."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    try:
        import path_demo
    finally:
        sys.path.pop(0)
    a = path_demo.custom_integrand(res=17, side=12, verbose=False)
    print(f"path_demo (a): |tau_path - tau_grid| max {a['diff']:.3e}, quadrature error estimate {a['quadrature']:.3e}, "
          f"|dL/drif| {a['grad_norm']:.3e}")
    assert np.isfinite(a["diff"]) and a["diff"] <= a["quadrature"] and a["grad_norm"] > 0 and a["tau_max"] > 0.1
    hist = path_demo.steer(res=17, side=6, iters=15, verbose=False)
    print(f"path_demo (b): loss {hist[0]:.4e} -> {hist[-1]:.4e}")
    assert len(hist) == 15 and np.isfinite(hist).all() and hist[-1] < hist[0]
