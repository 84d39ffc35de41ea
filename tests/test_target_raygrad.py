"""Ray-state adjoint of the target march (drrt_backtrace_target_rays_f32, tracer.ADRayTargetTracerC): dL/dpos and dL/dvel from
seeds on the closest-approach record (xt, vt) AND on dist2, and dL/dtarget.

CPU tier: the host build of the product's per-ray routine (tests/hostcheck/target_rays.hip: target_backtrace_ray_state of
csrc/drrt_device.h, both passes) against torch.autograd in float64 through tests/target_ad (the reference's whole global loop
with its masks), on the tie-free rays: those whose fp32 and fp64 records agree to TIE_TOL and were written on the same
iteration.  GPU tier: the target kernels of drrt_ray_adjoints.hip against that host build bit for bit, the autograd class end to end,
and its launches.

On the parent commit every test here fails: tests/hostcheck/target_rays.hip does not compile (no
target_backtrace_ray_state), the library has no such C symbol, TracerC no such method and tracer no such class.

The kinds of record, from the replay (e = the free-flight iterations before the first in-box sample, done = phase A's count):
j = 0 (the input), 0 < j <= e (inside the prefix), e < j <= done (inside the sampled run), j > done (after the escape).

Mutation checks (tried by hand on the routine, one at a time, each then undone; CPU tier):
  * dropping the free flight's update of q for a record written after the escape: all ten cases of
    test_host_routine_matches_float64_autograd fail (the rays that never enter the box: no sampled run follows, so q is the
    result); the closed forms pass, as they must: before a sampled run that q is a dead store;
  * starting the sampled run of such a record from the record instead of phase A's end state: the same ten fail;
  * sampling the first in-box iteration at the reconstructed position instead of the replayed one: the same ten fail;
  * dropping the free-flight prefix: all ten and test_uniform_medium_closed_form fail;
  * gx = dx + dd2 (x_j - t), the factor 2 lost: all ten and both closed forms fail."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import cases
import hostcheck_lib as HC
import stop_ad
import target_ad
import target_raygrad_host as TH
from raygrad_common import GRAD_TOL, SCENES, TIE_TOL, _t, grads, rel_err, target_scene

MAX_DROPPED = 0.10      # share of a case's rays that may be left out as not tie-free (test_stop_raygrad's cap)
ENTERING = ("plane", "point", "inside", "face")
CASES = [(n, z) for n in SCENES for z in ("zero", "nozero")]


def fuzz_scene(k):
    s = dict(cases.fuzz_config(k))
    W, H, D = s["res"]
    ext = np.array([(W - 1) * s["h"], (H - 1) * s["h"], (D - 1) * s["h"]])
    s["tg"] = (np.random.default_rng(31 + k).uniform(-0.3, 1.3, s["pos"].shape) * ext).astype(np.float32)
    s["dd2"] = np.random.default_rng(17).normal(size=len(s["pos"])).astype(np.float32)
    return s


def _case(case):
    return fuzz_scene(int(case[4:])) if case.startswith("fuzz") else target_scene(*case.split("/"))


_host = {}


def host(case, s=None, dd2=True):
    """The host routine on a named case, computed once per (case, with the dist2 seed or without)."""
    if (case, dd2) not in _host:
        s = s or _case(case)
        _host[case, dd2] = TH.backtrace_target_rays(s["rif"], s["res"], s["pos"], s["vel"], s["tg"], s["dx"], s["dv"], s["h"],
                                                    s["ds"], ddist2=s["dd2"] if dd2 else None)
    return _host[case, dd2]


def prefix_length(s, limit):
    """e per ray: the straight-flight iterations x += ds v (fp32) before the first in-bounds position, capped at `limit`."""
    x, v = s["pos"].astype(np.float64), s["vel"].astype(np.float64)
    hi = s["ext"].astype(np.float32).astype(np.float64)
    ds = float(np.float32(s["ds"]))
    e = np.zeros(len(x), np.int64)
    going = np.ones(len(x), bool)
    for _ in range(int(limit)):
        going &= ~((x >= 0) & (x < hi)).all(1)
        if not going.any():
            break
        e[going] += 1
        x = (x + ds * v).astype(np.float32).astype(np.float64)
    return e


def record_kinds(s, r):
    j, done = r["jstar"].astype(np.int64), r["fwd"].astype(np.int64)
    e = np.minimum(prefix_length(s, done.max()), done)
    return dict(input=j == 0, prefix=(j > 0) & (j <= e), sampled=(j > e) & (j <= done), after=j > done)


def autograd64(s):
    """float64 torch.autograd of L = <dx, xt> + <dv, vt> + <dd2, dist2> through target_ad
    -> (xt, vt, dist2, j, dL/dpos, dL/dvel, dL/dtarget)."""
    T = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)      # noqa: E731
    p, v, t = (T(s[k]).requires_grad_(True) for k in ("pos", "vel", "tg"))
    xt, vt, d2, j = target_ad.trace_target(T(s["rif"]), p, v, t, s["h"], s["ds"])
    L = (xt * T(s["dx"])).sum() + (vt * T(s["dv"])).sum() + (d2 * T(s["dd2"])).sum()
    gp, gv, gt = torch.autograd.grad(L, (p, v, t))
    return xt.detach().numpy(), vt.detach().numpy(), d2.detach().numpy(), j.numpy(), gp.numpy(), gv.numpy(), gt.numpy()


_ad64 = {}


def referee(case):
    if case not in _ad64:
        _ad64[case] = autograd64(_case(case))
    return _ad64[case]


def tie_free_rays(r, ref):
    x64, v64, _, j64 = ref[:4]
    return (j64 == r["jstar"].astype(np.int64)) & (np.abs(x64 - r["xt"]).max(1) <= TIE_TOL) & \
        (np.abs(v64 - r["vt"]).max(1) <= TIE_TOL)


# ---- CPU tier -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,zero", CASES)
def test_host_routine_matches_float64_autograd(name, zero):
    case = f"{name}/{zero}"
    s, r, ref = _case(case), host(case), referee(case)
    tie_free = tie_free_rays(r, ref)
    dropped = 1.0 - tie_free.mean()
    err = rel_err(r["dpos"], r["dvel"], ref[4], ref[5])
    kinds = record_kinds(s, r)
    print(f"{case}: {len(tie_free)} rays, {r['n_failed']} failed, global loop {r['iters']}; dropped as not tie-free "
          f"{100 * dropped:.2f} %; tie-free by record kind " + ", ".join(f"{k} {int((m & tie_free).sum())}" for k, m in kinds.items())
          + f"; rel err max {err[tie_free].max():.3e} median {np.median(err[tie_free]):.3e}")
    assert dropped <= MAX_DROPPED
    assert err[tie_free].max() <= GRAD_TOL
    for kind, m in kinds.items():
        assert (m & tie_free).sum() >= 10, kind
    for lab in ENTERING:
        assert (kinds["after"] & tie_free & (s["labels"] == lab)).sum() >= 10, lab
    # a ray that ran out of steps keeps its record and its gradient: reported in the statistics only
    if zero == "zero":
        assert r["n_failed"] > 0 and r["iters"] == stop_ad._max_steps(4.0, s["h"], s["rif"].shape, s["ds"])
        assert (tie_free & r["failed"]).sum() >= 10          # compared above like every other ray
    else:
        # the global loop is the slowest ray's: below the step bound unless a ray of the other sets ran out of steps (one
        # does at the multi-cell step on the lens)
        assert r["iters"] == r["fwd"].max() and r["n_failed"] <= 1
        assert r["n_failed"] or r["iters"] < stop_ad._max_steps(4.0, s["h"], s["rif"].shape, s["ds"])


@pytest.mark.parametrize("case", [f"{n}/{z}" for n, z in CASES] + [f"fuzz{k}" for k in range(6)])
def test_replay_is_the_forward_march(case):
    """The routine's replayed record and global loop count == the product's target_ray_a + target_ray_b (tests/hostcheck),
    bit for bit, NaN in the same places; a record that is the input, with no seed on dist2, gives (dx, dv) bit for bit."""
    s, r = _case(case), host(case)
    k = HC.trace_target(s["rif"], s["res"], s["pos"], s["vel"], s["tg"], s["h"], s["ds"])
    for key in ("xt", "vt", "dist2"):
        assert np.array_equal(r[key], k[key], equal_nan=True), key
        assert np.array_equal(np.isnan(r[key]), np.isnan(k[key])), key
    assert r["iters"] == k["iters"] == r["fwd"].max()
    assert r["ray_steps"] == int(r["steps"].astype(np.int64).sum()) and (r["steps"] >= r["fwd"]).all()
    moved = (r["xt"] != s["pos"]).any(1) | (r["vt"] != s["vel"]).any(1)
    assert (r["jstar"][moved] > 0).all()
    r0 = host(case, dd2=False)
    for key in ("xt", "vt", "dist2", "jstar", "fwd", "steps", "failed"):
        assert np.array_equal(r0[key], r[key], equal_nan=True), key
    z = r0["jstar"] == 0
    assert z.sum() >= 10
    assert np.array_equal(r0["dpos"][z].view(np.uint32), s["dx"][z].view(np.uint32))
    assert np.array_equal(r0["dvel"][z].view(np.uint32), s["dv"][z].view(np.uint32))
    # with the seed: (gx, dv), gx = dx + 2 dd2 (x_j - t) with one rounding
    pull = 2.0 * s["dd2"].astype(np.float64)[:, None] * (r["xt"].astype(np.float64) - s["tg"])
    gx = s["dx"] + pull
    fin = z & np.isfinite(gx).all(1)
    assert (np.abs(r["dpos"] - gx)[fin] <= 2.4e-7 * (np.abs(s["dx"]) + np.abs(pull))[fin]).all()      # two fp32 roundings
    assert np.array_equal(r["dvel"][z].view(np.uint32), s["dv"][z].view(np.uint32))


def test_uniform_medium_closed_form():
    """rif = 1 (no refraction anywhere), target k steps straight ahead: the record is iteration k, dpos = gx and
    dvel = dv + k ds gx -- through the prefix (a start outside), the sampled run and the flight after the escape, in one call
    whose slowest ray keeps the global loop running.  A handful of fp32 roundings: rtol 1e-6."""
    res, h, ds = (8, 9, 7), 1.0, 0.5
    rif = np.ones((res[2], res[1], res[0]), np.float32)
    starts = [((3.2, 1.1, 3.3), (0.1, 1.0, 0.05)), ((3.2, -1.3, 3.3), (0.1, 1.0, 0.05)), ((2.6, 3.1, 4.2), (-0.7, 0.2, 0.6))]
    ks = (1, 2, 3, 5, 9, 13, 17, 22, 30)
    pos = np.array([p for p, _ in starts for _ in ks] + [(4.0, 4.0, 3.0)], np.float32)
    vel = np.array([v for _, v in starts for _ in ks] + [(0.0, 0.15, 0.0)], np.float32)      # the slow ray: 54 of 72 iterations
    k = np.array([k for _ in starts for k in ks] + [4])
    tg = (pos.astype(np.float64) + (k * ds)[:, None] * vel).astype(np.float32)
    n = len(pos)
    dx = np.tile(np.array([[0.3, -1.2, 0.7]], np.float32), (n, 1)); dv = np.tile(np.array([[-0.4, 0.9, 0.2]], np.float32), (n, 1))
    dd2 = np.full(n, 0.8, np.float32)
    r = TH.backtrace_target_rays(rif, res, pos, vel, tg, dx, dv, h, ds, ddist2=dd2)
    assert r["iters"] > max(ks) and not r["failed"].any()
    assert np.array_equal(r["jstar"], k)
    after = r["jstar"] > r["fwd"]
    assert after.sum() >= 6 and (~after).sum() >= 6 and (r["jstar"][9:18] <= 2).sum() >= 2      # row 2 starts outside
    gx = dx + 2.0 * dd2.astype(np.float64)[:, None] * (r["xt"].astype(np.float64) - tg)
    np.testing.assert_allclose(r["dpos"], gx, rtol=1e-6)
    np.testing.assert_allclose(r["dvel"], dv + (k * ds)[:, None] * gx, rtol=1e-6)


def test_one_iteration_closed_form():
    """j = 1 from an in-bounds start on the unit-scale lens (as test_stop_raygrad.test_one_iteration_closed_form):
    dvel = dv + ds gx, dpos = gx + ds J(x0)^T dvel, J = d(n grad n)/dx at x0 by float64 autograd of the comparator's sampler."""
    rif = cases.luneburg(16)
    h, res = 1.0 / 15.0, (16, 16, 16)
    ds = h / 2
    dx = np.array([[0.3, -1.2, 0.7]], np.float32); dv = np.array([[-0.4, 0.9, 0.2]], np.float32)
    dd2 = np.array([0.8], np.float32)
    pos = np.array([[3.3, 9.4, 11.2]], np.float32) * np.float32(h); vel = np.array([[0.1, 1.0, -0.05]], np.float32)
    tg = (pos + np.float32(ds) * vel + np.array([[0.2, 0.0, -0.1]], np.float32) * np.float32(ds)).astype(np.float32)
    r = TH.backtrace_target_rays(rif, res, pos, vel, tg, dx, dv, h, ds, ddist2=dd2)
    assert r["jstar"][0] == 1 and r["fwd"][0] > 1 and r["steps"][0] == r["fwd"][0] + 1 and r["iters"] == r["fwd"][0]
    R = torch.tensor(rif, dtype=torch.float64)
    J = torch.autograd.functional.jacobian(lambda y: stop_ad.n_grad_n(R, y, h), torch.tensor(pos[0], dtype=torch.float64)).numpy()
    assert np.abs(J).max() > 0.5
    gx = dx[0] + 2.0 * float(dd2[0]) * (r["xt"][0].astype(np.float64) - tg[0])
    assert np.abs(gx - dx[0]).max() > 1e-3
    mu = dv[0].astype(np.float64) + ds * gx
    np.testing.assert_allclose(r["dvel"][0], mu, rtol=1e-6)
    np.testing.assert_allclose(r["dpos"][0], gx + ds * J.T @ mu, rtol=1e-5, atol=1e-6)


def test_abi_and_python_surface():
    """The C symbol is exported and bound, the profile id is appended, and the class exists next to the Back class."""
    from adjointnonlinearraytracing_amd import _lib, drrt, tracer
    lib = C.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "drrt_backtrace_target_rays_f32") and "drrt_backtrace_target_rays_f32" in _lib.SIGNATURES
    assert _lib.PROF_NAMES[10] == "backtrace_target_rays"
    assert _lib.PROF_NAMES[8] == "backtrace_pln_rays" and _lib.PROF_NAMES[9] == "backtrace_sdf_rays"
    assert callable(drrt.TracerC.backtrace_target_rays)
    assert issubclass(tracer.ADRayTargetTracerC, torch.autograd.Function)
    assert tracer.ADRayTargetTracerC is not tracer.BackTargetTracerC
    with open(os.path.join(os.path.dirname(_lib.LIB_PATH), "..", "include", "drrt_hip.h")) as f:
        hdr = f.read()
    assert "drrt_backtrace_target_rays_f32" in hdr and "#define DRRT_PROF_BACKTRACE_TARGET_RAYS 10" in hdr


def test_abi_argument_checks():
    """Null pointers, a bad resolution, bad steps and a missing workspace are refused before anything is launched."""
    from adjointnonlinearraytracing_amd import _lib
    lib = _lib.load()
    rif = np.ones(8 * 8 * 8, np.float32)
    a = np.zeros((4, 3), np.float32)
    ws = np.zeros(4096, np.uint8)
    P = lambda x: C.c_void_p(x.ctypes.data) if x is not None else None    # noqa: E731 (host pointers: never launched)

    def call(rif_=rif, nvox=rif.size, res=(8, 8, 8), n=4, pos=a, tg=a, dx=a, dd2=None, dpos=a, dvel=a, h=1.0, ds=0.5, ws_=ws):
        return lib.drrt_backtrace_target_rays_f32(P(rif_), nvox, (C.c_int * 3)(*res), n, P(pos), P(a), P(tg), P(dx), P(a),
                                                  P(dd2), h, ds, P(dpos), P(dvel), None, P(ws_),
                                                  0 if ws_ is None else ws_.size, 0, None)
    for kw, rc, msg in ((dict(rif_=None), _lib.ERR_ARG, "null rif"), (dict(res=(8, 8, 7)), _lib.ERR_RES_MISMATCH, "Resolution"),
                        (dict(res=(1, 8, 64)), _lib.ERR_BAD_RES, "invalid resolution"), (dict(h=0.0), _lib.ERR_ARG, "positive"),
                        (dict(h=float("nan")), _lib.ERR_ARG, "positive"), (dict(ds=-1.0), _lib.ERR_ARG, "positive"),
                        (dict(ds=float("inf")), _lib.ERR_ARG, "positive"), (dict(pos=None), _lib.ERR_ARG, "null ray"),
                        (dict(tg=None), _lib.ERR_ARG, "null ray"), (dict(dx=None), _lib.ERR_ARG, "null ray"),
                        (dict(dpos=None), _lib.ERR_ARG, "dpos"), (dict(dvel=None), _lib.ERR_ARG, "dpos"),
                        (dict(n=1 << 33), _lib.ERR_ARG, "uint32"), (dict(ws_=None), _lib.ERR_ARG, "workspace"),
                        (dict(ws_=np.zeros(64, np.uint8)), _lib.ERR_ARG, "workspace")):
        assert call(**kw) == rc, kw
        assert msg in _lib.last_error(), (kw, _lib.last_error())
    assert call(n=0, ws_=None) == 0 and _lib.last_error() == ""       # a valid call clears the message


def test_routine_under_sanitizers(tmp_path):
    """tests/hostcheck/target_rays.hip as a stand-alone program (its own main), compiled for the host with ASan + UBSan and run
    as a child process, nothing preloaded: a fuzz case with NaN, Inf, huge and zero-velocity rays, targets and seeds."""
    exe = HC.sanitized_program(tmp_path, TH.SOURCE, "TARGET_RAYS_MAIN")
    s = fuzz_scene(3)
    n = len(s["pos"])
    rng = np.random.default_rng(0)
    arrs = {k: s[k].copy() for k in ("pos", "vel", "tg", "dx", "dv")}
    bad = np.array([np.nan, np.inf, -np.inf, 3e38, -3e38, 1e30, 1e-40, 0.0], np.float32)
    for a in arrs.values():
        a[rng.integers(0, n, 40), rng.integers(0, 3, 40)] = rng.choice(bad, 40)
    arrs["vel"][rng.integers(0, n, 20)] = 0.0
    dd2 = s["dd2"].copy()
    dd2[rng.integers(0, n, 20)] = rng.choice(bad, 20)
    path = str(tmp_path / "case.bin")
    HC.write_case(path, list(s["res"]) + [n], [s["h"], s["ds"]],
                  [s["rif"]] + [arrs[k] for k in ("pos", "vel", "tg", "dx", "dv")] + [dd2])
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "finished without reports" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
    assert f"{n} rays" in r.stdout


# ---- GPU tier -------------------------------------------------------------------------------------------------------
def _gpu_call(T, s, dev, order=None, dd2=True):
    return T.backtrace_target_rays(_t(s["rif"], dev), s["res"], _t(s["pos"], dev), _t(s["vel"], dev), _t(s["tg"], dev),
                                   _t(s["dx"], dev), _t(s["dv"], dev), s["h"], s["ds"],
                                   ddist2=_t(s["dd2"], dev) if dd2 else None, order=order)


def _raw_call(lib, drrt, s, dev, pair, hint):
    """The C entry point itself with DRRT_FLAG_SORT_RAYS | DRRT_FLAG_DISPATCH_IN_ORDER (block order = visit order)."""
    _lib = drrt._lib
    rif, pos, vel, tg, dx, dv, dd2 = (_t(np.ascontiguousarray(s[k], np.float32), dev)
                                      for k in ("rif", "pos", "vel", "tg", "dx", "dv", "dd2"))
    n = pos.shape[0]
    fl = _lib.FLAG_SORT_RAYS | _lib.FLAG_DISPATCH_IN_ORDER | (_lib.FLAG_PAIR_GRID if pair else 0)
    ws = torch.empty(int(lib.drrt_workspace_bytes_grid(n, rif.numel(), fl)) + 256, dtype=torch.uint8, device=dev)
    st = torch.zeros(3, dtype=torch.int64, device=dev)
    dpos, dvel = torch.empty_like(pos), torch.empty_like(vel)
    p = lambda t: C.c_void_p(t.data_ptr())     # noqa: E731
    if hint is not None:
        lib.drrt_set_order_hint(p(hint), n)
    rc = lib.drrt_backtrace_target_rays_f32(p(rif), rif.numel(), (C.c_int * 3)(*s["res"]), n, p(pos), p(vel), p(tg), p(dx), p(dv),
                                            p(dd2), float(s["h"]), float(s["ds"]), p(dpos), p(dvel), p(st), p(ws), ws.numel(),
                                            fl, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    _lib.check(rc)
    torch.cuda.synchronize(dev)
    return dpos, dvel, drrt.read_stats(st)


def _same(got, want):
    got = got.cpu().numpy()
    return np.array_equal(np.isfinite(got), np.isfinite(want)) and np.array_equal(got, want, equal_nan=True)


@pytest.mark.gpu
@pytest.mark.parametrize("case", [f"{n}/{z}" for n, z in CASES] + [f"fuzz{k}" for k in range(5)])
def test_kernels_match_host_routine_bitwise(gpu, case):
    """Both target launches of drrt_ray_adjoints.hip == the host build, bit for bit (non-finite values in the same places), with the
    same statistics: plain and pair-copy gathers, with the forward's visit order, its own sort and none, XCD dispatch order
    on and off.  The forward kernel's record is the one the routine replayed."""
    from adjointnonlinearraytracing_amd import drrt
    s, r = _case(case), host(case)
    T = drrt.TracerC()
    xt, vt, d2 = T.trace_target(_t(s["rif"], gpu), s["res"], _t(s["pos"], gpu), _t(s["vel"], gpu), _t(s["tg"], gpu), s["h"], s["ds"])
    fwd = drrt.read_stats()
    order = drrt.keep_order(drrt.last_order)
    assert order is not None
    assert _same(xt, r["xt"]) and _same(vt, r["vt"]) and _same(d2, r["dist2"])
    assert fwd["iters"] == r["iters"] and fwd["n_failed"] == r["n_failed"]
    lib = drrt._lib.load()
    runs = 0
    for pair in (False, True):
        for sort, hint in ((False, None), (True, None), (True, order)):
            for in_order in ((False, True) if sort else (False,)):
                with drrt.using(pair_grid=pair, sort_rays=sort):
                    if in_order:               # DRRT_FLAG_DISPATCH_IN_ORDER has no option of its own: through the C ABI
                        dpos, dvel, st = _raw_call(lib, drrt, s, gpu, pair, hint)
                    else:
                        dpos, dvel = _gpu_call(T, s, gpu, order=hint)
                        st = drrt.read_stats()
                tag = (pair, sort, hint is not None, in_order)
                assert _same(dpos, r["dpos"]) and _same(dvel, r["dvel"]), tag
                assert st["ray_steps"] == r["ray_steps"] and st["iters"] == r["iters"] and st["n_failed"] == r["n_failed"], tag
                runs += 1
    assert runs == 10
    if case == "%s/%s" % CASES[0]:             # without the seed on dist2 (a null pointer)
        r0 = host(case, dd2=False)
        dpos, dvel = _gpu_call(T, s, gpu, dd2=False)
        assert _same(dpos, r0["dpos"]) and _same(dvel, r0["dvel"]) and not np.array_equal(r0["dpos"], r["dpos"])


@pytest.mark.gpu
def test_single_ray(gpu):
    """n = 1: the global loop count is the ray's own, nothing is sorted."""
    from adjointnonlinearraytracing_amd import drrt
    s = target_scene("lens16_h1_half", "nozero")
    r = host("lens16_h1_half/nozero")
    i = int(np.where((r["jstar"] > 0) & (r["jstar"] <= r["fwd"]) & (s["labels"] == "inside"))[0][0])
    one = dict(s, **{k: s[k][i:i + 1] for k in ("pos", "vel", "tg", "dx", "dv", "dd2")})
    r1 = TH.backtrace_target_rays(one["rif"], one["res"], one["pos"], one["vel"], one["tg"], one["dx"], one["dv"], one["h"],
                                  one["ds"], ddist2=one["dd2"])
    assert r1["iters"] == r1["fwd"][0] and r1["jstar"][0] > 0
    dpos, dvel = _gpu_call(drrt.TracerC(), one, gpu)
    st = drrt.read_stats()
    assert _same(dpos, r1["dpos"]) and _same(dvel, r1["dvel"])
    assert st["ray_steps"] == r1["ray_steps"] and st["iters"] == r1["iters"] and st["n_failed"] == 0


CUBE = "lens16_h1_half/nozero"


def _cube_case(n=64):
    """64 rays (one wave: the dL/dn adjoint's summation order is fixed) on the cubic lens, 16 of each record kind;
    tracer.* pass rif.shape as res."""
    s, r = _case(CUBE), host(CUBE)
    tie_free = tie_free_rays(r, referee(CUBE))
    rng = np.random.default_rng(0)
    sel = np.concatenate([rng.choice(np.where(m & tie_free)[0], n // 4, replace=False) for m in record_kinds(s, r).values()])
    return dict(s, **{k: s[k][sel] for k in ("pos", "vel", "tg", "dx", "dv", "dd2")}), sel


def _ad_grads(cls, s, dev, rif_grad=True, x_grad=False, v_grad=False, sp_grad=False, dist2=True, dtype=torch.float32):
    """cls.apply -> L = <dx, xt> + <dv, vt> [+ <dd2, dist2>] -> backward -> (rif.grad, x.grad, v.grad, sp.grad, xt)."""
    rif = _t(s["rif"], dev).requires_grad_(rif_grad)
    x = _t(s["pos"], dev).to(dtype).requires_grad_(x_grad)
    v = _t(s["vel"], dev).requires_grad_(v_grad)
    sp = _t(s["tg"], dev).requires_grad_(sp_grad)
    xt, vt, d2 = cls.apply(rif, x, v, sp, s["h"], s["ds"])
    loss = (xt * _t(s["dx"], dev)).sum() + (vt * _t(s["dv"], dev)).sum()
    if dist2:
        loss = loss + (d2 * _t(s["dd2"], dev)).sum()
    loss.backward()
    torch.cuda.synchronize()
    return rif.grad, x.grad, v.grad, sp.grad, xt.detach()


@pytest.mark.gpu
def test_adray_target_tracer_end_to_end(gpu):
    """ADRayTargetTracerC.apply -> loss on all three outputs -> backward: x.grad, v.grad are the direct call's for the four
    requires_grad combinations (None where not asked); rif.grad is BackTargetTracerC's bit for bit without dist2 in the loss
    and TracerC.backtrace's from the effective seed with it; sp.grad = -2 g (xt - sp)."""
    from adjointnonlinearraytracing_amd import drrt, tracer
    s, _ = _cube_case()
    T = drrt.TracerC()
    back, ad = tracer.BackTargetTracerC, tracer.ADRayTargetTracerC
    dpos, dvel = _gpu_call(T, s, gpu)
    dpos0, dvel0 = _gpu_call(T, s, gpu, dd2=False)
    assert float(dpos.abs().sum()) > 0 and bool((dpos != dpos0).any()) and bool((dpos0 != _t(s["dx"], gpu)).any())
    g_back, gx, gv = grads(lambda rif, x, v: back.apply(rif, x, v, _t(s["tg"], gpu), s["h"], s["ds"])[:2], s, gpu, True, True, True)
    assert gx is None and gv is None and float(g_back.abs().sum()) > 0
    # the documented effective seed, through the generic backtrace from the record
    rif_d, sp = _t(s["rif"], gpu), _t(s["tg"], gpu)
    xt, vt, _ = T.trace_target(rif_d, s["res"], _t(s["pos"], gpu), _t(s["vel"], gpu), sp, s["h"], s["ds"])
    order = drrt.keep_order(drrt.last_order)
    g = _t(s["dd2"], gpu)
    seed = _t(s["dx"], gpu) + (2 * g)[:, None] * (xt - sp)
    g_seed = T.backtrace(rif_d, s["res"], xt, vt, seed, _t(s["dv"], gpu), s["h"], s["ds"], order=order).reshape(rif_d.shape)
    assert not torch.equal(g_seed, g_back)
    for xg, vg in ((False, False), (True, False), (False, True), (True, True)):
        grif, gx, gv, gsp, _ = _ad_grads(ad, s, gpu, True, xg, vg, dist2=False)
        assert torch.equal(grif, g_back) and gsp is None, (xg, vg)
        assert (gx is not None) == xg and (gv is not None) == vg
        assert (gx is None or torch.equal(gx, dpos0)) and (gv is None or torch.equal(gv, dvel0))
        grif, gx, gv, gsp, _ = _ad_grads(ad, s, gpu, True, xg, vg)
        assert torch.equal(grif, g_seed) and gsp is None, (xg, vg)
        assert (gx is not None) == xg and (gv is not None) == vg
        assert (gx is None or torch.equal(gx, dpos)) and (gv is None or torch.equal(gv, dvel))
    grif, gx, gv, gsp, xt_ad = _ad_grads(ad, s, gpu, False, True, True, sp_grad=True)
    assert grif is None and torch.equal(gx, dpos) and torch.equal(gv, dvel) and torch.equal(xt_ad, xt)
    # dL/dsp: three fp32 roundings away from the float64 value of -2 g (xt - sp) at the call's own xt ...
    want = -2.0 * s["dd2"].astype(np.float64)[:, None] * (xt.cpu().numpy().astype(np.float64) - s["tg"])
    np.testing.assert_allclose(gsp.cpu().numpy(), want, rtol=1e-6, atol=1e-30)
    # ... and float64 autograd's on the tie-free rays of THIS call (its global loop count is that of its own 64 rays)
    ref = autograd64(s)
    r = TH.backtrace_target_rays(s["rif"], s["res"], s["pos"], s["vel"], s["tg"], s["dx"], s["dv"], s["h"], s["ds"], ddist2=s["dd2"])
    assert np.array_equal(xt.cpu().numpy(), r["xt"])
    tie_free = tie_free_rays(r, ref)
    err = np.linalg.norm(gsp.cpu().numpy() - ref[6], axis=1) / np.maximum(np.linalg.norm(ref[6], axis=1), 1e-30)
    print(f"dL/dsp: {int(tie_free.sum())} of {len(err)} rays tie-free, rel err max {err[tie_free].max():.3e}")
    assert tie_free.sum() >= 48 and err[tie_free].max() <= GRAD_TOL and np.abs(ref[6][tie_free]).max() > 0.1
    with pytest.raises(RuntimeError, match="float32"):
        _ad_grads(ad, s, gpu, True, True, False, dtype=torch.float64)


@pytest.mark.gpu
def test_adray_target_tracer_launches(gpu):
    """No ray-gradient kernel without a ray input requiring grad (then the launches are the Back class's); no dL/dn adjoint
    with rif frozen; no adjoint launch at all when only sp requires grad.  The lists are those of the sibling tests
    (["trace", "backtrace"], ["trace", "backtrace_target_rays"]) with the forward's part as the forward itself records it:
    drrt_trace_target_f32 has never taken a profile record (tests/golden/python_calls.json pins its launches), so that part
    is empty."""
    from adjointnonlinearraytracing_amd import _lib, drrt, tracer
    s, _ = _cube_case()
    back, ad = tracer.BackTargetTracerC, tracer.ADRayTargetTracerC
    lib = _lib.load()

    def collect(fn):
        lib.drrt_profile_begin(256)
        try:
            fn()
            torch.cuda.synchronize()
            # the march launches; the sort, the zero-fill and the pair copy are bookkeeping of whichever call needs them
            return [name for name, _ in _lib.profile_collect() if name not in ("sort", "zero", "quad")]
        finally:
            lib.drrt_profile_end()
    fwd = collect(lambda: drrt.TracerC().trace_target(_t(s["rif"], gpu), s["res"], _t(s["pos"], gpu), _t(s["vel"], gpu),
                                                      _t(s["tg"], gpu), s["h"], s["ds"]))
    assert fwd in ([], ["trace"])
    b = collect(lambda: grads(lambda rif, x, v: back.apply(rif, x, v, _t(s["tg"], gpu), s["h"], s["ds"])[:2], s, gpu))
    assert b == fwd + ["backtrace"]
    assert collect(lambda: _ad_grads(ad, s, gpu)) == b
    assert collect(lambda: _ad_grads(ad, s, gpu, sp_grad=True)) == b
    assert collect(lambda: _ad_grads(ad, s, gpu, rif_grad=False, x_grad=True, v_grad=True)) == fwd + ["backtrace_target_rays"]
    assert collect(lambda: _ad_grads(ad, s, gpu, rif_grad=False, sp_grad=True)) == fwd
    assert sorted(collect(lambda: _ad_grads(ad, s, gpu, v_grad=True))) == sorted(fwd + ["backtrace", "backtrace_target_rays"])
