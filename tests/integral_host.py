"""Loader for tests/hostcheck/integral_rays.hip (TEST INFRASTRUCTURE ONLY): the product's per-ray routines of the grid
integral family -- optical path length (trace_opl_ray, opl_backtrace_ray), line integral of a second field (trace_field_ray,
field_backtrace_ray), emission with self-absorption (exp_neg, trace_emission_ray, emission_backtrace_ray), line integral of
a vector field (trace_vector_ray, vector_backtrace_ray) and ray paths without and with the velocity series (trace_path_ray,
path_backtrace_ray; trace_phase_ray, phase_backtrace_ray) of csrc/drrt_device.h -- compiled for the host by
hostcheck_lib.build(), looped as the kernels run them.  Never imported by the package."""
import ctypes as C
import os

import numpy as np

from hostcheck_lib import HOSTCHECK, _f, _p, _res, build

SOURCE = os.path.join(HOSTCHECK, "integral_rays.hip")
_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = build("libintegral_rays.so", [SOURCE])
    return _lib


def _trace(entry, grids, res, pos, vel, h, ds, names, ints=(), more=()):
    """entry(grids..., res, n, pos, vel, h, ds, ints..., xt, vt, <an fp32 per ray for each of names>, more..., steps,
    &n_failed) -> dict(xt, vt, <names>, steps, n_failed)"""
    n = len(pos)
    xt, vt, steps, nf = np.empty_like(pos), np.empty_like(vel), np.empty(n, np.uint32), C.c_longlong(0)
    out = {k: np.empty(n, np.float32) for k in names}
    rc = getattr(lib(), entry)(*map(_p, grids), _p(_res(res)), C.c_size_t(n), _p(pos), _p(vel), C.c_float(h), C.c_float(ds),
                               *map(C.c_int, ints), _p(xt), _p(vt), *map(_p, out.values()), *map(_p, more), _p(steps),
                               C.byref(nf))
    assert rc == 0
    return dict(xt=xt, vt=vt, **out, steps=steps, n_failed=int(nf.value))


def _backtrace(entry, grids, res, rays, steps, more, seeds, h, ds, flags, grads):
    """entry(grids..., res, n, pos, vel, xt, vt, steps, more..., seeds... (nullable), h, ds, flags..., grads..., dpos, dvel,
    rsteps, failed), `grads` being {name: size} of the float64 sums -> dict(<grads>, dpos, dvel, steps (reverse iterations
    per ray), failed, ray_steps, n_failed)"""
    pos, vel, xt, vt = rays
    seeds = [None if a is None else _f(a) for a in seeds]
    steps = np.ascontiguousarray(np.asarray(steps).astype(np.uint32))
    n = len(pos)
    grads = {k: np.empty(size, np.float64) for k, size in grads.items()}
    dpos, dvel = np.empty_like(pos), np.empty_like(vel)
    rsteps, failed = np.empty(n, np.uint32), np.empty(n, np.uint8)
    rc = getattr(lib(), entry)(*map(_p, grids), _p(_res(res)), C.c_size_t(n), _p(pos), _p(vel), _p(xt), _p(vt), _p(steps),
                               *map(_p, more), *map(_p, seeds), C.c_float(h), C.c_float(ds), *map(C.c_int, flags),
                               *map(_p, grads.values()), _p(dpos), _p(dvel), _p(rsteps), _p(failed))
    assert rc == 0
    failed = failed.astype(bool)
    return dict(**grads, dpos=dpos, dvel=dvel, steps=rsteps, failed=failed,
                ray_steps=int(rsteps.astype(np.int64).sum()), n_failed=int(failed.sum()))


def _grids(rif, *further, what="every further grid must have rif's shape", lead=()):
    rif, further = _f(rif), [_f(a) for a in further]
    assert all(a.shape == tuple(lead) + rif.shape for a in further), what
    return [a.reshape(-1) for a in [rif] + further]


def trace_opl(rif, res, pos, vel, h, ds):
    """-> dict(xt, vt, opl, steps, n_failed): the host build of what drrt_trace_opl_f32 computes."""
    return _trace("opl_host_trace", _grids(rif), res, _f(pos), _f(vel), h, ds, ("opl",))


def backtrace_opl(rif, res, pos, vel, xt, vt, steps, dx, dv, dopl, h, ds, corrected_h=True, parts=0):
    """-> dict(grad float64[nvox], dpos, dvel, steps (reverse iterations per ray), failed, ray_steps, n_failed): the host
    build of what drrt_backtrace_opl_f32 computes; dx, dv, dopl may be None (zeros).  `parts`: 0 = the whole grid gradient,
    1 = the value weights of every contribution alone, 2 = their gradient splats alone."""
    g = _grids(rif)
    return _backtrace("opl_host_backtrace", g, res, [_f(a) for a in (pos, vel, xt, vt)], steps, (), (dx, dv, dopl), h, ds,
                      (bool(corrected_h), parts), dict(grad=g[0].size))


def trace_field(rif, field, res, pos, vel, h, ds):
    """-> dict(xt, vt, tau, steps, n_failed): the host build of what drrt_trace_field_f32 computes."""
    return _trace("field_host_trace", _grids(rif, field, what="field must have rif's shape"), res, _f(pos), _f(vel), h, ds,
                  ("tau",))


def backtrace_field(rif, field, res, pos, vel, xt, vt, steps, dx, dv, dtau, h, ds, corrected_h=True, parts=0):
    """-> dict(grad, grad_field (float64[nvox] each), dpos, dvel, steps (reverse iterations per ray), failed, ray_steps,
    n_failed): the host build of what drrt_backtrace_field_f32 computes; dx, dv, dtau may be None (zeros).  `parts`: 0 = the
    whole gradients, 1 = the value weights of every contribution alone, 2 = their gradient splats alone (dL/dfield has
    none)."""
    g = _grids(rif, field, what="field must have rif's shape")
    return _backtrace("field_host_backtrace", g, res, [_f(a) for a in (pos, vel, xt, vt)], steps, (), (dx, dv, dtau), h, ds,
                      (bool(corrected_h), parts), dict(grad=g[0].size, grad_field=g[0].size))


def exp_neg(t):
    """The product's exp_neg on every entry of `t` (fp32)."""
    t = np.ascontiguousarray(np.asarray(t, np.float32).reshape(-1))
    out = np.empty_like(t)
    assert lib().emission_host_exp_neg(_p(t), C.c_size_t(t.size), _p(out)) == 0
    return out


def trace_emission(rif, emis, absb, res, pos, vel, h, ds):
    """-> dict(xt, vt, rad, tau, steps, n_failed): the host build of what drrt_trace_emission_f32 computes."""
    g = _grids(rif, emis, absb, what="emission and absorption must have rif's shape")
    return _trace("emission_host_trace", g, res, _f(pos), _f(vel), h, ds, ("rad", "tau"))


def backtrace_emission(rif, emis, absb, res, pos, vel, xt, vt, steps, tau, dx, dv, drad, dtau, h, ds, corrected_h=True,
                       parts=0):
    """-> dict(grad, grad_emission, grad_absorption (float64[nvox] each), dpos, dvel, steps (reverse iterations per ray),
    failed, ray_steps, n_failed): the host build of what drrt_backtrace_emission_f32 computes; dx, dv, drad, dtau may be None
    (zeros).  `parts`: 0 = the whole gradients, 1 = the value weights of every contribution alone, 2 = their gradient splats
    alone (dL/de and dL/da have none)."""
    g = _grids(rif, emis, absb, what="emission and absorption must have rif's shape")
    return _backtrace("emission_host_backtrace", g, res, [_f(a) for a in (pos, vel, xt, vt)], steps, (_f(tau),),
                      (dx, dv, drad, dtau), h, ds, (bool(corrected_h), parts),
                      dict(grad=g[0].size, grad_emission=g[0].size, grad_absorption=g[0].size))


def trace_vector(rif, vfield, res, pos, vel, h, ds):
    """-> dict(xt, vt, circ, steps, n_failed): the host build of what drrt_trace_vector_f32 computes."""
    g = _grids(rif, vfield, what="vfield must have shape (3,) + rif.shape", lead=(3,))
    return _trace("vector_host_trace", g, res, _f(pos), _f(vel), h, ds, ("circ",))


def backtrace_vector(rif, vfield, res, pos, vel, xt, vt, steps, dx, dv, dcirc, h, ds, corrected_h=True, parts=0):
    """-> dict(grad float64[nvox], grad_vfield float64[3 nvox], dpos, dvel, steps (reverse iterations per ray), failed,
    ray_steps, n_failed): the host build of what drrt_backtrace_vector_f32 computes; dx, dv, dcirc may be None (zeros).
    `parts`: 0 = the whole gradients, 1 = the value weights of every contribution alone, 2 = their gradient splats alone
    (dL/du has none)."""
    g = _grids(rif, vfield, what="vfield must have shape (3,) + rif.shape", lead=(3,))
    return _backtrace("vector_host_backtrace", g, res, [_f(a) for a in (pos, vel, xt, vt)], steps, (), (dx, dv, dcirc), h, ds,
                      (bool(corrected_h), parts), dict(grad=g[0].size, grad_vfield=3 * g[0].size))


def _trace_series(entry, names, rif, res, pos, vel, h, ds, stride, samples):
    pos, vel = _f(pos).reshape(-1, 3), _f(vel).reshape(-1, 3)
    series = {k: np.empty((samples, len(pos), 3), np.float32) for k in names}
    count = np.empty(len(pos), np.int32)
    r = _trace(entry, _grids(rif), res, pos, vel, h, ds, (), (stride, samples), (*series.values(), count))
    return dict(xt=r["xt"], vt=r["vt"], **series, count=count, steps=r["steps"], n_failed=r["n_failed"])


def _backtrace_series(entry, rif, res, pos, vel, xt, vt, steps, dx, dv, series, h, ds, stride, samples, corrected_h):
    g = _grids(rif)
    rays = [_f(a).reshape(-1, 3) for a in (pos, vel, xt, vt)]
    assert all(a is None or _f(a).shape == (samples, len(rays[0]), 3) for a in series)
    return _backtrace(entry, g, res, rays, steps, (), (dx, dv, *series), h, ds, (stride, samples, bool(corrected_h)),
                      dict(grad=g[0].size))


def trace_path(rif, res, pos, vel, h, ds, stride, samples):
    """-> dict(xt, vt, path (samples, n, 3), count, steps, n_failed): the host build of what drrt_trace_path_f32 computes."""
    return _trace_series("path_host_trace", ("path",), rif, res, pos, vel, h, ds, stride, samples)


def trace_phase(rif, res, pos, vel, h, ds, stride, samples):
    """-> dict(xt, vt, path, vpath ((samples, n, 3) each), count, steps, n_failed): the host build of what
    drrt_trace_phase_f32 computes."""
    return _trace_series("phase_host_trace", ("path", "vpath"), rif, res, pos, vel, h, ds, stride, samples)


def backtrace_path(rif, res, pos, vel, xt, vt, steps, dx, dv, dpath, h, ds, stride, samples, corrected_h=True):
    """-> dict(grad float64[nvox], dpos, dvel, steps (reverse iterations per ray), failed, ray_steps, n_failed): the host
    build of what drrt_backtrace_path_f32 computes; dx, dv, dpath ((samples, n, 3)) may be None (zeros)."""
    return _backtrace_series("path_host_backtrace", rif, res, pos, vel, xt, vt, steps, dx, dv, (dpath,), h, ds, stride,
                             samples, corrected_h)


def backtrace_phase(rif, res, pos, vel, xt, vt, steps, dx, dv, dpath, dvpath, h, ds, stride, samples, corrected_h=True):
    """-> dict(grad float64[nvox], dpos, dvel, steps (reverse iterations per ray), failed, ray_steps, n_failed): the host
    build of what drrt_backtrace_phase_f32 computes; dx, dv, dpath, dvpath ((samples, n, 3)) may be None."""
    return _backtrace_series("phase_host_backtrace", rif, res, pos, vel, xt, vt, steps, dx, dv, (dpath, dvpath), h, ds,
                             stride, samples, corrected_h)
