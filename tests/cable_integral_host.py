"""Loader for tests/hostcheck/cable_integral_rays.hip (TEST INFRASTRUCTURE ONLY): the product's per-ray routines of the
fibre march with its optical path length (cable_trace_opl_ray, cable_opl_backtrace_ray of csrc/drrt_device.h) and with the
line integral of a second radial profile (cable_trace_field_ray, cable_field_backtrace_ray), compiled for the host by
hostcheck_lib.build() and looped as the kernels run them, and the kernels' LDS rule (cable_lds_bytes).  Never imported
by the package."""
import ctypes as C
import os

import numpy as np

from hostcheck_lib import HOSTCHECK, _f, _p, build

SOURCE = os.path.join(HOSTCHECK, "cable_integral_rays.hip")
_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = build("libcable_integral_rays.so", [SOURCE])
        _lib.cable_host_lds_bytes.restype = C.c_size_t
    return _lib


def max_steps(length, ds):
    """The forward's bound, (int)(4 length / ds) in fp32 (drrt_api.hip cable_begin)."""
    return int(np.float32(4.0) * np.float32(length) / np.float32(ds))


def lds_bytes(rres, nprof, ngrad):
    """cable_lds_bytes(rres, nprof, ngrad): the dynamic LDS of a cable block, 0 = global memory."""
    return int(lib().cable_host_lds_bytes(C.c_int(rres), C.c_int(nprof), C.c_int(ngrad)))


def _trace(entry, profiles, radius, length, pos, vel, target, ds, name):
    profiles = [_f(p).reshape(-1) for p in profiles]
    assert all(p.size == profiles[0].size for p in profiles)
    pos, vel, target = _f(pos), _f(vel), _f(target)
    n = len(pos)
    xt, vt = np.empty_like(pos), np.empty_like(vel)
    d2, integral = np.empty(n, np.float32), np.empty(n, np.float32)
    rec, steps, esc = np.empty(n, np.uint32), np.empty(n, np.uint32), np.empty(n, np.uint8)
    rc = getattr(lib(), entry)(*map(_p, profiles), C.c_int(profiles[0].size), C.c_float(radius), C.c_float(length),
                               C.c_size_t(n), _p(pos), _p(vel), _p(target), C.c_float(ds), _p(xt), _p(vt), _p(d2),
                               _p(integral), _p(rec), _p(steps), _p(esc))
    assert rc == 0
    return {"xt": xt, "vt": vt, "dist2": d2, name: integral, "rec_steps": rec, "steps": steps,
            "ray_steps": int(steps.astype(np.int64).sum()), "iters": int(steps.max()) if n else 0,
            "n_failed": int((esc == 0).sum())}


def _backtrace(entry, profiles, radius, length, pos, xt, vt, rec_steps, dx, dv, dint, ds, names):
    profiles = [_f(p).reshape(-1) for p in profiles]
    assert all(p.size == profiles[0].size for p in profiles)
    pos, xt, vt = _f(pos), _f(xt), _f(vt)
    dx, dv, dint = (None if a is None else _f(a) for a in (dx, dv, dint))
    rec = np.ascontiguousarray(np.asarray(rec_steps).astype(np.uint32))
    n = len(pos)
    grads = [np.empty(profiles[0].size, np.float64) for _ in profiles]
    dpos, dvel = np.empty_like(pos), np.empty_like(pos)
    rsteps, failed = np.empty(n, np.uint32), np.empty(n, np.uint8)
    rc = getattr(lib(), entry)(*map(_p, profiles), C.c_int(profiles[0].size), C.c_float(radius), C.c_float(length),
                               C.c_size_t(n), _p(pos), _p(xt), _p(vt), _p(rec), _p(dx), _p(dv), _p(dint), C.c_float(ds),
                               *map(_p, grads), _p(dpos), _p(dvel), _p(rsteps), _p(failed))
    assert rc == 0
    failed = failed.astype(bool)
    return dict(zip(names, grads), dpos=dpos, dvel=dvel, steps=rsteps, failed=failed,
                ray_steps=int(rsteps.astype(np.int64).sum()), iters=int(rsteps.max()) if n else 0, n_failed=int(failed.sum()))


def trace_cable_opl(rif, radius, length, pos, vel, target, ds):
    """-> dict(xt, vt, dist2, opl, rec_steps, steps, ray_steps, iters, n_failed): the host build of what
    drrt_trace_cable_opl_f32 computes (steps: the march's iterations per ray)."""
    return _trace("cable_opl_host_trace", (rif,), radius, length, pos, vel, target, ds, "opl")


def backtrace_cable_opl(rif, radius, length, pos, xt, vt, rec_steps, dx, dv, dopl, ds):
    """-> dict(grad float64[rres], dpos, dvel, steps (reverse iterations per ray), failed, ray_steps, iters, n_failed): the
    host build of what drrt_backtrace_cable_opl_f32 computes; dx, dv, dopl may be None (zeros)."""
    return _backtrace("cable_opl_host_backtrace", (rif,), radius, length, pos, xt, vt, rec_steps, dx, dv, dopl, ds, ("grad",))


def trace_cable_field(rif, field, radius, length, pos, vel, target, ds):
    """-> dict(xt, vt, dist2, tau, rec_steps, steps, ray_steps, iters, n_failed): the host build of what
    drrt_trace_cable_field_f32 computes (steps: the march's iterations per ray)."""
    return _trace("cable_field_host_trace", (rif, field), radius, length, pos, vel, target, ds, "tau")


def backtrace_cable_field(rif, field, radius, length, pos, xt, vt, rec_steps, dx, dv, dtau, ds):
    """-> dict(grad, grad_field (float64[rres] each), dpos, dvel, steps (reverse iterations per ray), failed, ray_steps,
    iters, n_failed): the host build of what drrt_backtrace_cable_field_f32 computes; dx, dv, dtau may be None (zeros)."""
    return _backtrace("cable_field_host_backtrace", (rif, field), radius, length, pos, xt, vt, rec_steps, dx, dv, dtau, ds,
                      ("grad", "grad_field"))
