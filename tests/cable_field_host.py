"""Loader for tests/hostcheck/cable_field_rays.hip (TEST INFRASTRUCTURE ONLY): the product's per-ray routines of the fibre
march with the line integral of a second radial profile (cable_trace_field_ray, cable_field_backtrace_ray of
csrc/drrt_device.h) compiled for the host with the line of hostcheck_lib.lib(), looped as the kernels run them.  Never
imported by the package."""
import ctypes as C
import os
import subprocess

import numpy as np

from cable_opl_host import max_steps      # noqa: F401  (the forward's bound, shared with the OPL pair)
from hostcheck_lib import _f, _p

_HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(_HERE, "hostcheck", "cable_field_rays.hip")
_HDR = os.path.join(_HERE, "..", "adjointnonlinearraytracing_amd", "csrc", "drrt_device.h")
_SO = os.path.join(_HERE, "hostcheck", "_build", "libcable_field_rays.so")
HIPCC = "/opt/rocm/bin/hipcc"
_lib = None


def lib():
    global _lib
    if _lib is None:
        os.makedirs(os.path.dirname(_SO), exist_ok=True)
        if not os.path.exists(_SO) or os.path.getmtime(_SO) < max(os.path.getmtime(f) for f in (SOURCE, _HDR)):
            subprocess.run([HIPCC, "--cuda-host-only", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-mfma", "-shared",
                            "-fvisibility=hidden", "-o", _SO, SOURCE], check=True, capture_output=True)
        _lib = C.CDLL(_SO)
    return _lib


def _profiles(rif, field):
    rif, field = _f(rif).reshape(-1), _f(field).reshape(-1)
    assert rif.size == field.size
    return rif, field


def trace_cable_field(rif, field, radius, length, pos, vel, target, ds):
    """-> dict(xt, vt, dist2, tau, rec_steps, steps, ray_steps, iters, n_failed): the host build of what
    drrt_trace_cable_field_f32 computes (steps: the march's iterations per ray)."""
    (rif, field), pos, vel, target = _profiles(rif, field), _f(pos), _f(vel), _f(target)
    n = len(pos)
    xt, vt = np.empty_like(pos), np.empty_like(vel)
    d2, tau = np.empty(n, np.float32), np.empty(n, np.float32)
    rec, steps, esc = np.empty(n, np.uint32), np.empty(n, np.uint32), np.empty(n, np.uint8)
    rc = lib().cable_field_host_trace(_p(rif), _p(field), C.c_int(rif.size), C.c_float(radius), C.c_float(length),
                                      C.c_size_t(n), _p(pos), _p(vel), _p(target), C.c_float(ds), _p(xt), _p(vt), _p(d2),
                                      _p(tau), _p(rec), _p(steps), _p(esc))
    assert rc == 0
    return dict(xt=xt, vt=vt, dist2=d2, tau=tau, rec_steps=rec, steps=steps, ray_steps=int(steps.astype(np.int64).sum()),
                iters=int(steps.max()) if n else 0, n_failed=int((esc == 0).sum()))


def backtrace_cable_field(rif, field, radius, length, pos, xt, vt, rec_steps, dx, dv, dtau, ds):
    """-> dict(grad, grad_field (float64[rres] each), dpos, dvel, steps (reverse iterations per ray), failed, ray_steps,
    iters, n_failed): the host build of what drrt_backtrace_cable_field_f32 computes; dx, dv, dtau may be None (zeros)."""
    (rif, field), pos, xt, vt = _profiles(rif, field), _f(pos), _f(xt), _f(vt)
    dx, dv, dtau = (None if a is None else _f(a) for a in (dx, dv, dtau))
    rec = np.ascontiguousarray(np.asarray(rec_steps).astype(np.uint32))
    n = len(pos)
    grad, gfield = np.empty(rif.size, np.float64), np.empty(rif.size, np.float64)
    dpos, dvel = np.empty_like(pos), np.empty_like(pos)
    rsteps, failed = np.empty(n, np.uint32), np.empty(n, np.uint8)
    rc = lib().cable_field_host_backtrace(_p(rif), _p(field), C.c_int(rif.size), C.c_float(radius), C.c_float(length),
                                          C.c_size_t(n), _p(pos), _p(xt), _p(vt), _p(rec), _p(dx), _p(dv), _p(dtau),
                                          C.c_float(ds), _p(grad), _p(gfield), _p(dpos), _p(dvel), _p(rsteps), _p(failed))
    assert rc == 0
    failed = failed.astype(bool)
    return dict(grad=grad, grad_field=gfield, dpos=dpos, dvel=dvel, steps=rsteps, failed=failed,
                ray_steps=int(rsteps.astype(np.int64).sum()), iters=int(rsteps.max()) if n else 0, n_failed=int(failed.sum()))
