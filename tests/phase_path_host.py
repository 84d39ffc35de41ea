"""Loader for tests/hostcheck/phase_path_rays.hip (TEST INFRASTRUCTURE ONLY): trace_phase_ray and phase_backtrace_ray of
csrc/drrt_device.h compiled for the host by hostcheck_lib.build() into a library of their own, looped as the kernels run
them.  Never imported by the package."""
import ctypes as C
import os

import numpy as np

from hostcheck_lib import HOSTCHECK, _f, _p, _res, build

SOURCE = os.path.join(HOSTCHECK, "phase_path_rays.hip")
_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = build("libphase_path_rays.so", [SOURCE])
    return _lib


def trace_phase(rif, res, pos, vel, h, ds, stride, samples):
    """-> dict(xt, vt, path, vpath ((samples, n, 3) each), count, steps, n_failed): the host build of what
    drrt_trace_phase_f32 computes."""
    rif = _f(rif).reshape(-1)
    pos, vel = _f(pos).reshape(-1, 3), _f(vel).reshape(-1, 3)
    n = len(pos)
    xt, vt, steps, nf = np.empty_like(pos), np.empty_like(vel), np.empty(n, np.uint32), C.c_longlong(0)
    path, vpath = np.empty((samples, n, 3), np.float32), np.empty((samples, n, 3), np.float32)
    count = np.empty(n, np.int32)
    rc = lib().phase_host_trace(_p(rif), _p(_res(res)), C.c_size_t(n), _p(pos), _p(vel), C.c_float(h), C.c_float(ds),
                                C.c_int(stride), C.c_int(samples), _p(xt), _p(vt), _p(path), _p(vpath), _p(count), _p(steps),
                                C.byref(nf))
    assert rc == 0
    return dict(xt=xt, vt=vt, path=path, vpath=vpath, count=count, steps=steps, n_failed=int(nf.value))


def backtrace_phase(rif, res, pos, vel, xt, vt, steps, dx, dv, dpath, dvpath, h, ds, stride, samples, corrected_h=True):
    """-> dict(grad float64[nvox], dpos, dvel, steps (reverse iterations per ray), failed, ray_steps, n_failed): the host
    build of what drrt_backtrace_phase_f32 computes; dx, dv, dpath, dvpath ((samples, n, 3)) may be None."""
    rif = _f(rif).reshape(-1)
    pos, vel, xt, vt = (_f(a).reshape(-1, 3) for a in (pos, vel, xt, vt))
    n = len(pos)
    seeds = [None if a is None else _f(a) for a in (dx, dv, dpath, dvpath)]
    assert all(a is None or a.shape == (samples, n, 3) for a in seeds[2:])
    steps = np.ascontiguousarray(np.asarray(steps).astype(np.uint32))
    grad = np.empty(rif.size, np.float64)
    dpos, dvel = np.empty_like(pos), np.empty_like(vel)
    rsteps, failed = np.empty(n, np.uint32), np.empty(n, np.uint8)
    rc = lib().phase_host_backtrace(_p(rif), _p(_res(res)), C.c_size_t(n), _p(pos), _p(vel), _p(xt), _p(vt), _p(steps),
                                    *map(_p, seeds), C.c_float(h), C.c_float(ds), C.c_int(stride), C.c_int(samples),
                                    C.c_int(bool(corrected_h)), _p(grad), _p(dpos), _p(dvel), _p(rsteps), _p(failed))
    assert rc == 0
    failed = failed.astype(bool)
    return dict(grad=grad, dpos=dpos, dvel=dvel, steps=rsteps, failed=failed,
                ray_steps=int(rsteps.astype(np.int64).sum()), n_failed=int(failed.sum()))
