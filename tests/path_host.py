"""Loader for tests/hostcheck/path_rays.hip (TEST INFRASTRUCTURE ONLY): the product's per-ray routines of the ray-path
operator (trace_path_ray, path_backtrace_ray of csrc/drrt_device.h) compiled for the host with the line of
hostcheck_lib.lib(), looped as the kernels run them.  Never imported by the package."""
import ctypes as C
import os
import subprocess

import numpy as np

from hostcheck_lib import _f, _p, _res

_HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(_HERE, "hostcheck", "path_rays.hip")
_HDR = os.path.join(_HERE, "..", "adjointnonlinearraytracing_amd", "csrc", "drrt_device.h")
_SO = os.path.join(_HERE, "hostcheck", "_build", "libpath_rays.so")
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


def trace_path(rif, res, pos, vel, h, ds, stride, samples):
    """-> dict(xt, vt, path (samples, n, 3), count, steps, n_failed): the host build of what drrt_trace_path_f32 computes."""
    rif, pos, vel = _f(rif).reshape(-1), _f(pos).reshape(-1, 3), _f(vel).reshape(-1, 3)
    n = len(pos)
    xt, vt = np.empty_like(pos), np.empty_like(vel)
    path = np.empty((samples, n, 3), np.float32)
    count, steps = np.empty(n, np.int32), np.empty(n, np.uint32)
    nf = C.c_longlong(0)
    rc = lib().path_host_trace(_p(rif), _p(_res(res)), C.c_size_t(n), _p(pos), _p(vel), C.c_float(h), C.c_float(ds),
                               C.c_int(stride), C.c_int(samples), _p(xt), _p(vt), _p(path), _p(count), _p(steps), C.byref(nf))
    assert rc == 0
    return dict(xt=xt, vt=vt, path=path, count=count, steps=steps, n_failed=int(nf.value))


def backtrace_path(rif, res, pos, vel, xt, vt, steps, dx, dv, dpath, h, ds, stride, samples, corrected_h=True):
    """-> dict(grad float64[nvox], dpos, dvel, steps (reverse iterations per ray), failed, ray_steps, n_failed): the host
    build of what drrt_backtrace_path_f32 computes; dx, dv, dpath ((samples, n, 3)) may be None (zeros)."""
    rif = _f(rif).reshape(-1)
    pos, vel, xt, vt = (_f(a).reshape(-1, 3) for a in (pos, vel, xt, vt))
    dx, dv, dpath = (None if a is None else _f(a) for a in (dx, dv, dpath))
    steps = np.ascontiguousarray(np.asarray(steps).astype(np.uint32))
    n = len(pos)
    assert dpath is None or dpath.shape == (samples, n, 3)
    grad = np.empty(rif.size, np.float64)
    dpos, dvel = np.empty_like(pos), np.empty_like(vel)
    rsteps, failed = np.empty(n, np.uint32), np.empty(n, np.uint8)
    rc = lib().path_host_backtrace(_p(rif), _p(_res(res)), C.c_size_t(n), _p(pos), _p(vel), _p(xt), _p(vt), _p(steps), _p(dx),
                                   _p(dv), _p(dpath), C.c_float(h), C.c_float(ds), C.c_int(stride), C.c_int(samples),
                                   C.c_int(bool(corrected_h)), _p(grad), _p(dpos), _p(dvel), _p(rsteps), _p(failed))
    assert rc == 0
    failed = failed.astype(bool)
    return dict(grad=grad, dpos=dpos, dvel=dvel, steps=rsteps, failed=failed,
                ray_steps=int(rsteps.astype(np.int64).sum()), n_failed=int(failed.sum()))
