"""Loader for tests/hostcheck/vector_rays.hip (TEST INFRASTRUCTURE ONLY): the product's per-ray routines of the line
integral of a vector field (trace_vector_ray, vector_backtrace_ray of csrc/drrt_device.h) compiled for the host with the line
of hostcheck_lib.lib(), looped as the kernels run them.  Never imported by the package."""
import ctypes as C
import os
import subprocess

import numpy as np

from hostcheck_lib import _f, _p, _res

_HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(_HERE, "hostcheck", "vector_rays.hip")
_HDR = os.path.join(_HERE, "..", "adjointnonlinearraytracing_amd", "csrc", "drrt_device.h")
_SO = os.path.join(_HERE, "hostcheck", "_build", "libvector_rays.so")
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


def _grids(rif, vfield):
    rif, vfield = _f(rif), _f(vfield)
    assert vfield.shape == (3,) + rif.shape, "vfield must have shape (3,) + rif.shape"
    return rif.reshape(-1), vfield.reshape(-1)


def trace_vector(rif, vfield, res, pos, vel, h, ds):
    """-> dict(xt, vt, circ, steps, n_failed): the host build of what drrt_trace_vector_f32 computes."""
    (rif, vfield), pos, vel = _grids(rif, vfield), _f(pos), _f(vel)
    n = len(pos)
    xt, vt = np.empty_like(pos), np.empty_like(vel)
    circ, steps = np.empty(n, np.float32), np.empty(n, np.uint32)
    nf = C.c_longlong(0)
    rc = lib().vector_host_trace(_p(rif), _p(vfield), _p(_res(res)), C.c_size_t(n), _p(pos), _p(vel), C.c_float(h),
                                 C.c_float(ds), _p(xt), _p(vt), _p(circ), _p(steps), C.byref(nf))
    assert rc == 0
    return dict(xt=xt, vt=vt, circ=circ, steps=steps, n_failed=int(nf.value))


def backtrace_vector(rif, vfield, res, pos, vel, xt, vt, steps, dx, dv, dcirc, h, ds, corrected_h=True, parts=0):
    """-> dict(grad float64[nvox], grad_vfield float64[3 nvox], dpos, dvel, steps (reverse iterations per ray), failed,
    ray_steps, n_failed): the host build of what drrt_backtrace_vector_f32 computes; dx, dv, dcirc may be None (zeros).
    `parts`: 0 = the whole gradients, 1 = the value weights of every contribution alone, 2 = their gradient splats alone
    (dL/du has none)."""
    rif, vfield = _grids(rif, vfield)
    pos, vel, xt, vt = (_f(a) for a in (pos, vel, xt, vt))
    dx, dv, dcirc = (None if a is None else _f(a) for a in (dx, dv, dcirc))
    steps = np.ascontiguousarray(np.asarray(steps).astype(np.uint32))
    n = len(pos)
    grad, gv = np.empty(rif.size, np.float64), np.empty(3 * rif.size, np.float64)
    dpos, dvel = np.empty_like(pos), np.empty_like(vel)
    rsteps, failed = np.empty(n, np.uint32), np.empty(n, np.uint8)
    rc = lib().vector_host_backtrace(_p(rif), _p(vfield), _p(_res(res)), C.c_size_t(n), _p(pos), _p(vel), _p(xt), _p(vt),
                                     _p(steps), _p(dx), _p(dv), _p(dcirc), C.c_float(h), C.c_float(ds),
                                     C.c_int(bool(corrected_h)), C.c_int(parts), _p(grad), _p(gv), _p(dpos), _p(dvel),
                                     _p(rsteps), _p(failed))
    assert rc == 0
    failed = failed.astype(bool)
    return dict(grad=grad, grad_vfield=gv, dpos=dpos, dvel=dvel, steps=rsteps, failed=failed,
                ray_steps=int(rsteps.astype(np.int64).sum()), n_failed=int(failed.sum()))
