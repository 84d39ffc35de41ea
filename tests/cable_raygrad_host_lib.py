"""Loader for tests/cable_raygrad_host/cable_raygrad_host.hip (TEST INFRASTRUCTURE ONLY): the product's own
__host__ __device__ ray-state adjoint of the cable march (cable_backtrace_ray_state of csrc/drrt_device.h) compiled for the
host.  Never imported by the package."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "cable_raygrad_host", "cable_raygrad_host.hip")
_HDR = os.path.join(_HERE, "..", "adjointnonlinearraytracing_amd", "csrc", "drrt_device.h")
_SO = os.path.join(_HERE, "cable_raygrad_host", "_build", "libcable_raygrad_host.so")
_lib = None


def lib():
    global _lib
    if _lib is None:
        os.makedirs(os.path.dirname(_SO), exist_ok=True)
        if (not os.path.exists(_SO) or os.path.getmtime(_SO) < max(os.path.getmtime(_SRC), os.path.getmtime(_HDR))):
            subprocess.run(["/opt/rocm/bin/hipcc", "--cuda-host-only", "-O2", "-std=c++17", "-fPIC",
                            "-ffp-contract=off", "-mfma", "-shared", "-fvisibility=hidden", "-o", _SO, _SRC],
                           check=True, capture_output=True)
        _lib = C.CDLL(_SO)
    return _lib


def _f(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32))


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def backtrace_cable_rays(rif, radius, length, pos, vel, target, dx, dv, ds):
    """-> dict(dpos, dvel, xt, vt, jstar, steps, ray_steps, iters): the host build of what drrt_backtrace_cable_rays_f32
    computes, plus the record it replayed (xt, vt, and its iteration jstar) and the per-ray iteration counts."""
    rif = _f(rif).reshape(-1)
    pos, vel, target, dx, dv = (_f(a) for a in (pos, vel, target, dx, dv))
    n = len(pos)
    dpos, dvel, xt, vt = (np.empty_like(pos) for _ in range(4))
    jstar, steps = np.empty(n, np.uint32), np.empty(n, np.uint32)
    rc = lib().cable_raygrad_host_backtrace_rays(_p(rif), C.c_int(rif.size), C.c_float(radius), C.c_float(length),
                                                 C.c_size_t(n), _p(pos), _p(vel), _p(target), _p(dx), _p(dv),
                                                 C.c_float(ds), _p(dpos), _p(dvel), _p(xt), _p(vt), _p(jstar), _p(steps))
    assert rc == 0, "the cable ray-state adjoint never marks a ray failed"
    return dict(dpos=dpos, dvel=dvel, xt=xt, vt=vt, jstar=jstar, steps=steps,
                ray_steps=int(steps.astype(np.int64).sum()), iters=int(steps.max()) if n else 0)
