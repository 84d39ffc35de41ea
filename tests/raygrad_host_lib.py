"""Loader for tests/raygrad_host/raygrad_host.hip (TEST INFRASTRUCTURE ONLY): the product's own __host__ __device__
ray-state adjoint (backtrace_ray_state of csrc/drrt_device.h) compiled for the host.  Never imported by the package."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "raygrad_host", "raygrad_host.hip")
_HDR = os.path.join(_HERE, "..", "adjointnonlinearraytracing_amd", "csrc", "drrt_device.h")
_SO = os.path.join(_HERE, "raygrad_host", "_build", "libraygrad_host.so")
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


def backtrace_rays(rif, res, pos, vel, xt, vt, steps, dx, dv, h, ds):
    """-> dict(dpos, dvel, ray_steps, n_failed), the host build of what drrt_backtrace_rays_f32 computes."""
    rif = _f(rif).reshape(-1)
    pos, vel, xt, vt, dx, dv = (_f(a) for a in (pos, vel, xt, vt, dx, dv))
    steps = np.ascontiguousarray(np.asarray(steps).astype(np.uint32))
    n = len(pos)
    dpos, dvel = np.empty_like(pos), np.empty_like(vel)
    st, nf = C.c_longlong(0), C.c_longlong(0)
    res_ = np.asarray(list(res), dtype=np.int32)
    lib().raygrad_host_backtrace_rays(_p(rif), _p(res_), C.c_size_t(n), _p(pos), _p(vel), _p(xt), _p(vt), _p(steps),
                                      _p(dx), _p(dv), C.c_float(h), C.c_float(ds), _p(dpos), _p(dvel),
                                      C.byref(st), C.byref(nf))
    return dict(dpos=dpos, dvel=dvel, ray_steps=st.value, n_failed=nf.value)
