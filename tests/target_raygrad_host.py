"""Loader for tests/hostcheck/target_rays.hip (TEST INFRASTRUCTURE ONLY): the product's per-ray ray-state adjoint of
trace_target (target_backtrace_ray_state of csrc/drrt_device.h) compiled for the host by hostcheck_lib.build(),
both passes looped as the kernels run them.  Never imported by the package."""
import ctypes as C
import os

import numpy as np

from hostcheck_lib import HOSTCHECK, _f, _p, _res, build

SOURCE = os.path.join(HOSTCHECK, "target_rays.hip")
_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = build("libtarget_rays.so", [SOURCE])
    return _lib


def backtrace_target_rays(rif, res, pos, vel, target, dx, dv, h, ds, ddist2=None):
    """-> dict(dpos, dvel, xt, vt, dist2, jstar, fwd, steps, failed, iters, ray_steps, n_failed): the host build of what
    drrt_backtrace_target_rays_f32 computes, plus the record it replayed (xt, vt, dist2, its iteration jstar), phase A's
    per-ray iteration counts (fwd) and the call's global loop count (iters)."""
    rif = _f(rif).reshape(-1)
    pos, vel, target, dx, dv = (_f(a) for a in (pos, vel, target, dx, dv))
    dd2 = None if ddist2 is None else _f(ddist2)
    n = len(pos)
    dpos, dvel, xt, vt = (np.empty_like(pos) for _ in range(4))
    dist2 = np.empty(n, np.float32)
    jstar, fwd, steps = (np.empty(n, np.uint32) for _ in range(3))
    failed = np.empty(n, np.uint8)
    iters = C.c_uint32(0)
    rc = lib().target_raygrad_host_backtrace_rays(_p(rif), _p(_res(res)), C.c_size_t(n), _p(pos), _p(vel), _p(target), _p(dx),
                                                  _p(dv), _p(dd2), C.c_float(h), C.c_float(ds), _p(dpos), _p(dvel), _p(xt),
                                                  _p(vt), _p(dist2), _p(jstar), _p(fwd), _p(steps), _p(failed), C.byref(iters))
    assert rc == 0
    failed = failed.astype(bool)
    return dict(dpos=dpos, dvel=dvel, xt=xt, vt=vt, dist2=dist2, jstar=jstar, fwd=fwd, steps=steps, failed=failed,
                iters=int(iters.value), ray_steps=int(steps.astype(np.int64).sum()), n_failed=int(failed.sum()))
