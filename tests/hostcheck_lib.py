"""Loader for tests/hostcheck/hostcheck.hip (TEST INFRASTRUCTURE ONLY): the product's own
__host__ __device__ per-ray code compiled for the host, so CPU-only tests can compare it with the
oracle's `factored` arithmetic bit for bit, and its ray-state adjoints with float64 autograd.  Never imported by the
package."""
import ctypes as C
import glob
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
HOSTCHECK = os.path.join(_HERE, "hostcheck")
SOURCES = [os.path.join(HOSTCHECK, "hostcheck.hip")]              # what a build of the library compiles
_CSRC = os.path.join(_HERE, "..", "adjointnonlinearraytracing_amd", "csrc")
_HDRS = [os.path.join(_CSRC, "drrt_device.h"), os.path.join(_CSRC, "drrt_keys.h")]   # what the units include of the product
HIPCC = "/opt/rocm/bin/hipcc"
_lib = None


def build(so_name, sources):
    """-> the CDLL of tests/hostcheck/_build/<so_name>, compiled from `sources` for the host if it is missing or older than
    a source, a header of tests/hostcheck or one of the product's headers the units include."""
    so = os.path.join(HOSTCHECK, "_build", so_name)
    deps = list(sources) + glob.glob(os.path.join(HOSTCHECK, "*.h")) + _HDRS
    os.makedirs(os.path.dirname(so), exist_ok=True)
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in deps):
        subprocess.run([HIPCC, "--cuda-host-only", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-mfma", "-shared",
                        "-fvisibility=hidden", "-o", so] + list(sources), check=True, capture_output=True)
    return C.CDLL(so)


def lib():
    global _lib
    if _lib is None:
        _lib = build("libhostcheck.so", SOURCES)
    return _lib


def sanitized_program(tmp_path, source, define):
    """-> the path of `source` built with -D<define> as a stand-alone program (its own main) under AddressSanitizer +
    UndefinedBehaviorSanitizer, to be run as a child process with nothing preloaded; skips the test that calls it where
    the image has no sanitizer runtime."""
    import pytest
    if not glob.glob("/opt/rocm*/lib/llvm/lib/clang/*/lib/linux/libclang_rt.asan-x86_64.a") or not os.path.exists(HIPCC):
        pytest.skip("no clang sanitizer runtime in this image")
    exe = str(tmp_path / (define.lower() + "_sanitize"))
    subprocess.run([HIPCC, "--cuda-host-only", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-mfma", "-D" + define,
                    "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                    "-o", exe, source], check=True, capture_output=True)
    return exe


def write_case(path, ints, floats, arrays):
    """The case file of a stand-alone program: `ints` as int32, `floats` as float32, then every array as float32."""
    with open(path, "wb") as f:
        f.write(np.array(ints, np.int32).tobytes())
        f.write(np.array(floats, np.float32).tobytes())
        for a in arrays:
            f.write(np.ascontiguousarray(a, np.float32).tobytes())


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _f(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32))


def _res(res):
    return np.asarray(list(res), dtype=np.int32)


def trace(rif, res, pos, vel, h, ds, mode="trace", sdf=None, pln_o=None, pln_d=None):
    m = {"trace": 0, "plane": 1, "sdf": 2}[mode]
    rif, pos, vel = _f(rif).reshape(-1), _f(pos), _f(vel)
    sdf = None if sdf is None else _f(sdf).reshape(-1)
    po = None if pln_o is None else _f(pln_o); pd = None if pln_d is None else _f(pln_d)
    n = len(pos)
    xt, vt = np.empty_like(pos), np.empty_like(vel)
    fm = np.zeros(n, np.uint8); steps = np.zeros(n, np.int32); nf = C.c_longlong(0)
    lib().hostcheck_trace(m, _p(rif), _p(sdf), _p(_res(res)), C.c_size_t(n), _p(pos), _p(vel), _p(po), _p(pd),
                          C.c_float(h), C.c_float(ds), _p(xt), _p(vt), _p(fm), _p(steps), C.byref(nf))
    return dict(xt=xt, vt=vt, failmask=fm.astype(bool), steps=steps, n_failed=nf.value)


def trace_target(rif, res, pos, vel, target, h, ds):
    rif, pos, vel, target = _f(rif).reshape(-1), _f(pos), _f(vel), _f(target)
    n = len(pos)
    xt, vt, d2 = np.empty_like(pos), np.empty_like(vel), np.empty(n, np.float32)
    it = C.c_int(0)
    lib().hostcheck_trace_target(_p(rif), _p(_res(res)), C.c_size_t(n), _p(pos), _p(vel), _p(target),
                                 C.c_float(h), C.c_float(ds), _p(xt), _p(vt), _p(d2), C.byref(it))
    return dict(xt=xt, vt=vt, dist2=d2, iters=it.value)


def backtrace(rif, res, xt, vt, dx, dv, h, ds, sdf=None, corrected_h=False):
    rif = _f(rif).reshape(-1)
    sdf_ = None if sdf is None else _f(sdf).reshape(-1)
    xt, vt, dx, dv = _f(xt), _f(vt), _f(dx), _f(dv)
    grad = np.zeros(rif.size, np.float32); st = C.c_longlong(0)
    gs = float(np.float32(1.0) / np.float32(h)) if corrected_h else 1.0
    lib().hostcheck_backtrace(0 if sdf is None else 1, _p(rif), _p(sdf_), _p(_res(res)), C.c_size_t(len(xt)),
                              _p(xt), _p(vt), _p(dx), _p(dv), C.c_float(h), C.c_float(ds), C.c_float(gs),
                              _p(grad), C.byref(st))
    return dict(grad=grad, steps_total=st.value)


def trace_cable(rif, radius, length, pos, vel, target, ds):
    rif, pos, vel, target = _f(rif).reshape(-1), _f(pos), _f(vel), _f(target)
    n = len(pos)
    xt, vt, d2 = np.empty_like(pos), np.empty_like(vel), np.empty(n, np.float32)
    st = C.c_longlong(0)
    lib().hostcheck_trace_cable(_p(rif), C.c_int(rif.size), C.c_float(radius), C.c_float(length), C.c_size_t(n),
                                _p(pos), _p(vel), _p(target), C.c_float(ds), _p(xt), _p(vt), _p(d2), C.byref(st))
    return dict(xt=xt, vt=vt, dist2=d2, steps_total=st.value)


def backtrace_cable(rif, radius, length, xt, vt, dx, dv, ds):
    rif = _f(rif).reshape(-1)
    xt, vt, dx, dv = _f(xt), _f(vt), _f(dx), _f(dv)
    grad = np.zeros(rif.size, np.float32); st = C.c_longlong(0)
    lib().hostcheck_backtrace_cable(_p(rif), C.c_int(rif.size), C.c_float(radius), C.c_float(length),
                                    C.c_size_t(len(xt)), _p(xt), _p(vt), _p(dx), _p(dv), C.c_float(ds),
                                    _p(grad), C.byref(st))
    return dict(grad=grad, steps_total=st.value)


# ---- ray-state adjoints: dL/dpos, dL/dvel ---------------------------------------------------------------------------
def backtrace_rays(rif, res, pos, vel, xt, vt, steps, dx, dv, h, ds):
    """-> dict(dpos, dvel, ray_steps, n_failed), the host build of what drrt_backtrace_rays_f32 computes."""
    rif = _f(rif).reshape(-1)
    pos, vel, xt, vt, dx, dv = (_f(a) for a in (pos, vel, xt, vt, dx, dv))
    steps = np.ascontiguousarray(np.asarray(steps).astype(np.uint32))
    n = len(pos)
    dpos, dvel = np.empty_like(pos), np.empty_like(vel)
    st, nf = C.c_longlong(0), C.c_longlong(0)
    lib().raygrad_host_backtrace_rays(_p(rif), _p(_res(res)), C.c_size_t(n), _p(pos), _p(vel), _p(xt), _p(vt), _p(steps),
                                      _p(dx), _p(dv), C.c_float(h), C.c_float(ds), _p(dpos), _p(dvel),
                                      C.byref(st), C.byref(nf))
    return dict(dpos=dpos, dvel=dvel, ray_steps=st.value, n_failed=nf.value)


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


def _backtrace_stop_rays(mode, rif, sdf, res, pos, vel, po, pd, dx, dv, h, ds):
    rif = _f(rif).reshape(-1)
    sdf = None if sdf is None else _f(sdf).reshape(-1)
    pos, vel, dx, dv = (_f(a) for a in (pos, vel, dx, dv))
    po, pd = (None if a is None else _f(a) for a in (po, pd))
    n = len(pos)
    dpos, dvel, xt, vt = (np.empty_like(pos) for _ in range(4))
    jstar, steps, fwd = (np.empty(n, np.uint32) for _ in range(3))
    flags = np.empty(n, np.uint8)
    iters = C.c_uint32(0)
    rc = lib().stop_raygrad_host_backtrace_rays(C.c_int(mode), _p(rif), _p(sdf), _p(_res(res)), C.c_size_t(n), _p(pos),
                                                _p(vel), _p(po), _p(pd), _p(dx), _p(dv), C.c_float(h), C.c_float(ds),
                                                _p(dpos), _p(dvel), _p(xt), _p(vt), _p(jstar), _p(steps), _p(fwd),
                                                _p(flags), C.byref(iters))
    assert rc == 0
    failed, again = (flags & 1).astype(bool), (flags & 2).astype(bool)
    return dict(dpos=dpos, dvel=dvel, xt=xt, vt=vt, jstar=jstar, steps=steps, fwd=fwd, failed=failed, again=again,
                ray_steps=int(steps.astype(np.int64).sum()), iters=int(iters.value), n_failed=int(failed.sum()))


def backtrace_pln_rays(rif, res, pos, vel, pln_o, pln_d, dx, dv, h, ds):
    """-> dict(dpos, dvel, xt, vt, jstar, steps, fwd, failed, again, ray_steps, iters, n_failed): the host build of what
    drrt_backtrace_pln_rays_f32 computes, plus the record it replayed (xt, vt, its iteration jstar) and which rays went
    through the second pass (again)."""
    return _backtrace_stop_rays(1, rif, None, res, pos, vel, pln_o, pln_d, dx, dv, h, ds)


def backtrace_sdf_rays(rif, sdf, res, pos, vel, dx, dv, h, ds):
    """The same for drrt_backtrace_sdf_rays_f32."""
    return _backtrace_stop_rays(2, rif, sdf, res, pos, vel, None, None, dx, dv, h, ds)


# ---- 16-bit ray state: the __host__ __device__ codecs of drrt_device.h -----------------------------------------------
def q16_params(res, h):
    """-> float32[3]: q_min, q_step, q_inv_step of the Vol that vol_finish builds."""
    out = np.empty(3, np.float32)
    lib().hostcheck_q16_params(_p(_res(res)), C.c_float(h), _p(out))
    return out


def _q16(name, res, h, a, in_dtype, out_dtype):
    a = np.ascontiguousarray(np.asarray(a, dtype=in_dtype))
    out = np.empty(a.shape, out_dtype)
    getattr(lib(), name)(_p(_res(res)), C.c_float(h), C.c_size_t(a.size), _p(a), _p(out))
    return out


def q16_pos_enc(res, h, x):
    return _q16("hostcheck_q16_pos_enc", res, h, x, np.float32, np.uint16)


def q16_pos_dec(res, h, code):
    return _q16("hostcheck_q16_pos_dec", res, h, code, np.uint16, np.float32)


def q16_vel_enc(res, h, v):
    return _q16("hostcheck_q16_vel_enc", res, h, v, np.float32, np.int16)


def q16_vel_dec(res, h, code):
    return _q16("hostcheck_q16_vel_dec", res, h, code, np.int16, np.float32)


# ---- locality-sort keys: the __host__ __device__ key functions of drrt_keys.h ---------------------------------------
def hilbert2(x, y):
    x = np.ascontiguousarray(np.asarray(x, dtype=np.uint32)); y = np.ascontiguousarray(np.asarray(y, dtype=np.uint32))
    assert x.shape == y.shape
    d = np.empty(x.shape, np.uint32)
    lib().hostcheck_hilbert2(C.c_size_t(x.size), _p(x), _p(y), _p(d))
    return d


def lf_cell_frame(a, b):
    """-> (c, t1, t2), each (n,3) float32: the centre direction and the frame of the direction cells (a, b)."""
    a = np.ascontiguousarray(np.asarray(a, dtype=np.int32)); b = np.ascontiguousarray(np.asarray(b, dtype=np.int32))
    assert a.shape == b.shape and a.ndim == 1
    c, t1, t2 = (np.empty((a.size, 3), np.float32) for _ in range(3))
    lib().hostcheck_lf_cell_frame(C.c_size_t(a.size), _p(a), _p(b), _p(c), _p(t1), _p(t2))
    return c, t1, t2


def _keys(name, dtype, res, h, pos, vel, sign):
    pos, vel = _f(pos), _f(vel)
    assert pos.shape == vel.shape and pos.ndim == 2 and pos.shape[1] == 3
    out = np.empty(len(pos), dtype)
    getattr(lib(), name)(_p(_res(res)), C.c_float(h), C.c_size_t(len(pos)), _p(pos), _p(vel), C.c_float(sign), _p(out))
    return out


def lightfield_keys(res, h, pos, vel, sign=1.0):
    """-> uint32[n]: what k_lightfield_keys writes for the fp32 rays (pos, vel) with dir_sign = sign."""
    return _keys("hostcheck_lightfield_keys", np.uint32, res, h, pos, vel, sign)


def chord_keys(res, h, pos, vel, sign=1.0):
    """-> uint64[n]: what k_chord_keys writes."""
    return _keys("hostcheck_chord_keys", np.uint64, res, h, pos, vel, sign)
