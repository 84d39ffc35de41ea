"""ctypes binding of ``libdrrt_hip.so`` -- the C ABI declared in ``include/drrt_hip.h``.

There is NO fallback: if the shared library is missing or a call fails, a ``RuntimeError`` is
raised (the reference turns ``std::runtime_error`` into Python ``RuntimeError`` the same way,
pybind default translator, ``/root/reference/src/volume.cpp:28,37,115,124``).
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

_HERE = os.path.dirname(os.path.abspath(__file__))
# DRRT_HIP_LIB: developer override (A-B builds of the same sources, e.g. other compiler flags); default = the in-tree build
LIB_PATH = os.environ.get("DRRT_HIP_LIB") or os.path.join(_HERE, "libdrrt_hip.so")

# flags (include/drrt_hip.h)
FLAG_NONE = 0
FLAG_SORT_RAYS = 1
FLAG_CORRECTED_H = 2
FLAG_NO_ZERO = 4
FLAG_DIRECT_ATOMICS = 8
FLAG_DEBUG_COUNTERS = 16
FLAG_PAIR_GRID = 64
FLAG_PAIR_REUSE = 128
FLAG_QUAD_GRID, FLAG_QUAD_REUSE = FLAG_PAIR_GRID, FLAG_PAIR_REUSE      # round-1 names
FLAG_Q16_POS_ONLY = 0x200000
FLAG_STATIC_WINDOW = 0x400000
FLAG_CHORD_KEY = 0x800000
FLAG_RING_WINDOW = 0x1000000
FLAG_DISPATCH_IN_ORDER = 0x2000000
FLAG_RING_SPARSE, FLAG_RING_GENERAL, FLAG_RING_DIRECT = 0x4000000, 0x8000000, 0x10000000
ADAM_MASK_BOUNDARY, ADAM_CLAMP_MIN = 1, 2

ERR_RES_MISMATCH, ERR_BAD_RES, ERR_ARG, ERR_HIP = -1, -2, -3, -4


class Stats(C.Structure):
    """Mirror of ``drrt_stats`` (device-resident; copy back to read)."""
    _fields_ = [("ray_steps", C.c_ulonglong), ("n_failed", C.c_ulonglong),
                ("iters", C.c_uint), ("reserved", C.c_uint)]


STATS_BYTES = C.sizeof(Stats)

_vp, _f, _sz, _u, _ll, _i = C.c_void_p, C.c_float, C.c_size_t, C.c_uint, C.c_longlong, C.c_int
_d = C.c_double
_tail = [_vp, _vp, _sz, _u, _vp]          # stats, workspace, workspace_bytes, flags, stream


def _sensor_signatures():
    """The 12 sensor entries, drrt_sensor_{family}[_dframe][_bwd]_f32: the family's rays, then its frame -- host float[3]
    vectors (p, n, t1, t2; the far field t1, t2), or ONE device pointer for a `_dframe` twin --, then the tail of the
    direction (res, span, ..., stream).  A twin differs from its plain entry in the frame only."""
    e = [_vp, _f]                                              # e (nullable), e_scalar
    splat = ([_i, _f, _vp, _u, _vp], [_i, _f, _vp, _vp, _vp, _vp])     # image, flags | grad_image, grad_x, grad_v
    families = {       # family: (rays, host vectors of the frame, forward tail, backward tail)
        "splat": ([_sz, _vp, _vp] + e, 4) + splat,
        "far_splat": ([_sz, _vp] + e, 2) + splat,
        "tex_get": ([_sz, _vp, _vp], 4, [_vp, _i, _f, _i, _vp, _vp], [_vp, _i, _f, _i, _vp, _vp, _vp, _vp]),   # tex .. mode, outputs
    }
    return {f"drrt_sensor_{family}{dframe}{bwd}_f32": (_i, rays + [_vp] * (1 if dframe else host) + tails[bool(bwd)])
            for family, (rays, host, *tails) in families.items() for dframe in ("", "_dframe") for bwd in ("", "_bwd")}


def _radiance_signatures():
    """The 8 radiance-splat entries, drrt_sensor_radiance[_far][_dframe][_bwd]_f32: the rays (n, x, v, rad, channels; the
    far field has no x), the frame as in _sensor_signatures(), then (res, span, image, flags) or (res, span, grad_image,
    grad_rad, grad_x, grad_v), and the stream."""
    tails = ([_i, _f, _vp, _u, _vp], [_i, _f, _vp, _vp, _vp, _vp, _vp])
    families = {"radiance": ([_sz, _vp, _vp, _vp, _i], 4), "radiance_far": ([_sz, _vp, _vp, _i], 2)}
    return {f"drrt_sensor_{family}{dframe}{bwd}_f32": (_i, rays + [_vp] * (1 if dframe else host) + tails[bool(bwd)])
            for family, (rays, host) in families.items() for dframe in ("", "_dframe") for bwd in ("", "_bwd")}


SIGNATURES = {
    # name: (restype, argtypes)   -- must stay in sync with include/drrt_hip.h
    "drrt_workspace_bytes": (_sz, [_sz, _u]),
    "drrt_workspace_bytes_grid": (_sz, [_sz, _ll, _u]),
    "drrt_last_error": (C.c_char_p, []),
    "drrt_version": (C.c_char_p, []),
    "drrt_trace_f32": (_i, [_vp, _ll, _vp, _sz, _vp, _vp, _f, _f, _vp, _vp] + _tail),
    "drrt_trace_f16io": (_i, [_vp, _ll, _vp, _sz, _vp, _vp, _f, _f, _vp, _vp] + _tail),
    "drrt_backtrace_f16io": (_i, [_vp, _ll, _vp, _sz, _vp, _vp, _vp, _vp, _f, _f, _vp] + _tail),
    "drrt_trace_q16io": (_i, [_vp, _ll, _vp, _sz, _vp, _vp, _f, _f, _vp, _vp] + _tail),
    "drrt_backtrace_q16io": (_i, [_vp, _ll, _vp, _sz, _vp, _vp, _vp, _vp, _f, _f, _vp] + _tail),
    "drrt_q16_params": (_i, [_vp, _f, _vp]),
    "drrt_q16_encode": (_i, [_vp, _f, _sz, _vp, _vp, _vp, _vp, _vp]),
    "drrt_q16_decode": (_i, [_vp, _f, _sz, _vp, _vp, _vp, _vp, _vp]),
    "drrt_trace_pln_f32": (_i, [_vp, _ll, _vp, _sz, _vp, _vp, _vp, _vp, _f, _f, _vp, _vp, _vp] + _tail),
    "drrt_trace_target_f32": (_i, [_vp, _ll, _vp, _sz, _vp, _vp, _vp, _f, _f, _vp, _vp, _vp] + _tail),
    "drrt_trace_sdf_f32": (_i, [_vp, _vp, _ll, _vp, _sz, _vp, _vp, _f, _f, _vp, _vp] + _tail),
    "drrt_trace_cable_f32": (_i, [_vp, _sz, _f, _f, _sz, _vp, _vp, _vp, _f, _vp, _vp, _vp] + _tail),
    "drrt_backtrace_f32": (_i, [_vp, _ll, _vp, _sz, _vp, _vp, _vp, _vp, _f, _f, _vp] + _tail),
    "drrt_backtrace_rays_f32": (_i, [_vp, _ll, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _f, _f, _vp, _vp] + _tail),
    "drrt_trace_opl_f32": (_i, [_vp, _ll, _vp, _sz, _vp, _vp, _f, _f, _vp, _vp, _vp, _vp] + _tail),
    "drrt_backtrace_opl_f32": (_i, [_vp, _ll, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _f, _f, _vp, _vp, _vp] + _tail),
    "drrt_trace_field_f32": (_i, [_vp, _vp, _ll, _vp, _sz, _vp, _vp, _f, _f, _vp, _vp, _vp, _vp] + _tail),
    "drrt_backtrace_field_f32": (_i, [_vp, _vp, _ll, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _f, _f, _vp, _vp, _vp, _vp] + _tail),
    "drrt_trace_emission_f32": (_i, [_vp, _vp, _vp, _ll, _vp, _sz, _vp, _vp, _f, _f, _vp, _vp, _vp, _vp, _vp] + _tail),
    "drrt_backtrace_emission_f32": (_i, [_vp, _vp, _vp, _ll, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _f, _f,
                                         _vp, _vp, _vp, _vp, _vp] + _tail),
    "drrt_trace_vector_f32": (_i, [_vp, _vp, _ll, _vp, _sz, _vp, _vp, _f, _f, _vp, _vp, _vp, _vp] + _tail),
    "drrt_backtrace_vector_f32": (_i, [_vp, _vp, _ll, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _f, _f, _vp, _vp, _vp, _vp] + _tail),
    "drrt_trace_path_f32": (_i, [_vp, _ll, _vp, _sz, _vp, _vp, _f, _f, _i, _i, _vp, _vp, _vp, _vp, _vp] + _tail),
    "drrt_backtrace_path_f32": (_i, [_vp, _ll, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _f, _f, _i, _i, _vp, _vp, _vp]
                                + _tail),
    "drrt_trace_phase_f32": (_i, [_vp, _ll, _vp, _sz, _vp, _vp, _f, _f, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp] + _tail),
    "drrt_backtrace_phase_f32": (_i, [_vp, _ll, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _f, _f, _i, _i, _vp, _vp,
                                      _vp] + _tail),
    "drrt_backtrace_chunk_state_bytes": (_sz, [_sz]),
    "drrt_backtrace_max_steps": (_i, [_vp, _f, _f]),
    "drrt_backtrace_chunk_f32": (_i, [_vp, _ll, _vp, _sz, _vp, _vp, _vp, _vp, _f, _f, _vp] + _tail + [_vp, _sz, _i, _i, _vp]),
    "drrt_backtrace_sdf_f32": (_i, [_vp, _vp, _ll, _vp, _sz, _vp, _vp, _vp, _vp, _f, _f, _vp] + _tail),
    "drrt_backtrace_cable_f32": (_i, [_vp, _sz, _f, _f, _sz, _vp, _vp, _vp, _vp, _f, _vp] + _tail),
    "drrt_backtrace_cable_rays_f32": (_i, [_vp, _sz, _f, _f, _sz, _vp, _vp, _vp, _vp, _vp, _f, _vp, _vp] + _tail),
    "drrt_trace_cable_opl_f32": (_i, [_vp, _sz, _f, _f, _sz, _vp, _vp, _vp, _f, _vp, _vp, _vp, _vp, _vp] + _tail),
    "drrt_backtrace_cable_opl_f32": (_i, [_vp, _sz, _f, _f, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _f, _vp, _vp, _vp] + _tail),
    "drrt_trace_cable_field_f32": (_i, [_vp, _vp, _sz, _f, _f, _sz, _vp, _vp, _vp, _f, _vp, _vp, _vp, _vp, _vp] + _tail),
    "drrt_backtrace_cable_field_f32": (_i, [_vp, _vp, _sz, _f, _f, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _f, _vp, _vp, _vp, _vp]
                                       + _tail),
    "drrt_backtrace_pln_rays_f32": (_i, [_vp, _ll, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _f, _f, _vp, _vp] + _tail),
    "drrt_backtrace_sdf_rays_f32": (_i, [_vp, _vp, _ll, _vp, _sz, _vp, _vp, _vp, _vp, _f, _f, _vp, _vp] + _tail),
    "drrt_backtrace_target_rays_f32": (_i, [_vp, _ll, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _f, _f, _vp, _vp] + _tail),
    **_sensor_signatures(),
    **_radiance_signatures(),
    "drrt_rays_to_plane_f32": (_i, [_sz, _vp, _vp, _vp, _vp, _i, _vp, _vp]),
    "drrt_rays_to_plane_bwd_f32": (_i, [_sz, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp]),
    "drrt_upres_volume_f32": (_i, [_vp, _vp, _vp, _vp, _vp]),
    "drrt_adam_step_f32": (_i, [_vp, _vp, _vp, _vp, _vp, _d, _d, _d, _d, _d, _d, _d, _u, _vp]),
    "drrt_gen_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "drrt_gen_rays_f32": (_i, [_i, _vp, _vp, _i, _i, _i, _i, _d, _d, _i, _i, _vp, _d, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "drrt_gen_cone_rays_f32": (_i, [_vp, _vp, _i, _i, _i, _i, _d, _d, _d, _vp, _d, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "drrt_last_order": (_vp, [_vp]),
    "drrt_set_order_hint": (None, [_vp, _sz]),
    "drrt_order_hint_pending": (_sz, []),
    "drrt_last_steps": (_vp, [_vp]),
    "drrt_set_step_hint": (None, [_vp, _sz]),
    "drrt_last_bundle_counters": (_vp, []),
    "drrt_ring_threshold_pct": (_i, []),
    "drrt_ring_long_threshold_permille": (_i, []),
    "drrt_ring_direct_threshold_pct": (_i, []),
    "drrt_profile_begin": (_i, [_i]),
    "drrt_profile_collect": (_i, [_vp, _vp, _i]),
    "drrt_profile_end": (None, []),
}

PROF_NAMES = {1: "trace", 2: "backtrace", 3: "sort", 4: "zero", 5: "quad", 6: "backtrace_rays",
              7: "backtrace_cable_rays", 8: "backtrace_pln_rays", 9: "backtrace_sdf_rays", 10: "backtrace_target_rays",
              11: "trace_opl", 12: "backtrace_opl", 13: "trace_field", 14: "backtrace_field"}
# the ids added after PROF_NAMES was closed (profile_collect consults all three tables)
PROF_NAMES_MORE = {15: "trace_emission", 16: "backtrace_emission"}
# ... and after PROF_NAMES_MORE was: this table stays open, a later id goes here
PROF_NAMES_LATER = {17: "trace_vector", 18: "backtrace_vector", 19: "trace_cable_opl", 20: "backtrace_cable_opl",
                    21: "trace_cable_field", 22: "backtrace_cable_field", 23: "trace_path", 24: "backtrace_path",
                    25: "trace_phase", 26: "backtrace_phase"}

_lib: Optional[C.CDLL] = None


def load() -> C.CDLL:
    """Load libdrrt_hip.so (after torch, so that both share ONE HIP runtime in the process)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"libdrrt_hip.so not found at {LIB_PATH}: build it with "
            "`python -c 'import __graft_entry__ as g; g.build()'` or "
            "`make -C adjointnonlinearraytracing_amd/csrc`.  There is no CPU fallback.")
    import torch  # noqa: F401  (loads torch's libamdhip64.so.7 first; ours binds to the same SONAME)
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError here == header/library mismatch: loud
        fn.restype, fn.argtypes = res, args
    _lib = lib
    return lib


def profile_collect(max_out: int = 4096):
    """-> list of (kernel name, ms) in launch order since the last collect (synchronises)."""
    ids = (C.c_int * max_out)()
    ms = (C.c_float * max_out)()
    n = load().drrt_profile_collect(ids, ms, max_out)
    names = {**PROF_NAMES, **PROF_NAMES_MORE, **PROF_NAMES_LATER}
    return [(names.get(ids[i], str(ids[i])), float(ms[i])) for i in range(n)]


def last_error() -> str:
    return load().drrt_last_error().decode()


def _p(t) -> C.c_void_p:
    """Device pointer of an optional tensor (None -> NULL)."""
    return C.c_void_p(0 if t is None else t.data_ptr())


def _stream(device) -> C.c_void_p:
    """The current stream of `device`."""
    import torch
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def check(rc: int) -> None:
    """Negative status -> RuntimeError carrying the library's message (reference: pybind maps
    std::runtime_error to RuntimeError)."""
    if rc != 0:
        raise RuntimeError(last_error() or f"drrt_hip error {rc}")
