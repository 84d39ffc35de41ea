"""The three compressed ray-state formats, restated in numpy -- TEST INFRASTRUCTURE ONLY.

Written from the description of the formats in ``include/drrt_hip.h`` ("16-bit ray state") and
``csrc/drrt_device.h``; it calls neither the library nor the host build of its code, so the tests can pin both to it.

  mode     positions                directions               adjoint seeds
  "f16"    IEEE half                IEEE half                IEEE half
  "q16"    box-relative u16 codes   2^-14 fixed point (i16)  IEEE half
  "qpos"   box-relative u16 codes   fp32                     fp32

Position codes cover [-E/16, E + E/16], E = the largest box extent (res - 1) * h, in 65535 steps; out-of-range values
saturate.  Every operation below is the single IEEE-754 binary32 operation the format's description names: numpy float32
scalars and arrays compute in binary32 and round to nearest even.
"""
from __future__ import annotations

import numpy as np

MODES = ("f16", "q16", "qpos")
KINDS = ("pos", "vel", "seed")
VEL_STEP = np.float32(2.0 ** -14)

_F = np.float32


def params(res, h):
    """-> (q_min, q_step, q_inv_step) as float32 scalars, each computed in fp32 arithmetic."""
    h = _F(h)
    with np.errstate(all="ignore"):
        ext = max(_F(int(r) - 1) * h for r in res)            # (float)(res - 1) * h per axis, the largest
        span = ext * _F(1.125)
        return -ext * _F(0.0625), span / _F(65535.0), _F(65535.0) / span


def pos_dec(res, h, code):
    """fma(code, q_step, q_min), rounded once.  The float64 sum is exact: the product of a 16-bit integer and a 24-bit
    significand has at most 40 significant bits, and q_min = -E/16 is a 24-bit term about 3641 steps away, so the sum
    spans fewer than 53 bits; rounding that exact value to fp32 once is what a fused multiply-add returns."""
    q_min, q_step, _ = params(res, h)
    c = np.asarray(code)
    if c.dtype == np.int16:                                   # the library keeps the unsigned codes in int16 storage
        c = c.view(np.uint16)
    if c.dtype != np.uint16:
        raise TypeError(f"position codes are uint16 (or int16 storage), got {c.dtype}")
    return (c.astype(np.float64) * np.float64(q_step) + np.float64(q_min)).astype(np.float32)


def pos_enc(res, h, x):
    """fp32 subtract, fp32 multiply, clamp to [0, 65535] (NaN -> 0), round half to even -> uint16."""
    q_min, _, q_inv = params(res, h)
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(all="ignore"):
        t = (x - q_min) * q_inv
        t = np.where(t > 0, t, _F(0.0))                       # false for NaN
        t = np.where(t < _F(65535.0), t, _F(65535.0))
        return np.rint(t).astype(np.uint16)


def vel_dec(code):
    """code * 2^-14: exact."""
    c = np.asarray(code)
    if c.dtype != np.int16:
        raise TypeError(f"direction codes are int16, got {c.dtype}")
    return c.astype(np.float32) * VEL_STEP


def vel_enc(v):
    """x 16384 in fp32, clamp to [-32768, 32767] (NaN -> -32768), round half to even -> int16."""
    v = np.asarray(v, dtype=np.float32)
    with np.errstate(all="ignore"):
        t = v * _F(16384.0)
        t = np.where(t > _F(-32768.0), t, _F(-32768.0))       # false for NaN
        t = np.where(t < _F(32767.0), t, _F(32767.0))
        return np.rint(t).astype(np.int16)


def half_enc(a):
    """IEEE round to nearest even, subnormals kept, overflow to +-inf (what numpy's float32 -> float16 cast does)."""
    with np.errstate(all="ignore"):
        return np.asarray(a, dtype=np.float32).astype(np.float16)


def _format(mode, kind):
    if mode not in MODES or kind not in KINDS:
        raise ValueError((mode, kind))
    if kind == "pos":
        return "half" if mode == "f16" else "qpos"
    if kind == "vel":
        return {"f16": "half", "q16": "qvel", "qpos": "f32"}[mode]
    return "f32" if mode == "qpos" else "half"


def store(mode, kind, a, res=None, h=None):
    """fp32 array -> what the library keeps for `kind` in `mode`, in the library's storage dtype (position codes: the
    unsigned 16-bit values in int16 storage).  `res`, `h` are needed for q16 / qpos positions."""
    f = _format(mode, kind)
    if f == "half":
        return half_enc(a)
    if f == "qpos":
        return pos_enc(res, h, a).view(np.int16)
    if f == "qvel":
        return vel_enc(a)
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32))


def widen(mode, kind, s, res=None, h=None):
    """Stored array -> the fp32 values the march computes with (exact for every format)."""
    f = _format(mode, kind)
    s = np.asarray(s)
    want = {"half": (np.float16,), "qpos": (np.int16, np.uint16), "qvel": (np.int16,), "f32": (np.float32,)}[f]
    if s.dtype not in want:
        raise TypeError(f"{mode} {kind} is stored as {want[0].__name__}, got {s.dtype}")
    if f == "qpos":
        return pos_dec(res, h, s)
    if f == "qvel":
        return vel_dec(s)
    return s.astype(np.float32)
