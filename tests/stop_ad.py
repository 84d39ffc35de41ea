"""Differentiable pure-torch restatements of ``Tracer::trace_plane`` and ``Tracer::trace_sdf`` -- TEST INFRASTRUCTURE ONLY.

The automatic-differentiation comparator of the ray-state adjoints drrt_backtrace_pln_rays_f32 / drrt_backtrace_sdf_rays_f32
(the role enoki autodiff plays in the reference, core/tracer.py:122-234).  Written from src/tracer.cpp:102-172 and :244-310:
the whole global loop -- every ray marches until ALL rays are flagged escaped or the step bound is reached -- with the
reference's masks (masked gathers read 0; ``xt[cross] = x`` as a select).  It shares no code with csrc/drrt_device.h; the
trilinear sampler and the box tests are oracle/torch_ad's.  float64 by default.  The package never imports it."""
from __future__ import annotations

import numpy as np
import torch

from oracle.torch_ad import escaped, eval_grad, inbounds


def _max_steps(factor, h, shape, ds):
    """``int max_steps = factor * h * hmax(res) / delta_s`` in the reference's float arithmetic (:120, :262)."""
    return int(np.float32(factor) * np.float32(h) * np.float32(max(shape)) / np.float32(ds))


def trace_plane(rif, pos, vel, pln_o, pln_d, h, ds):
    """-> (xt, vt, failmask, j): j = the iteration count at each ray's last record update (0: the record is the input)."""
    shape = rif.shape
    x, v = pos.clone(), vel.clone()
    xt, vt = pos.clone(), vel.clone()
    inside = inbounds(shape, h, x)                                        # :130 (no plane term)
    esc = torch.zeros_like(inside)
    j = torch.zeros(len(pos), dtype=torch.long)
    for i in range(_max_steps(4.0, h, shape, ds)):
        n, g = eval_grad(rif, x, h, inside)                               # :137
        v = v + (ds * n)[:, None] * g                                     # :139
        x = x + ds * v                                                    # :140
        past = ((x - pln_o) * pln_d).sum(-1) > 0                          # :144
        cur_inside = inbounds(shape, h, x) & ~past                        # :145
        cross = inside & ~cur_inside                                      # :146
        esc = esc | cross | escaped(shape, h, x, v)                       # :147-148
        xt = torch.where(cross[:, None], x, xt)                           # :151-152
        vt = torch.where(cross[:, None], v, vt)
        j = torch.where(cross, torch.full_like(j, i + 1), j)
        if bool(esc.all()):                                               # :154
            break
        inside = cur_inside                                               # :158
    xt = torch.where(esc[:, None], xt, x)                                 # :167
    return xt, vt, ~esc, j


def trace_sdf(rif, sdf, pos, vel, h, ds):
    """-> (xt, vt, j)."""
    shape = rif.shape
    x, v = pos.clone(), vel.clone()
    xt, vt = pos.clone(), vel.clone()
    inside = inbounds(shape, h, x)                                        # :272
    esc = torch.zeros_like(inside)
    j = torch.zeros(len(pos), dtype=torch.long)
    for i in range(_max_steps(2.0, h, shape, ds)):                        # :262
        n, g = eval_grad(rif, x, h, inside)                               # :282
        v = v + (ds * n)[:, None] * g
        x = x + ds * v
        dist, _ = eval_grad(sdf, x, h, inside)                            # :287 (masked: reads 0 once outside)
        cur_inside = dist < 0                                             # :288
        cross = inside & ~cur_inside
        esc = esc | cross | escaped(shape, h, x, v)
        xt = torch.where(cross[:, None], x, xt)
        vt = torch.where(cross[:, None], v, vt)
        j = torch.where(cross, torch.full_like(j, i + 1), j)
        if bool(esc.all()):
            break
        inside = cur_inside
    return xt, vt, j


def n_grad_n(rif, p, h):
    """n(p) grad n(p) at one point p (3,), sampled unmasked: the refraction term of one iteration."""
    n, g = eval_grad(rif, p[None], h, torch.tensor([True]))
    return (n[:, None] * g)[0]
