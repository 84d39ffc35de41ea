"""Differentiable pure-torch restatement of ``Tracer::trace_target`` -- TEST INFRASTRUCTURE ONLY.

The automatic-differentiation comparator of the ray-state adjoint drrt_backtrace_target_rays_f32 and of
tracer.ADRayTargetTracerC (the role enoki autodiff plays in the reference, which binds trace_target on its autodiff tracer,
src/drrt.cpp:34).  Written from src/tracer.cpp:174-242: the whole global loop -- every ray marches until ALL rays are flagged
escaped or the step bound is reached, and the closest-approach record is updated on every iteration, escaped or not -- with
the reference's masks (masked gathers read 0; ``xt[closer] = x`` as a select).  It shares no code with csrc/drrt_device.h;
the trilinear sampler and the box tests are oracle/torch_ad's.  float64 by default.  The package never imports it."""
from __future__ import annotations

import torch

from oracle.torch_ad import escaped, eval_grad, inbounds
from stop_ad import _max_steps


def trace_target(rif, pos, vel, target, h, ds):
    """-> (xt, vt, dist2, j): j = the iteration count at each ray's last record update (0: the record is the input)."""
    shape = rif.shape
    x, v = pos.clone(), vel.clone()
    xt, vt = pos.clone(), vel.clone()
    dist2 = ((x - target) ** 2).sum(-1)                                   # :200
    inside = inbounds(shape, h, x)                                        # :204
    esc = torch.zeros_like(inside)
    j = torch.zeros(len(pos), dtype=torch.long)
    for i in range(_max_steps(4.0, h, shape, ds)):                        # :192
        n, g = eval_grad(rif, x, h, inside)                               # :211
        v = v + (ds * n)[:, None] * g                                     # :213
        x = x + ds * v                                                    # :214
        cur = ((x - target) ** 2).sum(-1)                                 # :216
        closer = cur < dist2                                              # :217
        cur_inside = inbounds(shape, h, x)                                # :219
        cross = inside & ~cur_inside                                      # :220
        esc = esc | cross | escaped(shape, h, x, v)                       # :221-222
        xt = torch.where(closer[:, None], x, xt)                          # :225-227
        vt = torch.where(closer[:, None], v, vt)
        dist2 = torch.where(closer, cur, dist2)
        j = torch.where(closer, torch.full_like(j, i + 1), j)
        if bool(esc.all()):                                               # :229
            break
        inside = cur_inside                                               # :233
    return xt, vt, dist2, j
