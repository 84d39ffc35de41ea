"""Differentiable float64 torch restatement of trace with emission and self-absorption -- TEST INFRASTRUCTURE ONLY.

tests/field_ad.trace_field's loop with ``rad += exp(-tau) ds n e`` and then ``tau += ds n a`` per ray while the ray is not
yet flagged escaped, `e` and `a` the samples of the two fields from oracle/torch_ad.eval_grad with the same `inside` mask
as `n`, the exponential torch.exp.  Also returns the per-ray iteration count at which each ray was flagged (max_steps where
it never was)."""
import torch

from oracle.torch_ad import escaped, eval_grad, inbounds


def trace_emission(rif, emission, absorption, pos, vel, h, ds):
    """Differentiable w.r.t. rif, emission, absorption, pos, vel.  -> (xt, vt, rad, tau, steps)."""
    shape = rif.shape
    assert emission.shape == shape and absorption.shape == shape
    max_steps = int(4 * h * max(shape) / ds)
    x, v = pos.clone(), vel.clone()
    xt, vt = pos.clone(), vel.clone()
    tau = torch.zeros(pos.shape[0], dtype=pos.dtype, device=pos.device)
    rad = torch.zeros_like(tau)
    steps = torch.full((pos.shape[0],), max_steps, dtype=torch.int64, device=pos.device)
    inside = inbounds(shape, h, x)
    esc = torch.zeros_like(inside)
    for it in range(max_steps):
        n, g = eval_grad(rif, x, h, inside)
        e, _ = eval_grad(emission, x, h, inside)
        a, _ = eval_grad(absorption, x, h, inside)
        rad = rad + torch.where(esc, torch.zeros_like(n), torch.exp(-tau) * ds * n * e)
        tau = tau + torch.where(esc, torch.zeros_like(n), ds * n * a)
        v = v + (ds * n)[:, None] * g
        x = x + ds * v
        cur_inside = inbounds(shape, h, x)
        cross = inside & ~cur_inside
        now = (cross | escaped(shape, h, x, v)) & ~esc
        steps = torch.where(now, torch.full_like(steps, it + 1), steps)
        esc = esc | now
        xt = torch.where(cross[:, None], x, xt)
        vt = torch.where(cross[:, None], v, vt)
        if bool(esc.all()):
            break
        inside = cur_inside
    if not bool(esc.all()):
        xt = torch.where(esc[:, None], xt, x)
    return xt, vt, rad, tau, steps
