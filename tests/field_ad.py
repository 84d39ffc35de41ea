"""Differentiable float64 torch restatement of trace with the line integral of a second field -- TEST INFRASTRUCTURE ONLY.

tests/opl_ad.trace_opl's loop with ``tau += ds n a`` per ray while the ray is not yet flagged escaped, `a` the sample of the
field from oracle/torch_ad.eval_grad with the same `inside` mask as `n`.  Also returns the per-ray iteration count at which
each ray was flagged (max_steps where it never was)."""
import torch

from oracle.torch_ad import escaped, eval_grad, inbounds


def trace_field(rif, field, pos, vel, h, ds):
    """Differentiable w.r.t. rif, field, pos, vel.  -> (xt, vt, tau, steps)."""
    shape = rif.shape
    assert field.shape == shape
    max_steps = int(4 * h * max(shape) / ds)
    x, v = pos.clone(), vel.clone()
    xt, vt = pos.clone(), vel.clone()
    tau = torch.zeros(pos.shape[0], dtype=pos.dtype, device=pos.device)
    steps = torch.full((pos.shape[0],), max_steps, dtype=torch.int64, device=pos.device)
    inside = inbounds(shape, h, x)
    esc = torch.zeros_like(inside)
    for it in range(max_steps):
        n, g = eval_grad(rif, x, h, inside)
        a, _ = eval_grad(field, x, h, inside)
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
    return xt, vt, tau, steps
