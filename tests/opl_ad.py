"""Differentiable float64 torch restatement of trace with its optical path length -- TEST INFRASTRUCTURE ONLY.

oracle/torch_ad.trace's loop (its eval_grad / inbounds / escaped) with ``opl += ds n^2`` per ray while the ray is not yet
flagged escaped: the march of the library ends a ray at the iteration that flags it, the array-at-a-time loop here goes on
while any ray marches, and a flagged ray's later samples (masked to 0 outside the box anyway) do not count.  Also returns
the per-ray iteration count at which each ray was flagged (max_steps where it never was)."""
import torch

from oracle.torch_ad import escaped, eval_grad, inbounds


def trace_opl(rif, pos, vel, h, ds):
    """Differentiable w.r.t. rif, pos, vel.  -> (xt, vt, opl, steps)."""
    shape = rif.shape
    max_steps = int(4 * h * max(shape) / ds)
    x, v = pos.clone(), vel.clone()
    xt, vt = pos.clone(), vel.clone()
    opl = torch.zeros(pos.shape[0], dtype=pos.dtype, device=pos.device)
    steps = torch.full((pos.shape[0],), max_steps, dtype=torch.int64, device=pos.device)
    inside = inbounds(shape, h, x)
    esc = torch.zeros_like(inside)
    for it in range(max_steps):
        n, g = eval_grad(rif, x, h, inside)
        opl = opl + torch.where(esc, torch.zeros_like(n), ds * n * n)
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
    return xt, vt, opl, steps
