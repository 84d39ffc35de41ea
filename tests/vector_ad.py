"""Differentiable float64 torch restatement of trace with the line integral of a vector field -- TEST INFRASTRUCTURE ONLY.

tests/field_ad.trace_field's loop with ``circ += ds u(x_k) . v_{k+1}`` per ray while the ray is not yet flagged escaped: `u`
the samples of the three component planes ``vfield[c]`` (shape ``(3,) + rif.shape``; plane c pairs with component c of pos /
vel) from oracle/torch_ad.eval_grad with the same `inside` mask as `n`, and v_{k+1} the velocity BEHIND the update from sample
k, the one that carries the ray from x_k to x_{k+1}.  Also returns the per-ray iteration count at which each ray was flagged
(max_steps where it never was) and the per-ray scale ``S = sum ds (|ux vx| + |uy vy| + |uz vz|)`` of the same summands: circ
cancels, S does not, so an error of circ is measured against S."""
import torch

from oracle.torch_ad import escaped, eval_grad, inbounds


def trace_vector(rif, vfield, pos, vel, h, ds, extent=False):
    """Differentiable w.r.t. rif, vfield, pos, vel.  -> (xt, vt, circ, steps, S), and with `extent` a sixth result: per ray
    and axis, the largest |x_c| among the positions x_k, x_{k+1} of the iterations that sampled inside the box (0 for a ray
    that never did)."""
    shape = rif.shape
    assert tuple(vfield.shape) == (3,) + tuple(shape)
    max_steps = int(4 * h * max(shape) / ds)
    x, v = pos.clone(), vel.clone()
    xt, vt = pos.clone(), vel.clone()
    circ = torch.zeros(pos.shape[0], dtype=pos.dtype, device=pos.device)
    scale = torch.zeros_like(circ)
    reach = torch.zeros_like(pos)
    steps = torch.full((pos.shape[0],), max_steps, dtype=torch.int64, device=pos.device)
    inside = inbounds(shape, h, x)
    esc = torch.zeros_like(inside)
    for it in range(max_steps):
        n, g = eval_grad(rif, x, h, inside)
        u = torch.stack([eval_grad(vfield[c], x, h, inside)[0] for c in range(3)], 1)
        v = v + (ds * n)[:, None] * g
        term = u * v
        circ = circ + torch.where(esc, torch.zeros_like(n), ds * term.sum(1))
        scale = scale + torch.where(esc, torch.zeros_like(n), ds * term.abs().sum(1))
        live = (inside & ~esc)[:, None]
        reach = torch.where(live, torch.maximum(reach, x.detach().abs()), reach)
        x = x + ds * v
        reach = torch.where(live, torch.maximum(reach, x.detach().abs()), reach)
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
    if extent:
        return xt, vt, circ, steps, scale.detach(), reach
    return xt, vt, circ, steps, scale.detach()
