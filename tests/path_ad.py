"""Differentiable float64 torch restatement of trace with its path -- TEST INFRASTRUCTURE ONLY.

tests/opl_ad.trace_opl's loop (oracle/torch_ad's eval_grad / inbounds / escaped), recording the marching position x in front
of every iteration that is a multiple of `stride`, `samples` = M entries at most.  The per-ray count
``min(M, ceil(steps / stride))`` is known behind the loop; the entries at and behind it are replaced by xt with
``torch.where``, so autograd sees xt there and x_{j stride} in front of it.  The array-at-a-time loop ends when every ray is
flagged; the entries it has not reached then belong to no ray's samples (j stride >= steps for every ray) and are padding."""
import torch

from oracle.torch_ad import escaped, eval_grad, inbounds


def trace_path(rif, pos, vel, h, ds, stride, samples):
    """Differentiable w.r.t. rif, pos, vel.  -> (xt, vt, path (samples, n, 3), count, steps)."""
    shape = rif.shape
    max_steps = int(4 * h * max(shape) / ds)
    x, v = pos.clone(), vel.clone()
    xt, vt = pos.clone(), vel.clone()
    steps = torch.full((pos.shape[0],), max_steps, dtype=torch.int64, device=pos.device)
    inside = inbounds(shape, h, x)
    esc = torch.zeros_like(inside)
    rec = []
    for it in range(max_steps):
        if it % stride == 0 and len(rec) < samples:
            rec.append(x)
        n, g = eval_grad(rif, x, h, inside)
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
    count = torch.clamp((steps + stride - 1) // stride, max=samples)
    rows = []
    for j in range(samples):
        rows.append(torch.where((j < count)[:, None], rec[j], xt) if j < len(rec) else xt)
    return xt, vt, torch.stack(rows), count, steps
