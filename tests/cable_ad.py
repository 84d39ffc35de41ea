"""Differentiable torch restatement of the cable (radial profile) forward march, for tests only: the recurrences of
cable_fwd_step (csrc/drrt_device.h) in whatever dtype its inputs have, so that torch.autograd in float64 gives reference
gradients w.r.t. the profile AND the rays.

The record is selected with the per-ray iteration `jstar` handed in (0 = the input itself), not with a distance test of its
own: a float64 march cannot then pick another iteration than the fp32 march it is compared with, and the gradient holds
jstar fixed as the product does.  No escape logic is needed: the forward samples every iteration unmasked until it stops,
and jstar never lies beyond the stop."""
import torch


def sample(prof, radius, x):
    """n, and n grad n, at the points x (n,3) -- cyl_locate + the lerp of cable_fwd_step.  The cell index is piecewise
    constant; within 1e-6 of the axis rhat = 0 and r is a constant (the product's r < eps branch)."""
    rres = prof.shape[0]
    h = radius / (rres - 1)
    xs, zs = x[:, 0] - radius, x[:, 2] - radius
    r2 = xs * xs + zs * zs
    tiny = r2.detach().sqrt() < 1e-6
    r = torch.where(tiny, torch.zeros_like(r2), torch.sqrt(torch.where(tiny, torch.ones_like(r2), r2)))
    rm = r / h
    i0 = rm.detach().floor().long().clamp(0, rres - 1)
    i1 = (i0 + 1).clamp(0, rres - 1)
    w0 = rm - i0.to(rm.dtype)
    v0, v1 = prof[i0], prof[i1]
    n = v1 * w0 + v0 * (1 - w0)
    rx = (v1 - v0) / h
    inv_r = torch.where(tiny, torch.zeros_like(r), 1 / torch.where(tiny, torch.ones_like(r), r))
    g = torch.stack([rx * xs * inv_r, torch.zeros_like(r), rx * zs * inv_r], 1)
    return n, n[:, None] * g


def trace_cable(prof, radius, length, pos, vel, jstar, ds):
    """-> (xt, vt): the state after jstar[i] iterations of v += ds n grad n (sampled at x), x += ds v."""
    jstar = torch.as_tensor(jstar, dtype=torch.long)
    x, v = pos, vel
    xt, vt = pos, vel
    for k in range(1, int(jstar.max()) + 1 if jstar.numel() else 1):
        _, ngn = sample(prof, radius, x)
        v = v + ds * ngn
        x = x + ds * v
        sel = (jstar == k)[:, None]
        xt = torch.where(sel, x, xt)
        vt = torch.where(sel, v, vt)
    return xt, vt
