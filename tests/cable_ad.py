"""Differentiable torch restatement of the cable (radial profile) forward march, for tests only: the recurrences of
cable_fwd_step (csrc/drrt_device.h) in whatever dtype its inputs have, so that torch.autograd in float64 gives reference
gradients w.r.t. the profiles AND the rays.  trace_cable is the march, trace_cable_opl adds the latched sum
opl = sum_{k < jstar} ds n_k^2, trace_cable_field the latched sum tau = sum_{k < jstar} ds n_k a_k of a second profile.

The record is selected with the per-ray iteration `jstar` handed in (0 = the input itself), not with a distance test of its
own: a float64 march cannot then pick another iteration than the fp32 march it is compared with, and the gradient holds
jstar fixed as the product does.  No escape logic is needed: the forward samples every iteration unmasked until it stops,
and jstar never lies beyond the stop."""
import torch


def _locate(rres, radius, x):
    """cyl_locate at the points x (n,3) on a profile of rres entries -> (h, xs, zs, tiny, r, i0, i1, w0).  The cell index
    is piecewise constant; within 1e-6 of the axis r is a constant (the product's r < eps branch)."""
    h = radius / (rres - 1)
    xs, zs = x[:, 0] - radius, x[:, 2] - radius
    r2 = xs * xs + zs * zs
    tiny = r2.detach().sqrt() < 1e-6
    r = torch.where(tiny, torch.zeros_like(r2), torch.sqrt(torch.where(tiny, torch.ones_like(r2), r2)))
    rm = r / h
    i0 = rm.detach().floor().long().clamp(0, rres - 1)
    i1 = (i0 + 1).clamp(0, rres - 1)
    w0 = rm - i0.to(rm.dtype)
    return h, xs, zs, tiny, r, i0, i1, w0


def sample(prof, radius, x):
    """n, and n grad n, at the points x (n,3) -- cyl_locate + the lerp of cable_fwd_step; rhat = 0 on the axis."""
    h, xs, zs, tiny, r, i0, i1, w0 = _locate(prof.shape[0], radius, x)
    v0, v1 = prof[i0], prof[i1]
    n = v1 * w0 + v0 * (1 - w0)
    rx = (v1 - v0) / h
    inv_r = torch.where(tiny, torch.zeros_like(r), 1 / torch.where(tiny, torch.ones_like(r), r))
    g = torch.stack([rx * xs * inv_r, torch.zeros_like(r), rx * zs * inv_r], 1)
    return n, n[:, None] * g


def sample_field(field, radius, x):
    """a at the points x (n,3): the lerp of the second profile `field` with sample's cell and weight."""
    _, _, _, _, _, i0, i1, w0 = _locate(field.shape[0], radius, x)
    return field[i1] * w0 + field[i0] * (1 - w0)


def _march(prof, radius, pos, vel, jstar, ds, summand=None):
    """-> (xt, vt, latched): the state after jstar[i] iterations of v += ds n grad n (sampled at x), x += ds v, and
    ``summand(n, x)`` summed over the samples in front of it (None without one)."""
    jstar = torch.as_tensor(jstar, dtype=torch.long)
    x, v = pos, vel
    xt, vt = pos, vel
    acc = latched = torch.zeros_like(pos[:, 0]) if summand else None
    for k in range(1, int(jstar.max()) + 1 if jstar.numel() else 1):
        n, ngn = sample(prof, radius, x)
        if summand:
            acc = acc + summand(n, x)
        v = v + ds * ngn
        x = x + ds * v
        sel = jstar == k
        xt = torch.where(sel[:, None], x, xt)
        vt = torch.where(sel[:, None], v, vt)
        if summand:
            latched = torch.where(sel, acc, latched)
    return xt, vt, latched


def trace_cable(prof, radius, length, pos, vel, jstar, ds):
    """-> (xt, vt): the state after jstar[i] iterations."""
    return _march(prof, radius, pos, vel, jstar, ds)[:2]


def trace_cable_opl(prof, radius, length, pos, vel, jstar, ds):
    """-> (xt, vt, opl): the state after jstar[i] iterations, and ds n^2 summed over the samples in front of it."""
    return _march(prof, radius, pos, vel, jstar, ds, lambda n, x: ds * n * n)


def trace_cable_field(prof, field, radius, length, pos, vel, jstar, ds):
    """-> (xt, vt, tau): the state after jstar[i] iterations, and ds n a summed over the samples in front of it, a the
    sample of `field` in n's own cell."""
    return _march(prof, radius, pos, vel, jstar, ds, lambda n, x: ds * n * sample_field(field, radius, x))
