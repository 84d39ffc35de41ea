"""Differentiable torch restatement of the fibre march with the line integral of a second radial profile, for tests only:
cable_opl_ad.trace_cable_opl with acc += ds n_k a_k, a_k the lerp of the second profile with the indices and the weight of
n_k's own cell (cable_ad.sample's), in whatever dtype its inputs have.  The record's iteration `jstar` is handed in, as in
cable_ad, so that a float64 run cannot pick another iteration than the fp32 march it is compared with, and the gradient
holds it fixed."""
import torch

import cable_ad


def sample_field(field, radius, x):
    """a at the points x (n,3): cable_ad.sample's cell and weight (cyl_locate: the index is piecewise constant, r is a
    constant within 1e-6 of the axis) on the profile `field`."""
    rres = field.shape[0]
    h = radius / (rres - 1)
    xs, zs = x[:, 0] - radius, x[:, 2] - radius
    r2 = xs * xs + zs * zs
    tiny = r2.detach().sqrt() < 1e-6
    r = torch.where(tiny, torch.zeros_like(r2), torch.sqrt(torch.where(tiny, torch.ones_like(r2), r2)))
    rm = r / h
    i0 = rm.detach().floor().long().clamp(0, rres - 1)
    i1 = (i0 + 1).clamp(0, rres - 1)
    w0 = rm - i0.to(rm.dtype)
    return field[i1] * w0 + field[i0] * (1 - w0)


def trace_cable_field(prof, field, radius, length, pos, vel, jstar, ds):
    """-> (xt, vt, tau): the state after jstar[i] iterations, and ds n a summed over the samples in front of it."""
    jstar = torch.as_tensor(jstar, dtype=torch.long)
    x, v = pos, vel
    xt, vt = pos, vel
    acc = torch.zeros_like(pos[:, 0])
    tau = acc
    for k in range(1, int(jstar.max()) + 1 if jstar.numel() else 1):
        n, ngn = cable_ad.sample(prof, radius, x)
        acc = acc + ds * n * sample_field(field, radius, x)
        v = v + ds * ngn
        x = x + ds * v
        sel = jstar == k
        xt = torch.where(sel[:, None], x, xt)
        vt = torch.where(sel[:, None], v, vt)
        tau = torch.where(sel, acc, tau)
    return xt, vt, tau
