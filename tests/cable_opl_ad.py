"""Differentiable torch restatement of the fibre march with its optical path length, for tests only: cable_ad.trace_cable
(the recurrences of cable_fwd_step in whatever dtype its inputs have) plus the latched sum opl = sum_{k < jstar} ds n_k^2,
n_k = cable_ad.sample's n at x_k.  The record's iteration `jstar` is handed in, as in cable_ad, so that a float64 run
cannot pick another iteration than the fp32 march it is compared with, and the gradient holds it fixed."""
import torch

import cable_ad


def trace_cable_opl(prof, radius, length, pos, vel, jstar, ds):
    """-> (xt, vt, opl): the state after jstar[i] iterations, and ds n^2 summed over the samples in front of it."""
    jstar = torch.as_tensor(jstar, dtype=torch.long)
    x, v = pos, vel
    xt, vt = pos, vel
    acc = torch.zeros_like(pos[:, 0])
    opl = acc
    for k in range(1, int(jstar.max()) + 1 if jstar.numel() else 1):
        n, ngn = cable_ad.sample(prof, radius, x)
        acc = acc + ds * n * n
        v = v + ds * ngn
        x = x + ds * v
        sel = jstar == k
        xt = torch.where(sel[:, None], x, xt)
        vt = torch.where(sel[:, None], v, vt)
        opl = torch.where(sel, acc, opl)
    return xt, vt, opl
