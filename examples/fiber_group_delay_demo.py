#!/usr/bin/env python3
"""Equalise the GROUP delay of the rays guided by a graded-index fibre: `fiber_delay_demo.py` equalises the optical path
length int n dl, but the transit time that sets a fibre's modal dispersion is int N_g dl with the group index
N_g = n - lambda dn/dlambda -- a second radial profile integrated along rays that are bent by n.  That is
`tracer.CableFieldTracerC` (the HIP cable march with the line integral of a second profile, and its ONE exact adjoint for
both profiles and the rays).

The cone of `fiber_delay_demo.py`: rays leave an axis point just inside the entry face, scaled to |v| = n at their start, the
target lies far beyond the end face, so every ray's record is its first state past the end face.  The group index is
modelled as ``N_g(r) = n(r) + D (n(r) - n_cladding)`` and built in torch from the profile being optimised, so the profile's
gradient arrives through both of the operator's profile inputs (and through dL/dv).  The group delay to the end face is
``tau`` minus the overshoot ``n(xt) N_g(xt) (xt_y - length) / vt_y``; the loss is its variance over the rays that reach the
end face.  Adam, the cladding sample held fixed.

    python examples/fiber_group_delay_demo.py [--res 17] [--iters 200] [--rays 4096] [--cone 12] [--length 6] [--dispersion 0.5]

Prints the rms spread of the group delay at a few iterations, before and after, and the profile.
"""
from __future__ import annotations

import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch
import torch.optim as optim

from adjointnonlinearraytracing_amd import drrt, tracer
from fiber_delay_demo import cone_rays
from fiber_demo import radial_index


def group_index(nt, dispersion):
    """N_g(r) = n(r) + D (n(r) - n_cladding), the cladding sample a constant.  Differentiable w.r.t. the profile."""
    return nt + dispersion * (nt - nt[-1].detach())


def group_delays(nt, x, d, radius, length, dispersion):
    """-> (group delay to the end face per ray, mask of the rays that reach it).  Differentiable w.r.t. the profile `nt`."""
    sds = radius / nt.shape[0] / 2
    ng = group_index(nt, dispersion)
    v = d * radial_index(nt, radius, x)[:, None]                         # |v| = n: tau is the integral of N_g dl
    target = x + torch.tensor([0.0, 20.0 * length, 0.0], device=x.device)
    xt, vt, _, tau = tracer.CableFieldTracerC.apply(nt, ng, radius, length, x, v, target, sds)
    with torch.no_grad():
        reached = (xt[:, 1] > length) & (vt[:, 1] > 0) & (torch.hypot(xt[:, 0] - radius, xt[:, 2] - radius) < radius)
    vy = torch.where(reached, vt[:, 1], torch.ones_like(vt[:, 1]))
    return tau - radial_index(nt, radius, xt) * radial_index(ng, radius, xt) * (xt[:, 1] - length) / vy, reached


def run(res=17, iters=200, n_rays=4096, cone_deg=12.0, length=6.0, radius=1.0, lr=2e-3, dispersion=0.5, seed=0,
        verbose=True):
    """-> (profile, rms spread of the group delay per iteration, largest |profile gradient| per iteration)."""
    dev = torch.device("cuda:0")
    drrt.options.check_failed = False
    r = torch.linspace(0, 1, res, device=dev)
    n = (1.5 - 0.03 * r * r).requires_grad_(True)                         # a weak parabolic guide to start from
    opto = optim.Adam([n], lr=lr)
    x, d = cone_rays(n_rays, radius, radius / res / 2, cone_deg, dev, seed)
    hist, gmax = [], []
    for it in range(iters):
        opto.zero_grad()
        t, reached = group_delays(n, x, d, radius, length, dispersion)
        loss = t[reached].var()
        loss.backward()
        with torch.no_grad():
            n.grad[-1] = 0                                                # the cladding sample stays fixed
            gmax.append(float(n.grad.abs().max()))
        opto.step()
        hist.append(float(loss.detach().sqrt()))
        if verbose and it % 20 == 0:
            print(f"iter {it:4d}  rms spread {hist[-1]:.6f}  rays at the end face {int(reached.sum())}/{n_rays}")
    drrt.options.check_failed = True
    return n.detach(), hist, gmax


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=17)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rays", type=int, default=4096)
    ap.add_argument("--cone", type=float, default=12.0, help="half angle of the cone, degrees")
    ap.add_argument("--length", type=float, default=6.0)
    ap.add_argument("--dispersion", type=float, default=0.5, help="D of N_g = n + D (n - n_cladding)")
    a = ap.parse_args()
    n, hist, _ = run(a.res, a.iters, a.rays, a.cone, a.length, dispersion=a.dispersion)
    print(f"rms spread of the group delay {hist[0]:.6f} -> {hist[-1]:.6f};  profile (axis -> cladding): "
          + " ".join(f"{float(t):.4f}" for t in n[:: max(1, n.shape[0] // 8)]))
