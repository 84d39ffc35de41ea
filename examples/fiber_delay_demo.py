#!/usr/bin/env python3
"""Equalise the transit time of the rays guided by a graded-index fibre: optimise the RADIAL index profile so that the
optical path length from an axis point on the entry face to the end face is the same for every ray of a cone -- the modal
dispersion that grading a profile is meant to remove.  Where `fiber_demo.py` optimises where rays land, this one optimises
when they arrive: `tracer.CableOPLTracerC` (the HIP cable march with its optical path length, and its ONE exact adjoint for
the profile and the rays).

Rays leave an axis point just inside the entry face in a cone, scaled to |v| = n at their start (so that the march's
``opl = sum ds n^2`` is the integral of n along the path; the scale depends on the profile, and that gradient reaches the
profile through dL/dv).  The target lies far beyond the end face, so every ray's record is its last state, the first one
past the end face.  The transit time to the end face is ``opl`` minus the overshoot ``n(xt)^2 (xt_y - length) / vt_y``,
formed in torch from the differentiable outputs; the loss is the variance of that time over the rays that reach the end
face (rays that leave through the cladding drop out of the loss).  Adam, the cladding sample held fixed.

    python examples/fiber_delay_demo.py [--res 17] [--iters 200] [--rays 4096] [--cone 12] [--length 6]

Prints the rms spread of the transit time before and after, and the profile.
"""
from __future__ import annotations

import argparse
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch
import torch.optim as optim

from adjointnonlinearraytracing_amd import drrt, tracer
from fiber_demo import radial_index


def cone_rays(n_rays: int, radius: float, ds: float, cone_deg: float, device, seed: int = 0):
    """Unit directions in a cone of half angle `cone_deg` about +y (uniform in solid angle), from the axis point just inside
    the entry face -> (x, d), (n,3) each."""
    g = torch.Generator().manual_seed(seed)
    cos_t = 1.0 - torch.rand(n_rays, generator=g) * (1.0 - math.cos(math.radians(cone_deg)))
    sin_t = torch.sqrt(1.0 - cos_t * cos_t)
    phi = torch.rand(n_rays, generator=g) * (2.0 * math.pi)
    d = torch.stack([sin_t * torch.cos(phi), cos_t, sin_t * torch.sin(phi)], 1)
    x = torch.tensor([radius, 0.37 * ds, radius]).repeat(n_rays, 1)
    return x.to(device), d.to(device)


def transit_times(nt, x, d, radius, length):
    """-> (time to the end face per ray, mask of the rays that reach it).  Differentiable w.r.t. the profile `nt`."""
    sds = radius / nt.shape[0] / 2
    v = d * radial_index(nt, radius, x)[:, None]                         # |v| = n: opl is the integral of n dl
    target = x + torch.tensor([0.0, 20.0 * length, 0.0], device=x.device)
    xt, vt, _, opl = tracer.CableOPLTracerC.apply(nt, radius, length, x, v, target, sds)
    with torch.no_grad():
        reached = (xt[:, 1] > length) & (vt[:, 1] > 0) & (torch.hypot(xt[:, 0] - radius, xt[:, 2] - radius) < radius)
    n_end = radial_index(nt, radius, xt)
    vy = torch.where(reached, vt[:, 1], torch.ones_like(vt[:, 1]))
    return opl - n_end * n_end * (xt[:, 1] - length) / vy, reached


def run(res=17, iters=200, n_rays=4096, cone_deg=12.0, length=6.0, radius=1.0, lr=2e-3, seed=0, verbose=True):
    """-> (profile, rms spread of the transit time per iteration, largest |profile gradient| per iteration)."""
    dev = torch.device("cuda:0")
    drrt.options.check_failed = False
    r = torch.linspace(0, 1, res, device=dev)
    n = (1.5 - 0.03 * r * r).requires_grad_(True)                         # a weak parabolic guide to start from
    opto = optim.Adam([n], lr=lr)
    x, d = cone_rays(n_rays, radius, radius / res / 2, cone_deg, dev, seed)
    hist, gmax = [], []
    for it in range(iters):
        opto.zero_grad()
        t, reached = transit_times(n, x, d, radius, length)
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
    a = ap.parse_args()
    n, hist, _ = run(a.res, a.iters, a.rays, a.cone, a.length)
    print(f"rms spread of the transit time {hist[0]:.6f} -> {hist[-1]:.6f};  profile (axis -> cladding): "
          + " ".join(f"{float(t):.4f}" for t in n[:: max(1, n.shape[0] // 8)]))
