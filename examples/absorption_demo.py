#!/usr/bin/env python3
"""Absorption tomography through a refracting medium, every stage on the device: rays from `source.rand_rays_in_sphere`
(HIP generator), march + line integral + adjoint through `tracer.FieldIntegralTracerC` (HIP kernels: `trace_field`, and ONE
`backtrace_field` launch per backward), Adam on the absorption coefficient.

A flame, a mixing fluid or a piece of graded glass absorbs light along rays that its refractive index bends.  The demo
takes a KNOWN lens-like index n (a Luneburg-type ball, strong enough to bend the rays visibly) and an UNKNOWN non-negative
absorption coefficient a, "measures" the optical depth tau = int a dl of every ray of a few fixed views with the true a,
and recovers a from those numbers alone: the loss is the mean squared difference of the optical depths.  Straight-ray
tomography would put the absorption in the wrong voxels here; the adjoint spreads each residual along the bent path.

    python examples/absorption_demo.py [--res 33] [--views 6] [--side 48] [--iters 60]

Recorded on an MI355X (tests/test_field_integral.py::test_demo: 17^3, 3 views of 24^2 rays, 20 iterations): optical-depth
loss 2.06e-2 -> 5.28e-4 (ratio 0.026), rms(a - truth) 0.143 -> 0.092.
"""
from __future__ import annotations

import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from adjointnonlinearraytracing_amd import drrt, source, tracer


def _coords(res: int, device):
    g = torch.linspace(0.0, 1.0, res, device=device)
    return torch.meshgrid(g, g, g, indexing="ij")


def lens_index(res: int, device) -> torch.Tensor:
    """The known medium: n = sqrt(2 - (r / R)^2) inside a ball of radius R = 0.4 about the centre, 1 outside."""
    z, y, x = _coords(res, device)
    r = torch.sqrt((x - 0.5) ** 2 + (y - 0.5) ** 2 + (z - 0.5) ** 2) / 0.4
    return torch.sqrt(2.0 - torch.clamp(r, max=1.0) ** 2).contiguous()


def hidden_absorption(res: int, device) -> torch.Tensor:
    """Ground truth: an off-centre blob and a weaker second one, a in [0, 2] per unit length."""
    z, y, x = _coords(res, device)
    b1 = torch.exp(-((x - 0.42) ** 2 + (y - 0.55) ** 2 + (z - 0.5) ** 2) / 0.02)
    b2 = torch.exp(-((x - 0.65) ** 2 + (y - 0.4) ** 2 + (z - 0.45) ** 2) / 0.01)
    return (2.0 * (b1 + 0.6 * b2)).contiguous()


def optical_depths(n, a, rays, h, ds):
    """tau = int a dl of every ray bent by n (differentiable w.r.t. a, and n)."""
    x, v, _ = rays
    return tracer.FieldIntegralTracerC.apply(n, a, x, v, h, ds)[2]


def run(res=33, views=6, side=48, iters=60, span=1.0, lr=0.05, seed=0, verbose=True):
    dev = torch.device("cuda:0")
    torch.manual_seed(seed)
    n, truth = lens_index(res, dev), hidden_absorption(res, dev)
    h = span / (res - 1)
    ds = h / 2
    # the measurement is per ray, so the rays are drawn once: `views` plane sources turned about the z axis
    rays, _ = source.rand_rays_in_sphere(views, (side, side), 1, span, angle_span=180, circle=False, xaxis=False,
                                         sensor_dist=0.2 * span, device=dev)
    hist, err = [], []
    with drrt.using(corrected_h=True):
        with torch.no_grad():
            measured = optical_depths(n, truth, rays, h, ds)
        a = torch.zeros_like(truth).requires_grad_(True)
        opt = torch.optim.Adam([a], lr=lr)
        for it in range(iters):
            opt.zero_grad()
            loss = ((optical_depths(n, a, rays, h, ds) - measured) ** 2).mean()
            loss.backward()
            opt.step()
            with torch.no_grad():
                a.clamp_(min=0.0)                          # an absorption coefficient is not negative
                err.append(float(((a - truth) ** 2).mean().sqrt()))
            hist.append(float(loss.detach()))
            if verbose and (it % 10 == 0 or it == iters - 1):
                print(f"iter {it:3d}  optical-depth loss {hist[-1]:.5e}  rms(a - truth) {err[-1]:.3e}")
    return a.detach(), truth, hist, err


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=33)
    ap.add_argument("--views", type=int, default=6)
    ap.add_argument("--side", type=int, default=48)
    ap.add_argument("--iters", type=int, default=60)
    p = ap.parse_args()
    a, truth, hist, err = run(p.res, p.views, p.side, p.iters)
    print(f"optical-depth loss {hist[0]:.5e} -> {hist[-1]:.5e};  rms error {err[0]:.3e} -> {err[-1]:.3e}")
