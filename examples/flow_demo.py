#!/usr/bin/env python3
"""Flow (vector) tomography through a refracting medium, every stage on the device: rays from `source.rand_rays_in_sphere`
(HIP generator), march + line integral of the flow along the ray's own direction + adjoint through
`tracer.VectorIntegralTracerC` (HIP kernels: `trace_vector`, and ONE `backtrace_vector` launch per backward), Adam on the
three components of the flow.

A Doppler or time-of-flight measurement through a moving fluid, or the Faraday rotation through a magnetised plasma, gives
per ray the line integral circ = int u . dl of a vector field projected on the ray -- along a ray that the medium's
refractive index bends.  The demo takes a KNOWN lens-like index n (a Luneburg-type ball, strong enough to bend the rays
visibly) and an UNKNOWN flow u, a vortex inside the lens, "measures" circ of every ray of a few fixed views with the true u,
and recovers u from those numbers alone: the loss is the mean squared difference of the line integrals.

Line integrals see only the solenoidal part of u: for a potential flow u = grad phi the integral is phi(exit) - phi(entry)
whatever happens in between, so the data say nothing about a curl-free part that vanishes on the boundary (and the discrete
sum telescopes in the same way: a uniform u gives u . (xt - x_e) exactly).  The hidden flow here is a vortex, which is
divergence-free; the error reported is that of the recovered field against it, and what the data cannot see stays at its
start, zero.

    python examples/flow_demo.py [--res 33] [--views 6] [--side 48] [--iters 60]

Recorded on an MI355X (tests/test_vector_integral.py::test_demo: 17^3, 3 views of 24^2 rays, 20 iterations): line-integral
loss 6.04e-3 -> 4.07e-4 (ratio 0.067), rms(u - truth) 0.065 -> 0.051 against an rms of the truth of 0.067; at the defaults
6.38e-3 -> 1.24e-3 and 0.070 -> 0.059.  A few views of longitudinal data leave most of the field undetermined: the loss falls
fast, the field follows slowly.
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


def hidden_flow(res: int, device) -> torch.Tensor:
    """Ground truth, shape (3, res, res, res), planes (ux, uy, uz) on the [z, y, x] grid: a vortex about an off-centre axis
    parallel to z, azimuthal speed rho exp(-rho^2 / s^2) shaped by a profile in z.  It has no z component and its azimuthal
    speed does not depend on the angle, so it is divergence-free."""
    z, y, x = _coords(res, device)
    dx, dy = x - 0.45, y - 0.55
    amp = 8.0 * torch.exp(-(dx ** 2 + dy ** 2) / 0.03) * torch.exp(-((z - 0.5) ** 2) / 0.08)
    return torch.stack([-dy * amp, dx * amp, torch.zeros_like(amp)]).contiguous()


def line_integrals(n, u, rays, h, ds):
    """circ = int u . dl of every ray bent by n (differentiable w.r.t. u, and n)."""
    x, v, _ = rays
    return tracer.VectorIntegralTracerC.apply(n, u, x, v, h, ds)[2]


def run(res=33, views=6, side=48, iters=60, span=1.0, lr=0.02, seed=0, verbose=True):
    dev = torch.device("cuda:0")
    torch.manual_seed(seed)
    n, truth = lens_index(res, dev), hidden_flow(res, dev)
    h = span / (res - 1)
    ds = h / 2
    # the measurement is per ray, so the rays are drawn once: `views` plane sources turned about the z axis
    rays, _ = source.rand_rays_in_sphere(views, (side, side), 1, span, angle_span=180, circle=False, xaxis=False,
                                         sensor_dist=0.2 * span, device=dev)
    hist, err = [], []
    with drrt.using(corrected_h=True):
        with torch.no_grad():
            measured = line_integrals(n, truth, rays, h, ds)
        u = torch.zeros_like(truth).requires_grad_(True)
        # eps well above the gradients of voxels that hardly any ray crosses: with Adam's default those take full steps on
        # noise and the field drifts away from the truth while the loss still falls
        opt = torch.optim.Adam([u], lr=lr, eps=1e-4)
        for it in range(iters):
            opt.zero_grad()
            loss = ((line_integrals(n, u, rays, h, ds) - measured) ** 2).mean()
            loss.backward()
            opt.step()
            with torch.no_grad():
                err.append(float(((u - truth) ** 2).mean().sqrt()))
            hist.append(float(loss.detach()))
            if verbose and (it % 10 == 0 or it == iters - 1):
                print(f"iter {it:3d}  line-integral loss {hist[-1]:.5e}  rms(u - truth) {err[-1]:.3e}")
    return u.detach(), truth, hist, err


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=33)
    ap.add_argument("--views", type=int, default=6)
    ap.add_argument("--side", type=int, default=48)
    ap.add_argument("--iters", type=int, default=60)
    p = ap.parse_args()
    u, truth, hist, err = run(p.res, p.views, p.side, p.iters)
    print(f"line-integral loss {hist[0]:.5e} -> {hist[-1]:.5e};  rms error {err[0]:.3e} -> {err[-1]:.3e}")
