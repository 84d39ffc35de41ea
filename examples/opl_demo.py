#!/usr/bin/env python3
"""Multi-view phase tomography from optical path lengths, every stage on the device: rays from
`source.rand_rays_in_sphere` (HIP generator), march + path length + adjoint through `tracer.OPLTracerC` (HIP kernels:
`trace_opl`, and ONE `backtrace_opl` launch per backward), Adam on the volume.

What an interferometer or a time-of-flight camera measures is the optical path length of each ray, the integral of n along
it.  The demo hides a weak medium (n = 1 + 3e-4 blob, the value range of a gas flow), records the path length of every ray
of a few fixed views, and recovers the field from those numbers alone: the loss is the mean squared difference of the path
lengths, in units of the medium's contrast.  No sensor image is formed.

    python examples/opl_demo.py [--res 33] [--views 6] [--side 48] [--iters 60]

Recorded on an MI355X (tests/test_opl.py::test_demo: 17^3, 3 views of 24^2 rays, 20 iterations): path-length loss
9.85e-3 -> 4.12e-5 (ratio 0.0042), rms(n - truth) 2.31e-5 -> 5.31e-6.
"""
from __future__ import annotations

import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from adjointnonlinearraytracing_amd import drrt, source, tracer

CONTRAST = 3e-4


def hidden_field(res: int, device) -> torch.Tensor:
    """Ground truth: an off-centre blob and a weaker second one, n in [1, 1 + 3e-4]."""
    g = torch.linspace(0.0, 1.0, res, device=device)
    z, y, x = torch.meshgrid(g, g, g, indexing="ij")
    b1 = torch.exp(-((x - 0.42) ** 2 + (y - 0.55) ** 2 + (z - 0.5) ** 2) / 0.02)
    b2 = torch.exp(-((x - 0.65) ** 2 + (y - 0.4) ** 2 + (z - 0.45) ** 2) / 0.01)
    return (1.0 + CONTRAST * (b1 + 0.6 * b2)).contiguous()


def path_lengths(n, rays, h, ds):
    """The optical path length of every ray through the field n (differentiable w.r.t. n)."""
    x, v, _ = rays
    return tracer.OPLTracerC.apply(n, x, v, h, ds)[2]


def run(res=33, views=6, side=48, iters=60, span=1.0, lr=2e-5, seed=0, verbose=True):
    dev = torch.device("cuda:0")
    torch.manual_seed(seed)
    truth = hidden_field(res, dev)
    h = span / (res - 1)
    ds = h / 2
    # the measurement is per ray, so the rays are drawn once: `views` plane sources turned about the z axis
    rays, _ = source.rand_rays_in_sphere(views, (side, side), 1, span, angle_span=180, circle=False, xaxis=False,
                                         sensor_dist=0.2 * span, device=dev)
    hist, err = [], []
    # the exact discrete adjoint (the 1/h of the gradient splat), for this thread's calls only
    with drrt.using(corrected_h=True):
        with torch.no_grad():
            measured = path_lengths(truth, rays, h, ds)
        n = torch.ones_like(truth).requires_grad_(True)
        opt = torch.optim.Adam([n], lr=lr)
        for it in range(iters):
            opt.zero_grad()
            loss = (((path_lengths(n, rays, h, ds) - measured) / CONTRAST) ** 2).mean()
            loss.backward()
            with torch.no_grad():
                for k in (0, -1):                           # boundary voxels stay fixed (core/optimizer.py:63)
                    n.grad[k, :, :] = 0; n.grad[:, k, :] = 0; n.grad[:, :, k] = 0
            opt.step()
            with torch.no_grad():
                n.clamp_(min=1.0)
                err.append(float(((n - truth) ** 2).mean().sqrt()))
            hist.append(float(loss.detach()))
            if verbose and (it % 10 == 0 or it == iters - 1):
                print(f"iter {it:3d}  path-length loss {hist[-1]:.5e}  rms(n - truth) {err[-1]:.3e}")
    return n.detach(), truth, hist, err


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=33)
    ap.add_argument("--views", type=int, default=6)
    ap.add_argument("--side", type=int, default=48)
    ap.add_argument("--iters", type=int, default=60)
    a = ap.parse_args()
    n, truth, hist, err = run(a.res, a.views, a.side, a.iters)
    print(f"path-length loss {hist[0]:.5e} -> {hist[-1]:.5e};  rms error {err[0]:.3e} -> {err[-1]:.3e}")
