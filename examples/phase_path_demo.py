#!/usr/bin/env python3
"""Two uses of ray paths with velocities (`tracer.PhasePathTracerC`): what positions alone cannot do.

(1) A direction-dependent integrand written in torch.  The line integral int u . dl of an analytic solenoidal flow -- a
    Gaussian vortex about the z axis of the box, given as a function, not as a grid -- is summed along rays bent by a
    Luneburg ball as sum_j (ds stride) u(path[j]) . vpath[j] over the samples inside the box.  It is printed next to
    `tracer.VectorIntegralTracerC` on the same flow voxelised on the grid of the ball (which sums ds u(x_k) . v_{k+1} over
    every iteration), with their difference and with the gradient of the sum w.r.t. the index grid, which reaches it
    through the sample positions AND the sample directions.

(2) A design loss on directions at depth.  A bundle entering a block through its y = 0 face is to travel along a given
    axis when it reaches one intermediate sample index: the mean squared difference between the unit vector of `vpath`
    there and the axis is minimised over the index grid, with the masked Adam and the clamp at 1 of
    `optimizer.multires_opt`, as examples/path_demo.py.

    python examples/phase_path_demo.py [--res 33] [--side 24] [--iters 60]

Each part prints what it reaches; nothing is claimed beyond the printout.
"""
from __future__ import annotations

import argparse
import math
import os
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch
from adjointnonlinearraytracing_amd import optimizer, tracer
from path_demo import luneburg, plane_bundle


def direction_integrand(res=33, side=24, stride=2, verbose=True):
    """-> dict(circ_path, circ_grid (each the largest |circ| over the rays), diff, grad_norm, samples, count_max)"""
    dev = torch.device("cuda:0")
    span, h, ds = float(res - 1), 1.0, 0.5
    rif = luneburg(res, dev).requires_grad_(True)
    cx, cy = 0.55 * span, 0.5 * span
    amp, sigma = 0.05, 0.25 * span

    def flow(p):                                               # a vortex about the z axis through (cx, cy): div u = 0
        x, y = p[..., 0] - cx, p[..., 1] - cy
        f = amp * torch.exp(-(x * x + y * y) / (2 * sigma ** 2))
        return torch.stack([-f * y, f * x, torch.zeros_like(f)], -1)

    pos, vel = plane_bundle(side, 0.15 * span, 0.85 * span, -0.25, dev)
    _, _, path, vpath, count = tracer.PhasePathTracerC.apply(rif, pos, vel, h, ds, stride, None)
    live = torch.arange(path.shape[0], device=dev)[:, None] < count[None, :]               # the samples; padding repeats (xt, vt)
    inbox = ((path >= 0) & (path <= span)).all(-1)                                         # where the march samples
    circ_path = ((flow(path) * vpath).sum(-1) * (live & inbox)).sum(0) * (ds * stride)
    circ_path.abs().sum().backward()
    grad_norm = float(rif.grad.norm())
    with torch.no_grad():
        i = torch.arange(res, dtype=torch.float32, device=dev) * h
        grid_pts = torch.stack(torch.meshgrid(i, i, i, indexing="ij")[::-1], -1)           # axis order of the grid: z, y, x
        vfield = flow(grid_pts).permute(3, 0, 1, 2).contiguous()
        circ_grid = tracer.VectorIntegralTracerC.apply(rif.detach(), vfield, pos, vel, h, ds)[2]
        diff = float((circ_path - circ_grid).abs().max())
    out = dict(circ_path=float(circ_path.detach().abs().max()), circ_grid=float(circ_grid.abs().max()), diff=diff, grad_norm=grad_norm,
               samples=int(path.shape[0]), count_max=int(count.max()))
    if verbose:
        print(f"(1) {side * side} rays through a Luneburg ball of {res}^3, {out['samples']} samples of position and velocity "
              f"per ray (stride {stride}, at most {out['count_max']} in use)")
        print(f"    int u . dl of the analytic vortex: max |sum on (path, vpath)| {out['circ_path']:.4e}, max "
              f"|VectorIntegralTracerC on the voxelised vortex| {out['circ_grid']:.4e}, max |difference| {diff:.3e}")
        print(f"    |d sum|circ| / d rif| = {grad_norm:.3e} (through the sample positions and directions)")
    return out


def steer(res=33, side=12, iters=60, stride=2, lr=5e-3, tilt_deg=8.0, verbose=True):
    """-> the loss history of the steering design."""
    dev = torch.device("cuda:0")
    span, h, ds = float(res - 1), 1.0, 0.5
    pos, vel = plane_bundle(side, 0.3 * span, 0.7 * span, -0.25, dev)
    t = math.radians(tilt_deg)
    axis = torch.tensor([math.sin(t), math.cos(t), 0.0], device=dev)
    at = int(0.6 * span / (ds * stride))                       # the sample index: about 0.6 of the way through the block

    def loss_of(n):
        _, _, _, vpath, count = tracer.PhasePathTracerC.apply(n, pos, vel, h, ds, stride, None)
        v = vpath[at]
        unit = v / v.norm(dim=-1, keepdim=True)
        return ((unit - axis) ** 2).sum(-1).mean()

    with tempfile.TemporaryDirectory() as tmp:
        n, hist = optimizer.multires_opt(loss_of, torch.ones((res,) * 3, device=dev), iters, [res], lr=lr,
                                         statename=os.path.join(tmp, "state.pt"))
    if verbose:
        print(f"(2) {side * side} rays steered to travel along ({axis[0]:.3f}, {axis[1]:.3f}, 0) at sample {at}: mean |unit(v) - "
              f"axis|^2 {hist[0]:.4e} -> {hist[-1]:.4e} in {len(hist)} Adam steps; n in [{float(n.detach().min()):.3f}, "
              f"{float(n.detach().max()):.3f}]")
    return hist


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=33)
    ap.add_argument("--side", type=int, default=24)
    ap.add_argument("--iters", type=int, default=60)
    a = ap.parse_args()
    direction_integrand(a.res, a.side)
    steer(a.res, max(a.side // 2, 2), a.iters)
