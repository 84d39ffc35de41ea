#!/usr/bin/env python3
"""Emission tomography of a self-absorbing blob behind a lens, every stage on the device: rays from
`source.rand_rays_in_sphere` (HIP generator), march + radiative-transfer integral + adjoint through
`tracer.EmissionTracerC` (HIP kernels: `trace_emission`, and ONE `backtrace_emission` launch per backward), Adam on the
emission and the absorption coefficient together.

A flame, a hot jet or a fluorescing volume emits light along rays that its own refractive index bends, and absorbs part of
it on the way out: a camera pixel records rad = int e(s) exp(-int_0^s a) ds, not a plain line integral.  The demo takes a
KNOWN lens-like index n (a Luneburg-type ball, strong enough to bend the rays visibly), an UNKNOWN non-negative emission e
and an UNKNOWN non-negative absorption a that follows the same blob, "measures" the radiance of every ray of a few fixed
views with the true fields, and recovers e and a jointly from those images alone: the loss is the mean squared difference
of the radiances.  The views go all the way round (an even number of them face each other in pairs), which is what
separates the two fields: opposite pixels see the same emitters through different amounts of absorber.

    python examples/emission_demo.py [--res 33] [--views 6] [--side 48] [--iters 80]

Recorded on an MI355X.  tests/test_emission.py::test_demo (17^3, 3 views of 24^2 rays, 20 iterations): radiance loss
2.53e-2 -> 6.29e-4 (ratio 0.025), rms(e - truth) 0.215 -> 0.158, rms(a - truth) 0.278 -> 0.539.  The default run (33^3,
6 views of 48^2 rays, 80 iterations): radiance loss 2.52e-2 -> 3.16e-5, rms(e - truth) 0.224 -> 0.120, rms(a - truth)
0.291 -> 0.639.  The images are fitted and the emitter is found; the absorber is not separated from a dimmer emitter by
these few views and plain Adam (presumably because a dimmer e and a smaller a give nearly the same images), so its error grows while the
loss falls: the demo shows the operator and both gradients at work, not a regularised reconstruction.
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


def hidden_fields(res: int, device):
    """Ground truth: an off-centre emitting blob and a weaker second one, e in [0, 3] per unit length, and an absorber that
    is strongest in the first blob, a in [0, 4] per unit length (optical depth about 1 across it)."""
    z, y, x = _coords(res, device)
    b1 = torch.exp(-((x - 0.42) ** 2 + (y - 0.55) ** 2 + (z - 0.5) ** 2) / 0.02)
    b2 = torch.exp(-((x - 0.65) ** 2 + (y - 0.4) ** 2 + (z - 0.45) ** 2) / 0.01)
    return (3.0 * (b1 + 0.6 * b2)).contiguous(), (4.0 * b1 + 1.0 * b2).contiguous()


def radiances(n, e, a, rays, h, ds):
    """rad = int e exp(-int a) of every ray bent by n (differentiable w.r.t. e, a, and n)."""
    x, v, _ = rays
    return tracer.EmissionTracerC.apply(n, e, a, x, v, h, ds)[2]


def run(res=33, views=6, side=48, iters=80, span=1.0, lr=0.05, seed=0, verbose=True):
    """-> (e, a), (e truth, a truth), the loss history, and per iteration (rms(e - truth), rms(a - truth))."""
    dev = torch.device("cuda:0")
    torch.manual_seed(seed)
    n = lens_index(res, dev)
    e_true, a_true = hidden_fields(res, dev)
    h = span / (res - 1)
    ds = h / 2
    # the measurement is per ray, so the rays are drawn once: `views` plane sources turned about the z axis, all the way round
    rays, _ = source.rand_rays_in_sphere(views, (side, side), 1, span, angle_span=360, circle=False, xaxis=False,
                                         sensor_dist=0.2 * span, device=dev)
    hist, err = [], []
    with drrt.using(corrected_h=True):
        with torch.no_grad():
            measured = radiances(n, e_true, a_true, rays, h, ds)
        e = torch.zeros_like(e_true).requires_grad_(True)
        a = torch.zeros_like(a_true).requires_grad_(True)
        opt = torch.optim.Adam([e, a], lr=lr)
        for it in range(iters):
            opt.zero_grad()
            loss = ((radiances(n, e, a, rays, h, ds) - measured) ** 2).mean()
            loss.backward()
            opt.step()
            with torch.no_grad():
                e.clamp_(min=0.0)                          # neither coefficient is negative
                a.clamp_(min=0.0)
                err.append((float(((e - e_true) ** 2).mean().sqrt()), float(((a - a_true) ** 2).mean().sqrt())))
            hist.append(float(loss.detach()))
            if verbose and (it % 10 == 0 or it == iters - 1):
                print(f"iter {it:3d}  radiance loss {hist[-1]:.5e}  rms(e - truth) {err[-1][0]:.3e}  rms(a - truth) {err[-1][1]:.3e}")
    return (e.detach(), a.detach()), (e_true, a_true), hist, err


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=33)
    ap.add_argument("--views", type=int, default=6)
    ap.add_argument("--side", type=int, default=48)
    ap.add_argument("--iters", type=int, default=80)
    p = ap.parse_args()
    _, _, hist, err = run(p.res, p.views, p.side, p.iters)
    print(f"radiance loss {hist[0]:.5e} -> {hist[-1]:.5e};  rms error e {err[0][0]:.3e} -> {err[-1][0]:.3e}, "
          f"a {err[0][1]:.3e} -> {err[-1][1]:.3e}")
