#!/usr/bin/env python3
"""Absorption tomography from sensor IMAGES through a refracting medium, every stage on the device: a plane source per
view (`source.rand_rays_in_sphere`, HIP generator), march + line integral + adjoint through `tracer.FieldIntegralTracerC`,
`sensor.trace_rays_to_plane`, and the radiance splat `sensor.splat_radiance` (HIP kernels `k_sensor_radiance` and ONE
`k_sensor_radiance_bwd` launch per backward), Adam on the absorption coefficients.

A shadowgraph of an absorbing, refracting medium is the splat of exp(-tau_i) at the bent ray's landing point.  The demo
takes a KNOWN lens-like index n (a Luneburg-type ball) and two UNKNOWN non-negative absorption coefficients -- two
spectral bands, say --, renders the two-channel shadowgraphs of a few views with the true coefficients, and recovers
both fields from those images alone: the loss is the mean squared difference of the images.  examples/absorption_demo.py
puts its loss on the per-ray optical depths; here the measurement is what a camera records, and the gradient reaches
the fields through the energy argument of the splat (`rad = exp(-tau)`, C = 2), which generate_sensor refuses.

    python examples/shadowgraph_demo.py [--res 17] [--views 4] [--side 48] [--nbins 24] [--iters 60]

Recorded on an MI355X with the defaults: image loss 2.07e-1 -> 6.35e-4, rms(a - truth) 0.140 -> 0.082.
"""
from __future__ import annotations

import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from adjointnonlinearraytracing_amd import drrt, sensor, source, tracer


def _coords(res: int, device):
    g = torch.linspace(0.0, 1.0, res, device=device)
    return torch.meshgrid(g, g, g, indexing="ij")


def lens_index(res: int, device) -> torch.Tensor:
    """The known medium: n = sqrt(2 - (r / R)^2) inside a ball of radius R = 0.4 about the centre, 1 outside."""
    z, y, x = _coords(res, device)
    r = torch.sqrt((x - 0.5) ** 2 + (y - 0.5) ** 2 + (z - 0.5) ** 2) / 0.4
    return torch.sqrt(2.0 - torch.clamp(r, max=1.0) ** 2).contiguous()


def hidden_absorbers(res: int, device) -> torch.Tensor:
    """Ground truth (2, res, res, res): an off-centre blob and a weaker one in the first band, one blob elsewhere in the
    second; a in [0, 2] per unit length."""
    z, y, x = _coords(res, device)
    b1 = torch.exp(-((x - 0.42) ** 2 + (y - 0.55) ** 2 + (z - 0.5) ** 2) / 0.02)
    b2 = torch.exp(-((x - 0.65) ** 2 + (y - 0.4) ** 2 + (z - 0.45) ** 2) / 0.01)
    b3 = torch.exp(-((x - 0.55) ** 2 + (y - 0.45) ** 2 + (z - 0.6) ** 2) / 0.03)
    return torch.stack([2.0 * (b1 + 0.6 * b2), 1.5 * b3]).contiguous()


def shadowgraphs(n, fields, rays, views, h, ds, nbins, span):
    """(views, 2, nbins, nbins): per view the image of rad = exp(-tau), one channel per absorption field, splatted where
    the rays bent by n meet the view's sensor plane (differentiable w.r.t. the fields, and n)."""
    x, v, planes = rays
    marches = [tracer.FieldIntegralTracerC.apply(n, a, x, v, h, ds) for a in fields]
    xt, vt = marches[0][:2]                                    # the same bent rays for both fields
    rad = torch.stack([torch.exp(-m[2]) for m in marches], 1)
    xp, vp = sensor.trace_rays_to_plane((xt, vt), (planes[:, 0, :], planes[:, 1, :]))
    per = x.shape[0] // views                                  # the views' rays follow each other
    imgs = []
    for k in range(views):
        s, first = slice(k * per, (k + 1) * per), planes[None, k * per]
        imgs.append(sensor.splat_radiance((xp[s], vp[s]), rad[s], (first[:, 0], first[:, 1]), nbins, span, first[:, 2]))
    return torch.stack(imgs)


def run(res=17, views=4, side=48, nbins=24, iters=60, span=1.0, lr=0.05, seed=0, verbose=True):
    dev = torch.device("cuda:0")
    torch.manual_seed(seed)
    n, truth = lens_index(res, dev), hidden_absorbers(res, dev)
    h = span / (res - 1)
    ds = h / 2
    # the rays are drawn once: `views` plane sources turned about the z axis, (side / nbins)^2 rays per sensor pixel
    rays, _ = source.rand_rays_in_sphere(views, (side, side), 1, span, angle_span=180, circle=False, xaxis=False,
                                         sensor_dist=0.2 * span, device=dev)
    hist, err = [], []
    with drrt.using(corrected_h=True):
        with torch.no_grad():
            measured = shadowgraphs(n, truth, rays, views, h, ds, nbins, span)
        a = torch.zeros_like(truth).requires_grad_(True)
        opt = torch.optim.Adam([a], lr=lr)
        for it in range(iters):
            opt.zero_grad()
            loss = ((shadowgraphs(n, a, rays, views, h, ds, nbins, span) - measured) ** 2).mean()
            loss.backward()
            opt.step()
            with torch.no_grad():
                a.clamp_(min=0.0)                              # an absorption coefficient is not negative
                err.append(float(((a - truth) ** 2).mean().sqrt()))
            hist.append(float(loss.detach()))
            if verbose and (it % 10 == 0 or it == iters - 1):
                print(f"iter {it:3d}  image loss {hist[-1]:.5e}  rms(a - truth) {err[-1]:.3e}")
    return a.detach(), truth, hist, err


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=17)
    ap.add_argument("--views", type=int, default=4)
    ap.add_argument("--side", type=int, default=48)
    ap.add_argument("--nbins", type=int, default=24)
    ap.add_argument("--iters", type=int, default=60)
    p = ap.parse_args()
    a, truth, hist, err = run(p.res, p.views, p.side, p.nbins, p.iters)
    print(f"image loss {hist[0]:.5e} -> {hist[-1]:.5e};  rms error {err[0]:.3e} -> {err[-1]:.3e}")
