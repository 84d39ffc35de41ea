#!/usr/bin/env python3
"""Writes tests/golden/sensor_radiance.npz: the reference's core/sensor.py generate_sensor and generate_inf_sensor RUN AS
THEY ARE (float64, CPU), once per channel of a per-ray, per-channel energy, and torch.autograd through them under a
random seed image -- what sensor.splat_radiance / splat_radiance_far must compute, dL/d(energy) included.  Arrays only.

    python tests/golden/make_sensor_radiance.py [path of the reference's core/]

1024 rays onto 24 x 24 pixels, 3 channels, an oblique frame on a 1/64 grid (t1 = n x t2 is exact in fp32); about a
quarter of the rays miss the image, rays come from both sides of the plane (v.n of either sign) and from beyond it
(t < 0), the energy has negative entries and zeros.  The origins lie within half a span of the plane, as they do in
sensor_splat.npz, whose fp32 bounds (tests/test_sensor.py) this fixture is held to: the rounding of a landing point grows
with the distance travelled.  The far field has its own directions, a quarter of them outside the angular window, of
either sign of v.n and not of unit length.  Inputs are fp32 values, so a fp32 operator sees what the reference saw."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                                   # tests/: the ray recipes of the fuzz
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, sys.argv[1] if len(sys.argv) > 1 else "/root/reference/core")
sys.dont_write_bytecode = True

import sensor as ref_sensor                                                 # noqa: E402
from sensor_radiance_common import frame as _frame, near_rays as _near_rays, r32 as _r32                       # noqa: E402

N, RES, C, ANGLE = 1024, 24, 3, 100.0


def main():
    rng = np.random.default_rng(20240)
    n, t2, t1 = _frame(rng)
    p = _r32(rng.uniform(-1.0, 1.0, 3))
    span = float(np.float32(2.5))
    u = rng.uniform(-2.0, RES + 1.0, (N, 2))
    miss = rng.random(N) < 0.25
    side = rng.integers(0, 2, N)
    off = np.where(rng.random(N) < 0.5, -4.5 - rng.uniform(0, 6, N), RES + 2.5 + rng.uniform(0, 6, N))
    u[miss, side[miss]] = off[miss]
    x, v = _near_rays(rng, u, p, n, t2, t1, span, RES, trange=(-0.25, 0.5))
    x, v = _r32(x), _r32(v)
    ac = np.sin(0.5 * np.deg2rad(ANGLE))
    a = rng.uniform(-1.1, 1.1, (N, 2)) * ac
    a[: N // 4] = rng.uniform(1.4, 2.5, (N // 4, 2)) * ac * rng.choice([-1.0, 1.0], (N // 4, 2))
    # unit directions h with (h.t1, h.t2) = a: h = h0 + c k, with c from |h| = 1 (either root: both sides of the plane);
    # where a is out of a unit vector's reach, the nearest direction
    Minv = np.linalg.inv(np.stack([t1, t2, n]))
    h0, k = (Minv[:, :2] @ a.T).T, Minv[:, 2]
    b, disc = h0 @ k / (k @ k), (h0 @ k / (k @ k)) ** 2 - ((h0 * h0).sum(-1) - 1.0) / (k @ k)
    c = -b + rng.choice([-1.0, 1.0], N) * np.sqrt(np.maximum(disc, 0.0))
    vf = h0 + c[:, None] * k
    vf = _r32(vf * rng.uniform(0.2, 5.0, (N, 1)))
    rad = rng.normal(size=(N, C))
    rad[rng.random((N, C)) < 0.1] = 0.0
    rad = _r32(rad)
    gI = {"near": _r32(rng.normal(size=(C, RES, RES))), "far": _r32(rng.normal(size=(C, RES, RES)))}

    T = lambda arr: torch.from_numpy(np.ascontiguousarray(arr, dtype=np.float64))
    plane, tan = (T(p[None]), T(n[None])), T(t2[None])
    out = dict(x=x.astype(np.float32), v=v.astype(np.float32), v_far=vf.astype(np.float32), rad=rad.astype(np.float32),
               p=p, n=n, t=t2, res=RES, span=span, angle_span=ANGLE)
    for tag, dirs in (("near", v), ("far", vf)):
        xs, vs = T(x).requires_grad_(True), T(dirs).requires_grad_(True)
        es = [T(rad[:, k]).requires_grad_(True) for k in range(C)]
        if tag == "near":
            imgs = [ref_sensor.generate_sensor((xs, vs), e, plane, RES, span, tan) for e in es]
        else:
            imgs = [ref_sensor.generate_inf_sensor((xs, vs), e, plane, RES, ANGLE, tan) for e in es]
        img = torch.stack(imgs)
        (img * T(gI[tag])).sum().backward()
        assert img.dtype == torch.float64
        out.update({f"{tag}_img": img.detach().numpy(), f"{tag}_gI": gI[tag], f"{tag}_gv": vs.grad.numpy(),
                    f"{tag}_ge": torch.stack([e.grad for e in es], 1).numpy()})
        if tag == "near":
            out["near_gx"] = xs.grad.numpy()
        else:
            assert xs.grad is None or not xs.grad.any()
        hit = (torch.stack([e.grad for e in es], 1) != 0).any(1).numpy()
        print(f"{tag}: {1 - hit.mean():.1%} of the rays miss the image")
    den = v @ n
    print(f"v.n < 0: {(den < 0).mean():.1%}; t < 0: {((((p - x) @ n) / den) < 0).mean():.1%}; "
          f"rad < 0: {(rad < 0).mean():.1%}; rad == 0: {(rad == 0).mean():.1%}")
    path = os.path.join(HERE, "sensor_radiance.npz")
    np.savez_compressed(path, **out)
    print(f"sensor_radiance.npz: {os.path.getsize(path) / 1024:.1f} KiB")
    assert os.path.getsize(path) <= 256 * 1024


if __name__ == "__main__":
    main()
