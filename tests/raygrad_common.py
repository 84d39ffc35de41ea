"""What the ray-gradient test files (test_raygrad.py, test_cable_raygrad.py, test_stop_raygrad.py) share: the tolerances,
small helpers, and the grids and ray sets of the box march, which the plane and SDF marches are tested on too.  A plain
module: no fixtures, no tests."""
import numpy as np
import torch

import cases

TIE_TOL = 1e-5          # fp32 vs fp64 exit samples / records
GRAD_TOL = 1e-3         # per-ray relative error of (dpos, dvel) against float64 autograd


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def rel_err(dp, dv, gp, gv):
    a = np.concatenate([dp, dv], 1).astype(np.float64)
    b = np.concatenate([gp, gv], 1).astype(np.float64)
    return np.linalg.norm(a - b, axis=1) / np.maximum(np.linalg.norm(b, axis=1), 1e-30)


def _t(a, dev):
    return torch.as_tensor(np.asarray(a), device=dev)


def grads(apply, s, dev, rif_grad=True, x_grad=False, v_grad=False, rif="rif", dtype=torch.float32):
    """``apply(rif, x, v) -> (xt, vt, *more)`` on the case `s` -> L = <dx, xt> + <dv, vt> + sum(more) -> backward ->
    (rif.grad, x.grad, v.grad).  `rif` names the case's grid or profile; `dtype` is that of x."""
    rif = _t(s[rif], dev).requires_grad_(rif_grad)
    x = _t(s["pos"], dev).to(dtype).requires_grad_(x_grad)
    v = _t(s["vel"], dev).requires_grad_(v_grad)
    xt, vt, *more = apply(rif, x, v)
    loss = (xt * _t(s["dx"], dev)).sum() + (vt * _t(s["dv"], dev)).sum()
    for term in more:
        loss = loss + term
    loss.backward()
    torch.cuda.synchronize()
    return rif.grad, x.grad, v.grad


# ---- the box march's grids and ray sets ---------------------------------------------------------------------------------
def ray_sets(ext, ds, seed=0):
    """ext = (ex, ey, ez), the box extents ((res - 1) h).  -> {name: (pos, vel)} fp32."""
    ext = np.asarray(ext, np.float64)
    rng = np.random.default_rng(seed)
    out = {}
    # plane source outside the y = 0 face (the package's plane sources), and a point source below it
    p, v = cases.plane_rays(96, 1.0, ds, seed=seed, tilt=0.1)
    out["plane"] = (p * ext.astype(np.float32), v)
    n = 96
    d = rng.normal(0, 0.15, (n, 3)); d[:, 1] = 1.0
    out["point"] = (np.tile(np.array([[0.5, -0.35, 0.45]]) * ext, (n, 1)), _unit(d))
    # strictly inside, any direction
    out["inside"] = (rng.uniform(0.15, 0.85, (n, 3)) * ext, _unit(rng.normal(size=(n, 3))))
    # starting exactly on a face (x = 0, and the far z face heading back in)
    p = rng.uniform(0.1, 0.9, (n, 3)) * ext
    d = rng.normal(0, 0.2, (n, 3))
    p[: n // 2, 0] = 0.0; d[: n // 2, 0] = 1.0
    p[n // 2:, 2] = ext[2]; d[n // 2:, 2] = -1.0
    out["face"] = (p, _unit(d))
    # never entering: parallel to a face outside the box, and pointing away from it
    p = rng.uniform(0.1, 0.9, (n, 3)) * ext
    d = np.zeros((n, 3))
    p[: n // 2, 1] = -0.2 * ext[1]; d[: n // 2, 0] = 1.0; p[: n // 2, 0] = -0.1 * ext[0]
    p[n // 2:, 2] = -0.1 * ext[2]; d[n // 2:] = _unit(rng.normal(0, 0.1, (n - n // 2, 3)) + [0, 0, -1.0])
    out["never"] = (p, d)
    # grazing an edge: along x just inside / just outside the (y = 0, z = 0) edge
    p = np.zeros((n, 3)); d = np.zeros((n, 3))
    p[:, 0] = -0.1 * ext[0]
    p[:, 1] = rng.uniform(-0.02, 0.02, n) * ext[1]; p[:, 2] = rng.uniform(-0.02, 0.02, n) * ext[2]
    d[:, 0] = 1.0; d[:, 1] = rng.uniform(-0.02, 0.05, n); d[:, 2] = rng.uniform(-0.02, 0.05, n)
    out["graze"] = (p, _unit(d))
    # zero velocity: outside the box (fails the forward), and inside (n grad n sets it moving: an ordinary ray)
    p = rng.uniform(0.1, 0.9, (n, 3)) * ext
    p[: n // 2, 1] = -0.1 * ext[1]
    out["zero"] = (p, np.zeros((n, 3)))
    return {k: (a.astype(np.float32), b.astype(np.float32)) for k, (a, b) in out.items()}


SCENES = {
    # name: (torch-order grid (D, H, W), h, ds)
    "lens16_h1_half": ("lens16", 1.0, 0.5),
    "lens16_h05_half": ("lens16", 0.5, 0.25),
    "lens16_h1_multi": ("lens16", 1.0, 1.7),
    "box7x11x5_h1_half": ("box", 1.0, 0.5),
    "box7x11x5_h05_multi": ("box", 0.5, 0.8),
}


def grid(kind):
    if kind == "lens16":
        return cases.luneburg(16)
    rng = np.random.default_rng(5)
    D, H, W = 5, 11, 7
    z, y, x = np.meshgrid(np.linspace(0, 1, D), np.linspace(0, 1, H), np.linspace(0, 1, W), indexing="ij")
    f = 1.0 + 0.3 * np.sin(2.1 * x + 0.4) * np.cos(1.7 * y - 0.3) * np.sin(2.6 * z + 1.1) + 0.05 * rng.random((D, H, W))
    return f.astype(np.float32)
