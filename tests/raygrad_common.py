"""What the ray-gradient test files (test_raygrad.py, test_cable_raygrad.py, test_stop_raygrad.py, test_target_raygrad.py) and the
support modules built on them share: the tolerances, small helpers, the grids and ray sets of the box march, which the plane,
SDF and target marches are tested on too, and the scenes and host calls of those marches.  A plain
module: no fixtures, no tests."""
import numpy as np
import torch

import cases
import hostcheck_lib as HC

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


def max_steps_fwd(res, h, ds):
    return int(np.float32(4.0) * np.float32(h) * np.float32(max(res)) / np.float32(ds))


# ---- the scenes and host calls of the ray, plane, SDF and target marches ---------------------------------------------------
def scene(name, seed=0):
    """The box march's scene with seeds on (xt, vt)."""
    kind, h, ds = SCENES[name]
    rif = grid(kind)
    D, H, W = rif.shape
    res = (W, H, D)
    ext = ((W - 1) * h, (H - 1) * h, (D - 1) * h)
    sets = ray_sets(ext, ds, seed)
    pos = np.concatenate([s[0] for s in sets.values()])
    vel = np.concatenate([s[1] for s in sets.values()])
    labels = np.concatenate([[k] * len(s[0]) for k, s in sets.items()])
    rng = np.random.default_rng(seed + 11)
    dx = rng.normal(size=pos.shape).astype(np.float32)
    dv = rng.normal(size=pos.shape).astype(np.float32)
    return dict(rif=rif, res=res, h=h, ds=ds, pos=pos, vel=vel, labels=labels, dx=dx, dv=dv)


PLANES = {
    # name: (origin as a fraction of the box extents, direction)
    "axis": ((0.5, 0.6, 0.5), (0.0, 1.0, 0.0)),
    "tilted": ((0.5, 0.45, 0.5), (0.3, 0.9, 0.1)),
}


def _concat(s, sets):
    pos = np.concatenate([a for a, _ in sets.values()]).astype(np.float32)
    vel = np.concatenate([b for _, b in sets.values()]).astype(np.float32)
    s["labels"] = np.concatenate([[k] * len(a) for k, (a, _) in sets.items()])
    rng = np.random.default_rng(17)
    s.update(pos=pos, vel=vel, dx=rng.normal(size=pos.shape).astype(np.float32),
             dv=rng.normal(size=pos.shape).astype(np.float32))
    return s


def _base(name):
    kind, h, ds = SCENES[name]
    rif = grid(kind)
    D, H, W = rif.shape
    ext = np.array([(W - 1) * h, (H - 1) * h, (D - 1) * h])
    return dict(rif=rif, res=(W, H, D), h=h, ds=ds, ext=ext), dict(ray_sets(ext, ds, 0))


def plane_scene(name, plane):
    """The box march's scene and ray sets (raygrad_common), one sensor plane for all rays, and the "back" set: rays that
    start in bounds PAST the plane and head back through it (the global-loop case: their record is overwritten when they
    leave again)."""
    s, sets = _base(name)
    ext = s["ext"]
    o = np.array(PLANES[plane][0]) * ext
    d = _unit(PLANES[plane][1])
    rng = np.random.default_rng(23)
    p = rng.uniform(0.12, 0.88, (4000, 3)) * ext
    dist = (p - o) @ d
    p = p[dist > 1.5 * s["ds"]][:96]
    assert len(p) == 96
    sets["back"] = (p, _unit(-d + rng.normal(0, 0.12, (96, 3))))
    s = _concat(s, sets)
    n = len(s["pos"])
    s["po"] = np.tile(o.astype(np.float32), (n, 1))
    s["pd"] = np.tile(d.astype(np.float32), (n, 1))
    return s


def sphere_sdf(s):
    W, H, D = s["res"]
    h = s["h"]
    z, y, x = np.meshgrid(np.arange(D) * h, np.arange(H) * h, np.arange(W) * h, indexing="ij")
    c = s["ext"] / 2
    return (np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2) - 0.42 * s["ext"].min()).astype(np.float32)


def sdf_scene(name):
    """The box march's scene and ray sets (raygrad_common), a sphere of radius 0.42 of the smallest extent as the object,
    and the "object" set: rays that start inside it."""
    s, sets = _base(name)
    s["sdf"] = sphere_sdf(s)
    rng = np.random.default_rng(29)
    r = 0.42 * s["ext"].min()
    u = _unit(rng.normal(size=(96, 3))) * (r * 0.85 * rng.uniform(0, 1, (96, 1)) ** (1 / 3))
    sets["object"] = (s["ext"] / 2 + u, _unit(rng.normal(size=(96, 3))))
    return _concat(s, sets)


def host_plane(s):
    return HC.backtrace_pln_rays(s["rif"], s["res"], s["pos"], s["vel"], s["po"], s["pd"], s["dx"], s["dv"], s["h"], s["ds"])


def host_sdf(s):
    return HC.backtrace_sdf_rays(s["rif"], s["sdf"], s["res"], s["pos"], s["vel"], s["dx"], s["dv"], s["h"], s["ds"])


def _targets(sets, ext, ds):
    """Every set in quarters: somewhere in the middle of the box; just beyond the box along the ray (the record is written
    after the escape); the ray's origin (j = 0); 2.4 steps ahead (inside the prefix for the sets that start outside)."""
    rng = np.random.default_rng(31)
    out = []
    for pos, vel in sets.values():
        pos, vel = pos.astype(np.float64), vel.astype(np.float64)
        n = len(pos)
        q = [slice(k * n // 4, (k + 1) * n // 4) for k in range(4)]
        speed = np.linalg.norm(vel, axis=1, keepdims=True)
        u = np.divide(vel, speed, out=np.zeros_like(vel), where=speed > 0)
        tg = np.empty_like(pos)
        tg[q[0]] = (0.5 + rng.uniform(-0.2, 0.2, (q[0].stop - q[0].start, 3))) * ext
        tg[q[1]] = 0.5 * ext + u[q[1]] * (0.5 * np.linalg.norm(ext) + 4 * ds) + rng.normal(0, 0.5 * ds, (q[1].stop - q[1].start, 3))
        tg[q[2]] = pos[q[2]]
        tg[q[3]] = pos[q[3]] + vel[q[3]] * 2.4 * ds + rng.normal(0, 0.3 * ds, (q[3].stop - q[3].start, 3))
        out.append(tg)
    return np.concatenate(out).astype(np.float32)


_scenes = {}


def target_scene(name, zero):
    """The box march's scene and ray sets (raygrad_common), with (`zero` = "zero") or without the "zero" set: without it the
    global loop count is the slowest ray's and not max_steps, so phase B's dependence on the other rays shows."""
    if (name, zero) in _scenes:
        return _scenes[name, zero]
    kind, h, ds = SCENES[name]
    rif = grid(kind)
    D, H, W = rif.shape
    ext = np.array([(W - 1) * h, (H - 1) * h, (D - 1) * h])
    sets = dict(ray_sets(ext, ds, 0))
    if zero != "zero":
        del sets["zero"]
    pos = np.concatenate([a for a, _ in sets.values()]).astype(np.float32)
    vel = np.concatenate([b for _, b in sets.values()]).astype(np.float32)
    rng = np.random.default_rng(17)
    s = dict(rif=rif, res=(W, H, D), h=h, ds=ds, ext=ext, pos=pos, vel=vel,
             labels=np.concatenate([[k] * len(a) for k, (a, _) in sets.items()]),
             dx=rng.normal(size=pos.shape).astype(np.float32), dv=rng.normal(size=pos.shape).astype(np.float32),
             dd2=rng.normal(size=len(pos)).astype(np.float32), tg=_targets(sets, ext, ds))
    assert len(pos) % 256 != 0
    _scenes[name, zero] = s
    return s
