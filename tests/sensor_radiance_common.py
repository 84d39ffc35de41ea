"""What the tests of the radiance splats (sensor.splat_radiance / splat_radiance_far, csrc/drrt_sensor.hip
k_sensor_radiance, k_sensor_radiance_bwd) share: the float64 restatements -- oracle/sensor_ref.py per channel, plus the
one it does not have, dL/drad, built here on its taps -- and the fixture made by running the reference."""
import os

import numpy as np
import torch

from oracle import sensor_ref as S

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sensor_radiance.npz")


def coords(x, v, p, n, arg, t2, far):
    """The sensor coordinates of a radiance splat -> dict(xn (N, 2), span, F0 (N,): |v.n|, far field 1, t1, t2).  `arg`:
    span, or angle_span in degrees for the far field."""
    x, v = np.asarray(x, np.float64), np.asarray(v, np.float64)
    if not far:
        c = S.sdf_coords(x, v, p, n, arg, t2)                    # generate_sensor places its rays at the same coordinates
        return dict(c, F0=np.abs(c["den"]))
    t1, t2 = S.tan_vecs(n, t2)
    ac = S._ang_cut(arg)
    vh = v / np.linalg.norm(v, axis=-1, keepdims=True)
    return dict(xn=np.stack([vh @ t1, vh @ t2], -1) + ac, span=2 * ac, F0=np.ones(len(v)), t1=t1, t2=t2)


def seed_taps(taps, gI, res):
    """The seed image at the 16 taps of every ray, 0 off the image."""
    return np.where(taps[7], gI[np.clip(taps[1], 0, res - 1), np.clip(taps[2], 0, res - 1)], 0.0)


def grad_rad(x, v, p, n, res, arg, gI, t2, far=False):
    """dL/drad (N, C) of L = sum(gI * image), gI (C, res, res):  F0 G_c  with  G_c = sum_{j in image} gI[c, tap_j] w_j / W,
    W the sum of all 16 weights."""
    c = coords(x, v, p, n, arg, t2, far)
    taps = S._taps(c["xn"], res, c["span"])
    w = taps[6]
    W = w.sum(axis=(1, 2))
    gI = np.asarray(gI, np.float64)
    return np.stack([c["F0"] * (seed_taps(taps, g, res) * w).sum(axis=(1, 2)) / W for g in gI], -1)


def images(x, v, rad, p, n, res, arg, t2, far=False):
    """(C, res, res): oracle/sensor_ref.py's image per channel."""
    rad = np.asarray(rad, np.float64)
    if far:
        return np.stack([S.generate_inf_sensor(v, rad[:, k], n, res, arg, t2) for k in range(rad.shape[1])])
    return np.stack([S.generate_sensor(x, v, rad[:, k], p, n, res, arg, t2) for k in range(rad.shape[1])])


def ray_grads(x, v, rad, p, n, res, arg, gI, t2, far=False):
    """(dL/dx, dL/dv): oracle/sensor_ref.py's backward per channel, summed (far field: dL/dx = 0)."""
    rad = np.asarray(rad, np.float64)
    gx, gv = np.zeros((len(v), 3)), np.zeros((len(v), 3))
    for k in range(rad.shape[1]):
        if far:
            gv += S.generate_inf_sensor_backward(v, rad[:, k], n, res, gI[k], arg, t2)
        else:
            a, b = S.generate_sensor_backward(x, v, rad[:, k], p, n, res, arg, gI[k], t2)
            gx += a; gv += b
    return gx, gv


def fixture(tag):
    """The reference-run case `tag` ("near" / "far") of tests/golden/sensor_radiance.npz as float64 arrays."""
    z = np.load(GOLDEN)
    far = tag == "far"
    c = dict(x=z["x"], v=z["v_far"] if far else z["v"], rad=z["rad"], p=z["p"], n=z["n"], t=z["t"], res=int(z["res"]),
             arg=float(z["angle_span"] if far else z["span"]), far=far, img=z[f"{tag}_img"], gI=z[f"{tag}_gI"],
             ge=z[f"{tag}_ge"], gv=z[f"{tag}_gv"], gx=np.zeros(z["x"].shape) if far else z["near_gx"])
    return {k: (np.asarray(a, np.float64) if isinstance(a, np.ndarray) else a) for k, a in c.items()}


# ---- the error model of tests/test_sensor_fuzz.py ---------------------------------------------------------------------
# |kernel - restatement| <= c 2^-24 S per element, S the sum of the magnitudes of the output's terms.  That file states the
# model for generate_sensor, generate_inf_sensor and the texture lookups and keeps its helpers to itself (a test module
# is not imported by another, tests/test_support_layout.py); these are the same helpers, for the radiance splats.
EPS = 2.0 ** -24
SQ2 = np.sqrt(2.0)
KINK = 2.0 ** -22          # a tap within KINK * U texels of r = 0 or sqrt(2) leaves its ray out of the ray-gradient check
KINK_FRACTION = 0.1        # ... which may happen to at most this fraction of the rays


def r32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def to_dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


def to_np(tensor):
    return tensor.detach().cpu().numpy().astype(np.float64)


def frame(rng):
    """(n, t2, t1): oblique, lengths 0.5..2, t2 not quite perpendicular to n, on a 1/64 grid (t1 = n x t2 exact)."""
    n = rng.normal(size=3); n *= rng.uniform(0.5, 2.0) / np.linalg.norm(n)
    t = np.cross(n, rng.normal(size=3)); t *= rng.uniform(0.5, 2.0) / np.linalg.norm(t)
    n, t = np.round(n * 64) / 64, np.round(t * 64) / 64
    return n, t, np.cross(n, t)


def check(name, got, want, terms, c, keep=None):
    """Per element |got - want| <= c * 2^-24 * terms; prints the largest ratio (what each `c` is stated with)."""
    got, want, terms = (np.asarray(a, np.float64) for a in (got, want, terms))
    assert np.isfinite(got).all(), f"{name}: {int((~np.isfinite(got)).sum())} non-finite outputs"
    err = np.abs(got - want)
    ratio = np.where(terms > 0, err / np.where(terms > 0, EPS * terms, 1.0), np.where(err > 0, np.inf, 0.0))
    if keep is not None:
        ratio = ratio[keep]
    worst = float(ratio.max()) if ratio.size else 0.0
    print(f"\n[radiance fuzz] {name}: max err / (2^-24 S) = {worst:.3g} (c = {c})")
    assert worst <= c, f"{name}: error {worst:.3g} x 2^-24 S exceeds c = {c}"


def tent(taps, fi):
    """The interpolant sum w f_i / sum w over 16 taps and the magnitudes of its terms -> f, fu (d f / d u, per texel),
    A0 (terms of f), A1 (terms of fu), H (bounds |d fu / d u|: how far an error in u moves fu), kink (distance of the
    nearest tap from r = 0 or r = sqrt 2)."""
    _, _, _, da, db, r, w = taps[:7]
    W = w.sum(axis=(1, 2))
    f = (w * fi).sum(axis=(1, 2)) / W
    live = (w > 0) & (r > 0)
    rs = np.where(live, r, 1.0)
    dwa, dwb = np.where(live, -da / rs, 0.0), np.where(live, -db / rs, 0.0)
    dfi = fi - f[:, None, None]
    fu = np.stack([(dfi * dwa).sum(axis=(1, 2)), (dfi * dwb).sum(axis=(1, 2))], -1) / W[:, None]
    af = np.abs(fi) + np.abs(f)[:, None, None]
    adw = np.abs(dwa) + np.abs(dwb)
    A0 = (af * (w + SQ2)).sum(axis=(1, 2)) / W
    A1 = (af * (adw + 1.0)).sum(axis=(1, 2)) / W
    H = (2 * (live * np.abs(dfi) / rs).sum(axis=(1, 2)) + 2 * np.abs(fu).sum(-1) * adw.sum(axis=(1, 2))) / W
    kink = np.minimum(r.min(axis=(1, 2)), np.abs(r - SQ2).min(axis=(1, 2)))
    return f, fu, A0, A1, H, kink


def plane_terms(x, v, p, n):
    """-> (den, t, dt): t = n.(p - x) / n.v and the terms of t (its rounding error is ~ 2^-24 dt)."""
    den = (v * n).sum(-1)
    t = ((p - x) * n).sum(-1) / den
    dt = (((np.abs(p) + np.abs(x)) * np.abs(n)).sum(-1) + np.abs(t) * (np.abs(v) * np.abs(n)).sum(-1)) / np.abs(den)
    return den, t, dt


def u_terms(qt, half, hs, u):
    """Terms of a sensor coordinate u = (q.t + half) / hs - 0.5, in texels, from the terms qt of q.t."""
    return (qt + half) / hs + np.abs(u).max(-1) + 1.0


def near_qt(x, v, p, t, dt, t1, t2):
    """Terms of q.t1 and q.t2, q = x + t v - p."""
    T = np.abs(t1) + np.abs(t2)
    return (np.abs(x) + np.abs(t)[:, None] * np.abs(v) + np.abs(p)) @ T + dt * (np.abs(v) @ T)


def grad_chain(gu, mu, hs, t1, t2):
    """dL/du (per texel: values and terms) -> dL/d(sensor point) (values and terms)."""
    g, m = gu / hs, (mu + 4 * np.abs(gu)) / hs
    gq = g[:, :1] * t1 + g[:, 1:] * t2
    return gq, m[:, :1] * np.abs(t1) + m[:, 1:] * np.abs(t2) + np.abs(gq)


def plane_chain(gq, mq, v, n, den, t, dt):
    """Terms of gx = (I - v n^T / den)^T gq and of t gx."""
    vg = (v * gq).sum(-1) / den
    mvg = ((np.abs(v) * mq).sum(-1) + np.abs(v * gq).sum(-1) + np.abs(vg) * (np.abs(v) * np.abs(n)).sum(-1)) / np.abs(den)
    gx = gq - n * vg[:, None]
    mgx = mq + np.abs(n) * mvg[:, None] + np.abs(gx)
    return mgx, np.abs(t)[:, None] * mgx + np.abs(gx) * dt[:, None]


def near_rays(rng, u, p, n, t2, t1, span, res, trange=(-1.0, 2.0)):
    """Rays that meet the plane (p, n) at sensor coordinates u (texels), from either side (v.n of either sign), the
    plane ahead of or behind the origin (t in trange * span)."""
    hs, m = span / res, len(u)
    q = np.linalg.solve(np.stack([t1, t2, n]), np.stack([(u[:, 0] + 0.5) * hs - span / 2,
                                                         (u[:, 1] + 0.5) * hs - span / 2, np.zeros(m)])).T
    nh = n / np.linalg.norm(n)
    v = rng.normal(size=(m, 3)) * 0.5 + nh * (rng.uniform(0.3, 1.0, (m, 1)) * rng.choice([-1.0, 1.0], (m, 1)))
    return p + q - rng.uniform(*trange, (m, 1)) * span * v, v


def both_frames(gpu, run, p, n, t2):
    """run(P, N, T) with the frame on the host (drrt_sensor_*_f32) and on the device (drrt_sensor_*_dframe_*)."""
    return [run(to_dev(p[None], d), to_dev(n[None], d), to_dev(t2[None], d)) for d in ("cpu", gpu)]


def same_per_ray(outs, names):
    for a, b, name in zip(outs[0], outs[1], names):
        assert np.isfinite(a).all(), f"{name}: {int((~np.isfinite(a)).sum())} non-finite outputs"
        assert np.array_equal(a, b), f"{name}: host-frame and device-frame entries differ"


def image_terms(taps, F, U, res):
    """Per-pixel terms of a splatted image: each contribution F w / W with its own terms and those of the coordinate it
    was placed at, and one fp32 add per (pixel, 256-ray block) of the accumulation."""
    _, ia, ib, _, _, _, w, valid = taps
    W = w.sum(axis=(1, 2))[:, None, None]
    aF = np.abs(F)[:, None, None] * np.ones_like(w)
    contrib = aF * w / W
    own = aF / W * (w + SQ2 + (1.0 + 16.0 * w / W) * U[:, None, None])
    pix = (ia * res + ib)[valid]
    blk = ((np.arange(len(F)) // 256)[:, None, None] + np.zeros_like(ia))[valid]
    terms, total = np.zeros(res * res), np.zeros(res * res)
    np.add.at(terms, pix, own[valid])
    np.add.at(total, pix, contrib[valid])
    nb = int(blk.max()) + 1 if blk.size else 1
    blocks = np.bincount(np.unique(pix * nb + blk) // nb, minlength=res * res)
    return (terms + blocks * total).reshape(res, res)
