"""Seeded GPU fuzz of the fused sensor kernels (csrc/drrt_sensor.hip) against the float64 restatements of
oracle/sensor_ref.py (which tests/test_sensor.py pins to runs of the reference itself), at the shapes and edges where
they could go wrong: textures from 1x1 to 256x256, points far off the texture and exactly on texel centres,
near-parallel rays and rays with t < 0, angular windows from 10 to 179 degrees, images from 1^2 to 2048^2 with focused
bundles on tile edges and image corners.

Error model.  The restatement is evaluated on the fp32-rounded inputs, and every output (per ray; per pixel for
images) must satisfy  |kernel - restatement| <= c * 2^-24 * S,  where S is the sum of the absolute values of the terms
that form the output -- including the terms U of the sensor coordinate u (in texels) it is evaluated at, since an error
du there moves the output by |d out / d u| du.  There is no rel-L2 over a set: one ray off by 1e-3 fails.  Gradients
jump where a tap crosses r = 0 or r = sqrt(2); rays with a tap within KINK * U texels of such a kink are not compared
for their gradient, and their number must stay small.

Every operator that takes a sensor frame runs through both of its entries -- the frame in host float[3] arrays (planes
on the host) and in device memory (planes on the device) -- and their per-ray outputs must be equal.  Frames are drawn
on a 1/64 grid (oblique, not unit length): n x t2 is then exact in fp32, so every path uses the same tangent t1."""
import numpy as np
import pytest
import torch

from oracle import sensor_ref as S

EPS = 2.0 ** -24
SQ2 = np.sqrt(2.0)
KINK = 2.0 ** -22          # a tap within KINK * U texels of r = 0 or sqrt(2) leaves its ray out of the gradient check
KINK_FRACTION = 0.1        # ... which may happen to at most this fraction of the rays on or near the image / texture

# c of each bound; after each, the largest err / (2^-24 S) measured on an MI355X over the cases below
C_TEX_F, C_TEX_G = 4.0, 1.5          # texture lookups: value [1.07], ray gradients [0.47]
C_FAR_IMG, C_FAR_G = 1.5, 0.5        # far-field splat: image per pixel [0.33], dL/dv [0.09]
C_R2P_X, C_R2P_G = 2.0, 2.0          # rays_to_plane: x' [0.98], (dL/dx, dL/dv) [1.01]
C_IMG, C_SPLAT_G = 2.0, 1.0          # near splat: image per pixel and its sum [0.57], ray gradients [0.30]


def _r32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _frame(rng):
    """(n, t2, t1): oblique, lengths 0.5..2, t2 not quite perpendicular to n, on a 1/64 grid (t1 = n x t2 exact)."""
    n = rng.normal(size=3); n *= rng.uniform(0.5, 2.0) / np.linalg.norm(n)
    t = np.cross(n, rng.normal(size=3)); t *= rng.uniform(0.5, 2.0) / np.linalg.norm(t)
    n, t = np.round(n * 64) / 64, np.round(t * 64) / 64
    return n, t, np.cross(n, t)


def _check(name, got, want, terms, c, keep=None):
    """Per element |got - want| <= c * 2^-24 * terms; prints the largest ratio (what each `c` is stated with)."""
    got, want, terms = (np.asarray(a, np.float64) for a in (got, want, terms))
    assert np.isfinite(got).all(), f"{name}: {int((~np.isfinite(got)).sum())} non-finite outputs"
    err = np.abs(got - want)
    ratio = np.where(terms > 0, err / np.where(terms > 0, EPS * terms, 1.0), np.where(err > 0, np.inf, 0.0))
    if keep is not None:
        ratio = ratio[keep]
    worst = float(ratio.max()) if ratio.size else 0.0
    print(f"\n[sensor fuzz] {name}: max err / (2^-24 S) = {worst:.3g} (c = {c})")
    assert worst <= c, f"{name}: error {worst:.3g} x 2^-24 S exceeds c = {c}"


def _tent(taps, fi):
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


def _plane_terms(x, v, p, n):
    """-> (den, t, dt): t = n.(p - x) / n.v and the terms of t (its rounding error is ~ 2^-24 dt)."""
    den = (v * n).sum(-1)
    t = ((p - x) * n).sum(-1) / den
    dt = (((np.abs(p) + np.abs(x)) * np.abs(n)).sum(-1) + np.abs(t) * (np.abs(v) * np.abs(n)).sum(-1)) / np.abs(den)
    return den, t, dt


def _u_terms(qt, half, hs, u):
    """Terms of a sensor coordinate u = (q.t + half) / hs - 0.5, in texels, from the terms qt of q.t."""
    return (qt + half) / hs + np.abs(u).max(-1) + 1.0


def _near_qt(x, v, p, t, dt, t1, t2):
    """Terms of q.t1 and q.t2, q = x + t v - p."""
    T = np.abs(t1) + np.abs(t2)
    return (np.abs(x) + np.abs(t)[:, None] * np.abs(v) + np.abs(p)) @ T + dt * (np.abs(v) @ T)


def _grad_chain(gu, mu, hs, t1, t2):
    """dL/du (per texel: values and terms) -> dL/d(sensor point) (values and terms)."""
    g, m = gu / hs, (mu + 4 * np.abs(gu)) / hs
    gq = g[:, :1] * t1 + g[:, 1:] * t2
    return gq, m[:, :1] * np.abs(t1) + m[:, 1:] * np.abs(t2) + np.abs(gq)


def _plane_chain(gq, mq, v, n, den, t, dt):
    """Terms of gx = (I - v n^T / den)^T gq and of t gx."""
    vg = (v * gq).sum(-1) / den
    mvg = ((np.abs(v) * mq).sum(-1) + np.abs(v * gq).sum(-1) + np.abs(vg) * (np.abs(v) * np.abs(n)).sum(-1)) / np.abs(den)
    gx = gq - n * vg[:, None]
    mgx = mq + np.abs(n) * mvg[:, None] + np.abs(gx)
    return mgx, np.abs(t)[:, None] * mgx + np.abs(gx) * dt[:, None]


def _near_rays(rng, u, p, n, t2, t1, span, res, trange=(-1.0, 2.0)):
    """Rays that meet the plane (p, n) at sensor coordinates u (texels), from either side (v.n of either sign), the
    plane ahead of or behind the origin (t in trange * span)."""
    hs, m = span / res, len(u)
    q = np.linalg.solve(np.stack([t1, t2, n]), np.stack([(u[:, 0] + 0.5) * hs - span / 2,
                                                         (u[:, 1] + 0.5) * hs - span / 2, np.zeros(m)])).T
    nh = n / np.linalg.norm(n)
    v = rng.normal(size=(m, 3)) * 0.5 + nh * (rng.uniform(0.3, 1.0, (m, 1)) * rng.choice([-1.0, 1.0], (m, 1)))
    return p + q - rng.uniform(*trange, (m, 1)) * span * v, v


def _both_frames(gpu, run, p, n, t2):
    """run(P, N, T) with the frame on the host (drrt_sensor_*_f32) and on the device (drrt_sensor_*_dframe_*)."""
    return [run(_t(p[None], d), _t(n[None], d), _t(t2[None], d)) for d in ("cpu", gpu)]


def _same_per_ray(outs, names):
    for a, b, name in zip(outs[0], outs[1], names):
        assert np.isfinite(a).all(), f"{name}: {int((~np.isfinite(a)).sum())} non-finite outputs"
        assert np.array_equal(a, b), f"{name}: host-frame and device-frame entries differ"


# ---- texture lookups: get_sdf_vals_near / get_sdf_vals_far (k_sensor_tex_get, k_sensor_tex_get_bwd) -----------------
def _tex_targets(rng, res, m):
    """Sensor coordinates (texels): m spread over the texture and two texels around it, and m off the texture on every
    side and corner, 1 to 1e7 texels away."""
    inside = rng.uniform(-2.0, res + 1.0, (m, 2))
    dirs = np.array([[-1, 0], [1, 0], [0, -1], [0, 1], [-1, -1], [-1, 1], [1, -1], [1, 1]])[rng.integers(0, 8, m)]
    dist = 10.0 ** rng.uniform(0.0, 7.0, m)
    off = np.empty((m, 2))
    for k in range(2):
        d = dist * rng.uniform(1.0, 1.5, m)
        off[:, k] = np.where(dirs[:, k] < 0, -0.5 - d, np.where(dirs[:, k] > 0, res - 0.5 + d, rng.uniform(-1.0, res, m)))
    return np.concatenate([inside, off])


def _tex_case(gpu, x, v, tex, p, n, t2, t1, arg, far, gf, keep_all=False):
    from adjointnonlinearraytracing_amd import sensor
    fn = sensor.get_sdf_vals_far if far else sensor.get_sdf_vals_near

    def run(P, N, T):
        xs, vs = _t(x, gpu).requires_grad_(True), _t(v, gpu).requires_grad_(True)
        f = fn((xs, vs), _t(tex, gpu), (P, N), arg, T)
        (f * _t(gf, gpu)).sum().backward()
        return _np(f), _np(xs.grad), _np(vs.grad)

    outs = _both_frames(gpu, run, p, n, t2)
    _same_per_ray(outs, ("f", "dL/dx", "dL/dv"))
    f_k, gx_k, gv_k = outs[0]
    f_r = S.get_sdf_vals(x, v, tex, p, n, arg, t2, far)
    gx_r, gv_r = S.get_sdf_vals_backward(x, v, tex, p, n, arg, t2, far, grad_f=gf)
    c = S.sdf_coords(x, v, p, n, arg, t2, far)
    _, _, taps = S.tent_get(c["xn"], tex, c["span"])
    hs = taps[0]
    u = c["xn"] / hs - 0.5
    _, fu, A0, A1, H, kink = _tent(taps, taps[7])
    if far:
        U = _u_terms(np.abs(v) @ (np.abs(t1) + np.abs(t2)), c["span"] / 2, hs, u)
    else:
        den, t, dt = _plane_terms(x, v, p, n)
        U = _u_terms(_near_qt(x, v, p, t, dt, t1, t2), c["span"] / 2, hs, u)
    # fp32 places a point to ~2^-24 U texels: to first order (plus H for the change of slope) where that is below a
    # thousandth of a texel; beyond (points ~1e4+ texels off the texture) through a slope that holds for any u, 8 x the
    # texture's range (|fu| <= range x live taps / sum w), and those rays are left out of the gradient check
    far_off = EPS * U > 2.0 ** -10
    slope = np.where(far_off, 8 * np.ptp(tex), np.abs(fu).sum(-1) + H * EPS * U)
    tag = "tex far" if far else "tex near"
    _check(f"{tag} value", f_k, f_r, A0 + slope * U, C_TEX_F)
    gq, mq = _grad_chain(fu * gf[:, None], (np.abs(gf) * (A1 + H * U))[:, None], hs, t1, t2)
    if far:
        mgx, mgv = np.zeros_like(mq), mq
    else:
        mgx, mgv = _plane_chain(gq, mq, v, n, den, t, dt)
    keep = np.ones(len(x), bool) if keep_all else (kink > KINK * np.maximum(U, 1.0)) & ~far_off
    _check(f"{tag} dL/dx", gx_k, gx_r, mgx, C_TEX_G, keep)
    _check(f"{tag} dL/dv", gv_k, gv_r, mgv, C_TEX_G, keep)
    return keep


@pytest.mark.gpu
@pytest.mark.parametrize("far", [False, True], ids=["near", "far"])
@pytest.mark.parametrize("res", [1, 2, 3, 24, 97, 256])
def test_tex_lookup_fuzz(gpu, res, far):
    """Oblique planes, non-unit tangents, rays from either side of the plane (v.n < 0) and with t < 0, non-unit v in
    the far field; points on and around the texture, and off it on every side and corner up to 1e7 texels away
    (where the taps see only clipped edge texels: value and derivative stay finite and depend on frac(u))."""
    rng = np.random.default_rng(1000 + 2 * res + int(far))
    n, t2, t1 = _frame(rng)
    p = rng.uniform(-1.0, 1.0, 3)
    m = 1500
    u = _tex_targets(rng, res, m)
    if far:
        arg = float(rng.uniform(10.0, 170.0))
        ac = S._ang_cut(arg); hs = 2 * ac / res
        c = rng.uniform(0.2, 1.5, 2 * m) * rng.choice([-1.0, 1.0], 2 * m)          # v.n of either sign; |v| != 1
        v = np.linalg.solve(np.stack([t1, t2, n]), np.stack([(u[:, 0] + 0.5) * hs - ac, (u[:, 1] + 0.5) * hs - ac, c])).T
        x = rng.normal(size=v.shape)
    else:
        arg = float(np.float32(rng.uniform(0.3, 20.0)))
        x, v = _near_rays(rng, u, p, n, t2, t1, arg, res)
    tex = _r32(rng.normal(size=(res, res)))
    gf = _r32(rng.normal(size=2 * m))
    keep = _tex_case(gpu, _r32(x), _r32(v), tex, _r32(p), n, t2, t1, arg, far, gf)
    left_out = float((~keep[:m]).mean())
    print(f"[sensor fuzz] tex {'far' if far else 'near'} res {res}: {left_out:.2%} of the rays on the texture near a kink")
    assert left_out <= KINK_FRACTION


@pytest.mark.gpu
@pytest.mark.parametrize("res", [1, 2, 24])
def test_tex_lookup_on_texel_centres(gpu, res):
    """Points exactly on texel centres (r = 0 for one tap: the branch that gives it no derivative; the diagonal taps
    then lie exactly sqrt 2 away) and on texel edges, on and off the texture.  Axis-aligned frame, one texel per unit,
    rays along the normal: every coordinate is exact in fp32, so kernel and restatement see the same kinks and no ray
    is left out of the gradient check."""
    rng = np.random.default_rng(1500 + res)
    ia, ib = np.meshgrid(np.arange(-3, res + 3), np.arange(-3, res + 3), indexing="ij")
    u = np.stack([ia.ravel(), ib.ravel()], -1).astype(np.float64)
    u = np.concatenate([u, u + [0.5, 0.0], u + [0.0, 0.5], u + 0.5])
    n, t2 = np.array([0.0, 1.0, 0.0]), np.array([1.0, 0.0, 0.0])
    t1, p = np.cross(n, t2), np.array([0.0, 1.0, 0.0])                   # t1 = (0, 0, -1)
    m = len(u)
    x = np.stack([u[:, 1] + 0.5 - res / 2, np.full(m, 0.5), res / 2 - 0.5 - u[:, 0]], -1)
    v = np.zeros((m, 3)); v[:, 1] = rng.choice([1.0, 2.0], m)          # t = 0.5 or 0.25
    tex = _r32(rng.normal(size=(res, res)))
    gf = _r32(rng.normal(size=m))
    _tex_case(gpu, x, v, tex, p, n, t2, t1, float(res), False, gf, keep_all=True)


@pytest.mark.gpu
def test_tex_lookup_nan_in_nan_out(gpu):
    """NaN or infinite coordinates give NaN (not a value from a clipped edge texel); the other rays are unaffected."""
    from adjointnonlinearraytracing_amd import sensor
    x = torch.tensor([[0.1, 0.0, 0.2], [float("nan"), 0.0, 0.0], [0.3, 0.0, 0.1], [0.2, 0.0, 0.2]], device=gpu)
    v = torch.tensor([[0.0, 1.0, 0.0], [0.0, 1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, float("inf")]], device=gpu)
    tex = torch.rand(8, 8, device=gpu)
    p, n = torch.tensor([[0.0, 1.0, 0.0]], device=gpu), torch.tensor([[0.0, 1.0, 0.0]], device=gpu)
    t = torch.tensor([[1.0, 0.0, 0.0]], device=gpu)
    near = sensor.get_sdf_vals_near((x, v), tex, (p, n), 1.0, t).cpu()          # ray 2: v.n = 0 -> t = inf
    assert torch.isfinite(near[0]) and near[1:].isnan().all()
    far = sensor.get_sdf_vals_far((x, v), tex, (p, n), 90.0, t).cpu()           # ray 3: v = (0, 1, inf)
    assert torch.isfinite(far[:3]).all() and far[3].isnan()


# ---- far-field splat: generate_inf_sensor (k_sensor_splat / k_sensor_splat_bwd with far = 1) -------------------------
def _image_terms(taps, F, U, res):
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


@pytest.mark.gpu
@pytest.mark.parametrize("case", range(6))
def test_far_splat_fuzz(gpu, case):
    """angle_span from 10 to 179 degrees, res from 1 to 97, directions inside and outside the angular window, non-unit
    v, scalar and per-ray e: image per pixel and dL/dv per ray."""
    from adjointnonlinearraytracing_amd import sensor
    res, angle = [(1, 10.0), (2, 35.0), (3, 90.0), (17, 120.0), (64, 160.0), (97, 179.0)][case]
    rng = np.random.default_rng(2000 + case)
    n, t2, t1 = _frame(rng)
    p = rng.uniform(-1.0, 1.0, 3)
    m = 4000 + 77
    ac = S._ang_cut(angle)
    a = rng.uniform(-1.3, 1.3, (m, 2)) * ac
    a[: m // 10] = rng.uniform(1.5, 3.0, (m // 10, 2)) * ac * rng.choice([-1.0, 1.0], (m // 10, 2))   # outside
    c = rng.uniform(0.3, 1.0, m) * rng.choice([-1.0, 1.0], m)
    v = np.linalg.solve(np.stack([t1, t2, n]), np.stack([a[:, 0], a[:, 1], c])).T
    v = _r32(v * rng.uniform(0.2, 5.0, (m, 1)))
    x = _r32(rng.normal(size=(m, 3)))
    e = float(np.float32(rng.uniform(0.5, 2.0))) if case % 2 else _r32(rng.uniform(0.1, 2.0, m))
    gI = _r32(rng.normal(size=(res, res)))

    def run(P, N, T):
        xs, vs = _t(x, gpu).requires_grad_(True), _t(v, gpu).requires_grad_(True)
        img = sensor.generate_inf_sensor((xs, vs), e if isinstance(e, float) else _t(e, gpu), (P, N), res, angle, T)
        (img * _t(gI, gpu)).sum().backward()
        return _np(img), _np(vs.grad)

    outs = _both_frames(gpu, run, p, n, t2)
    _same_per_ray([outs[0][1:], outs[1][1:]], ("dL/dv",))
    img_r = S.generate_inf_sensor(v, e, n, res, angle, t2)
    gv_r = S.generate_inf_sensor_backward(v, e, n, res, gI, angle, t2)
    nv = np.linalg.norm(v, axis=-1, keepdims=True)
    vh = v / nv
    xn = np.stack([vh @ t1, vh @ t2], -1) + ac
    taps = S._taps(xn, res, 2 * ac)
    hs = taps[0]
    U = _u_terms(3 * (np.abs(vh) @ (np.abs(t1) + np.abs(t2))), ac, hs, xn / hs - 0.5)
    F = np.asarray(e, np.float64) * np.ones(m)
    terms = _image_terms(taps, F, U, res)
    for k, (img, _) in enumerate(outs):
        _check(f"far image res {res} ({'host' if k == 0 else 'device'} frame)", img, img_r, terms, C_FAR_IMG)
    gi = np.where(taps[7], gI[np.clip(taps[1], 0, res - 1), np.clip(taps[2], 0, res - 1)], 0.0)
    _, Gu, A0, A1, H, kink = _tent(taps, gi)
    gq, mq = _grad_chain(F[:, None] * Gu, (np.abs(F) * (A1 + H * U))[:, None], hs, t1, t2)
    mgv = (mq + np.abs(vh) * ((np.abs(vh) * mq).sum(-1) + np.abs(vh * gq).sum(-1))[:, None]) / nv + 4 * np.abs(gv_r)
    keep = kink > KINK * np.maximum(U, 1.0)
    _check(f"far res {res} dL/dv", outs[0][1], gv_r, mgv, C_FAR_G, keep)
    assert (~keep).mean() <= KINK_FRACTION


# ---- trace_rays_to_plane (k_rays_to_plane, k_rays_to_plane_bwd) ------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("per_ray", [True, False], ids=["per_ray_planes", "one_plane"])
def test_rays_to_plane_fuzz(gpu, per_ray):
    """Against the CPU float64 torch path (the reference's own expression, pinned by rays_to_plane.npz): planes ahead of
    and behind the origins (t < 0), v.n down to 1e-6 of |v| |n|, per-ray planes and one broadcast plane."""
    from adjointnonlinearraytracing_amd import sensor
    rng = np.random.default_rng(3000 + int(per_ray))
    m = 5000 + 13
    k = m if per_ray else 1
    n = rng.normal(size=(k, 3)); n *= rng.uniform(0.5, 2.0, (k, 1)) / np.linalg.norm(n, axis=1, keepdims=True)
    p = rng.uniform(-2.0, 2.0, (k, 3))
    x = rng.normal(size=(m, 3)) * 2.0
    nh = n / np.linalg.norm(n, axis=1, keepdims=True)
    v = rng.normal(size=(m, 3))
    v -= (v * nh).sum(-1, keepdims=True) * nh
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    v += nh * (10.0 ** rng.uniform(-6.0, 0.5, (m, 1)) * rng.choice([-1.0, 1.0], (m, 1)))
    v *= rng.uniform(0.3, 3.0, (m, 1))
    x, v, p, n = (_r32(a) for a in (x, v, p, n))
    g = _r32(rng.normal(size=(m, 3)))

    xs, vs = _t(x, gpu).requires_grad_(True), _t(v, gpu).requires_grad_(True)
    xo, _ = sensor.trace_rays_to_plane((xs, vs), (_t(p, gpu), _t(n, gpu)))
    assert type(xo.grad_fn).__name__.startswith("_RaysToPlane")
    xo.backward(_t(g, gpu))
    xr, vr = torch.from_numpy(x).requires_grad_(True), torch.from_numpy(v).requires_grad_(True)
    xo_r, _ = sensor.trace_rays_to_plane((xr, vr), (torch.from_numpy(p), torch.from_numpy(n)))
    xo_r.backward(torch.from_numpy(g))

    den, t, dt = _plane_terms(x, v, p, n)
    rel = np.abs(den) / (np.linalg.norm(v, axis=1) * np.linalg.norm(n, axis=1))
    assert (t < 0).mean() > 0.2 and rel.min() < 1e-5
    an = np.abs(n) * np.ones((m, 1))
    _check("rays_to_plane x'", _np(xo), _np(xo_r), np.abs(x) + np.abs(t)[:, None] * np.abs(v) + np.abs(v) * dt[:, None],
           C_R2P_X)
    c = (g * v).sum(-1) / den
    dc = (np.abs(g * v).sum(-1) + np.abs(c) * (an * np.abs(v)).sum(-1)) / np.abs(den)
    gcn = np.abs(g) + np.abs(c)[:, None] * an
    _check("rays_to_plane dL/dx", _np(xs.grad), _np(xr.grad), gcn + an * dc[:, None], C_R2P_G)
    _check("rays_to_plane dL/dv", _np(vs.grad), _np(vr.grad),
           np.abs(t)[:, None] * (gcn + an * dc[:, None]) + gcn * dt[:, None], C_R2P_G)


# ---- near splat: generate_sensor (k_sensor_splat's LDS tile and anchor vote, k_sensor_splat_bwd) ---------------------
@pytest.mark.gpu
@pytest.mark.parametrize("res", [1, 2, 47, 48, 49, 1277, 1300, 2048])
def test_near_splat_tile_path(gpu, res):
    """Blocks of 256 rays laid out for the tile path (kTile = 48 pixels, anchor vote clamped above 1277^2): a focused
    bundle plus stray rays in one block, a bundle at each image corner, a bundle wider than a tile, all rays of a
    block in one pixel, bundles beyond pixel 1277, and a ray count that is not a multiple of 256.  Image per pixel and
    ray gradients against the restatement; energy conservation for the rays whose 16 taps all land on the image."""
    from adjointnonlinearraytracing_amd import sensor
    rng = np.random.default_rng(4000 + res)
    n, t2, t1 = _frame(rng)
    p = rng.uniform(-1.0, 1.0, 3)
    span = float(np.float32(rng.uniform(0.5, 4.0)))

    def bundle(centre, spread, k):
        return np.asarray(centre, np.float64) + rng.normal(0.0, spread, (k, 2))

    blocks = [np.concatenate([bundle(rng.uniform(0, res, 2), 0.3, 200), rng.uniform(-3.0, res + 2.0, (56, 2))])]
    blocks += [bundle((ca, cb), 1.5, 256) for ca in (-0.5, res - 0.5) for cb in (-0.5, res - 0.5)]
    blocks.append(rng.integers(0, res, 2) + rng.uniform(-0.45, 0.45, (256, 2)))
    blocks.append(bundle(rng.uniform(0, res, 2), 20.0, 256))
    if res > 1277:
        blocks += [bundle((res - 8.0, res - 3.0), 2.0, 256), bundle((1278.0 + 0.5 * (res - 1278), res - 20.0), 30.0, 256)]
    blocks.append(rng.uniform(-3.0, res + 2.0, (2 * 256 + 77, 2)))
    u = np.concatenate(blocks)
    m = len(u)
    x, v = _near_rays(rng, u, p, n, t2, t1, span, res, trange=(-0.25, 0.5))
    x, v, p = _r32(x), _r32(v), _r32(p)
    e = float(np.float32(1.25)) if res in (48, 2048) else _r32(rng.uniform(0.5, 2.0, m))
    gI = _r32(rng.normal(size=(res, res)))

    def run(P, N, T, sel=slice(None)):
        xs, vs = _t(x[sel], gpu).requires_grad_(True), _t(v[sel], gpu).requires_grad_(True)
        ee = e if isinstance(e, float) else _t(e[sel], gpu)
        img = sensor.generate_sensor((xs, vs), ee, (P, N), res, span, T)
        (img * _t(gI, gpu)).sum().backward()
        return _np(img), _np(xs.grad), _np(vs.grad)

    outs = _both_frames(gpu, run, p, n, t2)
    _same_per_ray([outs[0][1:], outs[1][1:]], ("dL/dx", "dL/dv"))
    img_r = S.generate_sensor(x, v, e, p, n, res, span, t2)
    gx_r, gv_r = S.generate_sensor_backward(x, v, e, p, n, res, span, gI, t2)
    c = S.sdf_coords(x, v, p, n, span, t2)                   # generate_sensor places the rays at the same coordinates
    taps = S._taps(c["xn"], res, span)
    hs = taps[0]
    den, t, dt = _plane_terms(x, v, p, n)
    U = _u_terms(_near_qt(x, v, p, t, dt, t1, t2), span / 2, hs, c["xn"] / hs - 0.5)
    ev = np.asarray(e, np.float64) * np.ones(m)
    F = np.abs(den) * ev
    terms = _image_terms(taps, F, U, res)
    for k, (img, _, _) in enumerate(outs):
        _check(f"near image res {res} ({'host' if k == 0 else 'device'} frame)", img, img_r, terms, C_IMG)
    inside = taps[7].all(axis=(1, 2))
    if inside.any():
        img_in = run(_t(p[None], gpu), _t(n[None], gpu), _t(t2[None], gpu), inside)[0]
        terms_in = _image_terms(tuple(a[inside] if np.ndim(a) else a for a in taps), F[inside], U[inside], res)
        _check(f"near image res {res}: energy of the rays inside", img_in.sum(), F[inside].sum(), terms_in.sum(), C_IMG)
    gi = np.where(taps[7], gI[np.clip(taps[1], 0, res - 1), np.clip(taps[2], 0, res - 1)], 0.0)
    G, Gu, A0, A1, H, kink = _tent(taps, gi)
    gq, mq = _grad_chain(F[:, None] * Gu, (np.abs(F) * (A1 + H * U))[:, None], hs, t1, t2)
    mgx, mgv = _plane_chain(gq, mq, v, n, den, t, dt)
    mgv = mgv + (np.abs(ev) * (np.abs(G) + A0 + np.abs(Gu).sum(-1) * U))[:, None] * np.abs(n)
    keep = kink > KINK * np.maximum(U, 1.0)
    _check(f"near splat res {res} dL/dx", outs[0][1], gx_r, mgx, C_SPLAT_G, keep)
    _check(f"near splat res {res} dL/dv", outs[0][2], gv_r, mgv, C_SPLAT_G, keep)
    print(f"[sensor fuzz] near splat res {res}: {(~keep).mean():.2%} of the rays near a kink")
    assert (~keep).mean() <= KINK_FRACTION
