"""What tests/test_cable_fuzz.py is built from: the configurations, the compared rays, the float64 referee and the ensemble
of float32 runs of the three restatements of the fibre march (tests/cable_ad), the
host build of the product's per-ray routines (hostcheck_lib, cable_integral_host) and the errors that go under the bound of
tests/integral_fuzz_common.py.  A plain module: no fixtures, no tests.  Everything is computed once per seed or per
(seed, routine) and handed out unchanged."""
import numpy as np
import torch

import cable_ad
import cable_common as CC
import cable_integral_host as H
import cases
import hostcheck_lib as HC
from integral_fuzz_common import CAPS, FLOOR, MARGIN, bound      # noqa: F401 (MARGIN, FLOOR: the bound's own, re-exported)
from cable_common import MAX_DROPPED      # noqa: F401 (the share test_cable_fuzz.py allows)
from raygrad_common import TIE_TOL, rel_err

LENGTHS = (2, 3, 5, 9, 17, 33, 64, 127, 200)      # profile samples, by seed % 9
SHAPES = ("luneburg", "random", "rising", "wavy")  # profile shape, by seed % 4
N_RAYS, N_REST = 400, 8
# The first 16 of range(64) whose configuration keeps at least MIN_REF_SHARE of its rays under the criteria that come from
# the restatement alone (1, 3 and 4 of `base`), in order, nothing skipped for any other reason:
# tests/test_cable_fuzz.py::test_seed_rule recomputes it.
SEEDS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 14, 15, 16, 18, 19)
MIN_REF_SHARE = 0.85    # leaves 5 % of a configuration to criterion 2, the only one the product has a say in
MAX_PRODUCT_ONLY = 0.05
# Criterion 3.  rhat = x / r and the Hessian term n' / r: a rounding of 2^-24 radius in x - radius is a relative change of
# 2^-24 radius / r in both, which every later iteration carries on.  At r = 0.02 radius that is 3e-6 per pass, within what
# the bound's cap (GRAD_TOL = 1e-3) leaves a march of a few hundred iterations; at 0.0035 samples from the axis, where a
# prototype of this test met it, the product and the float32 restatement agreed with each other and were 3e-3 from float64.
AXIS_SHARE = 0.02
AXIS_EXACT = 1e-6       # below it the ray is on the axis for the product (CylCell::tiny) and for cable_ad.sample: it stays in
# Criterion 4.  |(dpos, dvel)| / |(dx, dv)| is how far the march amplifies a perturbation of its input.  An input ulp
# (2^-24 relative) amplified 30 times is 1.8e-6: with MARGIN = 8 and a few hundred roundings of that size on the way, an
# honest fp32 run of such a ray can stand at GRAD_TOL = 1e-3, the cap no yardstick lifts.  Beyond 30 the comparison measures
# the ray's conditioning, not the product.
TAME = 30.0
N_RUNS = 5              # float32 runs of the restatement in the yardstick: one at the inputs, four at inputs moved by an ulp

# routine -> (profiles it differentiates, its seeds, its integral, the host result's profile gradients, their labels)
ROUTINES = {
    "rays": ((), ("dx", "dv"), None, (), ()),
    "opl": (("prof",), ("dx", "dv", "dopl"), "opl", ("grad",), ("dL/dprofile",)),
    "field": (("prof", "field"), ("dx", "dv", "dtau"), "tau", ("grad", "grad_field"), ("dL/dprofile", "dL/dfield")),
}
MODES = {"rays": {"all": ()}, "opl": CC.OPL_MODES, "field": CC.FIELD_MODES}      # routine -> {mode: the seeds it leaves out}

_configs, _bases, _inputs, _refs, _hosts = {}, {}, {}, {}, {}


def _f32(x):
    return float(np.float32(x))


def profile(shape, rres, rng):
    t = np.linspace(0, 1, rres)
    if shape == "luneburg":
        p = np.sqrt(2.0 - t ** 2)
    elif shape == "random":
        p = 1.0 + (0.5 if rres <= 9 else 0.1) * rng.random(rres)
    elif shape == "rising":                               # n' > 0: the sign of grad n and of the Hessian term n' / r flips
        p = 1.2 + 0.3 * t ** 2 + 0.02 * rng.random(rres)
    else:                                                 # not monotone: n' changes sign along the radius
        p = 1.5 - 0.2 * np.cos(3 * np.pi * t) + 0.02 * rng.random(rres)
    return p.astype(np.float32)


def config(seed):
    """The configuration of a seed: a profile of LENGTHS[seed % 9] samples and shape SHAPES[seed % 4], radius 0.1 .. 2, a
    step of 0.3 .. 3 radial samples, a length of 30 .. 120 steps (a ray at rest marches 4 length / ds <= 480 iterations), all
    rounded through float32; 400 rays drawn as cases.fuzz_cable_config draws them -- radii up to 1.2 of the fibre's, y from
    -0.1 to 1.1 of the length, 5 % with x == radius and 5 % with z == radius, its three fixed first rays, a quarter heading
    towards -y -- the last 8 at rest, 6 of them inside the fibre; targets as tests/cable_common.py::scene draws them
    (behind the start, near the path ahead, far beyond), the path ahead taken no longer than the ray needs to cross the
    fibre; the seeds (dx, dv, dopl, dtau) from a generator of this module's own, the second profile from
    tests/cable_common.py::field_profile."""
    if seed in _configs:
        return _configs[seed]
    rng = np.random.default_rng(5200 + seed)
    rres, shape = LENGTHS[seed % 9], SHAPES[seed % 4]
    # 0.1 .. 2, and every seventh configuration a thin fibre of 0.01 .. 0.02: the product's on-axis threshold is absolute
    # (r < 1e-6), and with every radius above 0.05 a threshold of 1e-3 in its place lies inside the band that criterion 3
    # leaves out (AXIS_SHARE radius) and passes.  On a thin fibre the rays that start close to the axis (below) are inside it
    u = rng.uniform(0.0, 1.0)
    radius = _f32(0.01 + 0.01 * u if seed % 7 == 6 else 0.1 + 1.9 * u)
    ds = _f32(radius / (rres - 1) * rng.uniform(0.3, 3.0))
    length = _f32(ds * rng.uniform(30, 120))
    prof = profile(shape, rres, rng)
    n = N_RAYS
    ang = rng.uniform(0, 2 * np.pi, n)
    rad = radius * rng.uniform(0, 1.2, n)
    yy = rng.uniform(-0.1, 1.1, n) * length
    rest = np.arange(n) >= n - N_REST
    inside_rest = rest & (np.arange(n) < n - 2)             # the last two stay where they were drawn
    rad[inside_rest] = radius * rng.uniform(0.15, 0.9, int(inside_rest.sum()))
    yy[inside_rest] = rng.uniform(0.1, 0.9, int(inside_rest.sum())) * length
    # 15 % of the rays inside start just outside the band of criterion 3, where x / r is at its worst among the compared.  On
    # a thin fibre they are 1e-3 from the axis or less: were they on the axis for the product, it would lose their records
    # to criterion 2, more than MAX_PRODUCT_ONLY allows
    close = (rng.random(n) < 0.15) & ~rest & (rad < radius)
    rad[close] = radius * rng.uniform(0.025, 0.05, n)[close]
    pos = np.stack([radius + rad * np.cos(ang), yy, radius + rad * np.sin(ang)], -1)
    on_x, on_z = (rng.random(n) < 0.05) & ~rest & ~close, (rng.random(n) < 0.05) & ~rest & ~close
    pos[on_x, 0] = radius
    pos[on_z, 2] = radius
    pos[:3] = [[radius, 0.0, radius], [radius, 0.3 * ds, radius], [2 * radius, 0.5 * length, radius]]
    vel = rng.normal(0, 0.4, (n, 3)); vel[:, 1] = rng.choice([1.0, 1.0, 1.0, -1.0], n)
    vel /= np.linalg.norm(vel, axis=1, keepdims=True)
    vel[1] = [0, 1, 0]
    vel[rest] = 0.0
    pos, vel = pos.astype(np.float32), vel.astype(np.float32)
    # targets: behind the start (j = 0), near the path ahead (0 < j < K) and far beyond along the heading (j = K).  "Ahead"
    # is a share of what the straight ray has left inside the fibre (its chord, its way to the end it is heading for), not of
    # the length: on a 2-sample profile a ray crosses the fibre in two steps
    kind = rng.integers(0, 3, n)
    xs = pos[:, [0, 2]].astype(np.float64) - radius
    vt = vel[:, [0, 2]].astype(np.float64)
    a, b, c0 = (vt * vt).sum(1), (xs * vt).sum(1), (xs * xs).sum(1) - radius * radius
    disc = np.maximum(b * b - a * c0, 0.0)
    chord = np.where(a > 0, (-b + np.sqrt(disc)) / np.maximum(a, 1e-30), np.inf)       # to the far wall (0 if it misses)
    vy = vel[:, 1].astype(np.float64)
    to_end = np.where(vy > 0, (length - pos[:, 1]) / np.maximum(vy, 1e-30), np.where(vy < 0, pos[:, 1] / np.maximum(-vy, 1e-30), 0.0))
    ahead = np.clip(np.minimum(chord, to_end), 4 * ds, length)
    along = np.where(kind == 0, -0.3 * length, np.where(kind == 1, rng.uniform(0.15, 0.6, n) * ahead, 20.0 * length))
    tg = pos + along[:, None] * vel + (kind == 1)[:, None] * rng.normal(0, 0.02 * radius, (n, 3))
    # the rays at rest fall along the radius (n grad n sets them moving): a target beside them in the cross-section, so that
    # about half of them get a record that moved
    off = rng.normal(0, 0.2 * radius, (n, 3)); off[:, 1] = 0.0
    tg[rest] = pos[rest] + off[rest]
    srng = np.random.default_rng(6100 + seed)
    c = dict(seed=seed, rres=rres, shape=shape, prof=prof, field=CC.field_profile(rres, seed), radius=radius, length=length,
             ds=ds, pos=pos, vel=vel, tg=tg.astype(np.float32), rest=rest, close=close,
             beyond=np.hypot(pos[:, 0].astype(np.float64) - radius, pos[:, 2].astype(np.float64) - radius) > radius,
             back=vel[:, 1] < 0, on_axis=(pos[:, 0] == np.float32(radius)) | (pos[:, 2] == np.float32(radius)),
             dx=srng.normal(size=(n, 3)).astype(np.float32), dv=srng.normal(size=(n, 3)).astype(np.float32),
             dopl=srng.normal(size=n).astype(np.float32), dtau=srng.normal(size=n).astype(np.float32))
    assert H.max_steps(length, ds) <= 480 and 0.29 < ds * (rres - 1) / radius < 3.01
    _configs[seed] = c
    return c


def _T(a, dtype):
    return torch.tensor(np.asarray(a), dtype=dtype)


def _records(c, j, dtype, pos=None, vel=None):
    """The restatement's (xt, vt) at the iterations j; whether any sample k < j of the ray lay within AXIS_SHARE of the
    radius of the axis without being on it (r < AXIS_EXACT); and a hash of the cells i0 those samples fell in:
    cable_ad.trace_cable's loop with that look at x_k in front of every step."""
    with torch.no_grad():
        prof = _T(c["prof"], dtype)
        x, v = _T(c["pos"] if pos is None else pos, dtype), _T(c["vel"] if vel is None else vel, dtype)
        jt = torch.as_tensor(j.astype(np.int64))
        xt, vt = x, v
        near = torch.zeros(len(j), dtype=torch.bool)
        cells = torch.zeros(len(j), dtype=torch.int64)
        h = c["radius"] / (c["rres"] - 1)
        for k in range(1, int(jt.max()) + 1):
            r = torch.hypot(x[:, 0] - c["radius"], x[:, 2] - c["radius"])
            live = jt >= k
            near |= live & (r > AXIS_EXACT) & (r < AXIS_SHARE * c["radius"])
            i0 = (torch.where(r < AXIS_EXACT, torch.zeros_like(r), r) / h).floor().long().clamp(0, c["rres"] - 1)
            cells = torch.where(live, cells * 1000003 + i0 + 1, cells)
            _, ngn = cable_ad.sample(prof, c["radius"], x)
            v = v + c["ds"] * ngn
            x = x + c["ds"] * v
            sel = (jt == k)[:, None]
            xt, vt = torch.where(sel, x, xt), torch.where(sel, v, vt)
    return xt.numpy(), vt.numpy(), near.numpy(), cells.numpy()


def base(seed):
    """-> dict(k, j, K, tie_ref, tie_prod, off_axis, tame, amp, ref_ok, compared): the host forward (its record and the
    record's iteration j, which every restatement takes as an input) and the four criteria a compared ray passes:
      1 tie_ref    the float32 and the float64 restatement records agree within TIE_TOL      (tie-free for the yardstick)
      2 tie_prod   the host build's record is within TIE_TOL of the float64 record           (tie-free for the product)
      3 off_axis   no sample k < j of the float64 march has AXIS_EXACT < r_k < AXIS_SHARE radius
      4 tame       |(dpos, dvel)| <= TAME |(dx, dv)| in float64, from (dx, dv) alone, one preliminary run
    1, 3 and 4 come from the restatement alone (ref_ok); the product can remove rays through 2 only.  The preliminary run
    covers the rays that pass 1 and 3: a ray's gradient does not depend on which other rays march beside it, so `tame` is
    what a run over those that pass 1 to 3 gives, and ref_ok needs no word from the product."""
    if seed in _bases:
        return _bases[seed]
    c = config(seed)
    k = H.trace_cable_opl(c["prof"], c["radius"], c["length"], c["pos"], c["vel"], c["tg"], c["ds"])
    j = k["rec_steps"]
    x64, v64, near, _ = _records(c, j, torch.float64)
    x32, v32, _, cells = _records(c, j, torch.float32)
    close = lambda a, b: np.abs(a.astype(np.float64) - b).max(1) <= TIE_TOL      # noqa: E731
    tie_ref = close(x32, x64) & close(v32, v64)
    tie_prod = close(k["xt"], x64) & close(k["vt"], v64)
    off_axis = ~near
    idx = np.nonzero(tie_ref & off_axis)[0]
    p, v = _T(c["pos"][idx], torch.float64).requires_grad_(True), _T(c["vel"][idx], torch.float64).requires_grad_(True)
    xt, vt = cable_ad.trace_cable(_T(c["prof"], torch.float64), c["radius"], c["length"], p, v, j[idx].astype(np.int64), c["ds"])
    gp, gv = torch.autograd.grad((xt * _T(c["dx"][idx], torch.float64)).sum() + (vt * _T(c["dv"][idx], torch.float64)).sum(), (p, v))
    amp = np.full(N_RAYS, np.inf)
    amp[idx] = np.linalg.norm(np.concatenate([gp.numpy(), gv.numpy()], 1), axis=1) / \
        np.linalg.norm(np.concatenate([c["dx"][idx], c["dv"][idx]], 1).astype(np.float64), axis=1)
    tame = amp <= TAME
    ref_ok = tie_ref & off_axis & tame
    _bases[seed] = dict(k=k, j=j, K=k["steps"], cells=cells, tie_ref=tie_ref, tie_prod=tie_prod, off_axis=off_axis, tame=tame, amp=amp,
                        ref_ok=ref_ok, compared=ref_ok & tie_prod)
    return _bases[seed]


def ref_share(seed):
    """The share of a configuration's rays that pass criteria 1, 3 and 4: what the seed rule looks at."""
    return float(base(seed)["ref_ok"].mean())


def seeds_of(c, routine, mode, compared):
    """{name: array}: the seeds of a mode, those of the rays that are not compared zeroed, those the mode leaves out zero."""
    out = {}
    for name in ROUTINES[routine][1]:
        a = (c[name] * (compared[:, None] if c[name].ndim == 2 else compared)).astype(np.float32)
        out[name] = np.zeros_like(a) if name in MODES[routine][mode] else a
    return out


def _march(routine, prof, field, c, p, v, j):
    """-> the restatement's differentiable outputs, in the order of the routine's seeds."""
    if routine == "rays":
        return cable_ad.trace_cable(prof, c["radius"], c["length"], p, v, j, c["ds"])
    if routine == "opl":
        return cable_ad.trace_cable_opl(prof, c["radius"], c["length"], p, v, j, c["ds"])
    return cable_ad.trace_cable_field(prof, field, c["radius"], c["length"], p, v, j, c["ds"])


def _autograd(c, routine, j, compared, pos, vel, dtype):
    """torch.autograd of L = sum <seed, output> through the routine's restatement on the compared rays (the seeds of the
    others are zero: they add nothing to any gradient), one forward, one backward per mode ->
    dict(out=the integral or None, mode: (profile gradients..., dpos, dvel)), per-ray results scattered back to every ray."""
    grids, seed_names, integral = ROUTINES[routine][:3]
    idx = np.nonzero(compared)[0]

    def full(a):
        out = np.zeros((N_RAYS,) + a.shape[1:], a.dtype)
        out[idx] = a
        return out
    prof, field = _T(c["prof"], dtype).requires_grad_(True), _T(c["field"], dtype).requires_grad_(True)
    p, v = _T(pos[idx], dtype).requires_grad_(True), _T(vel[idx], dtype).requires_grad_(True)
    outs = _march(routine, prof, field, c, p, v, j[idx].astype(np.int64))
    r = dict(out=full(outs[2].detach().numpy()) if integral else None)
    wrt = [dict(prof=prof, field=field)[g] for g in grids] + [p, v]
    for mode in MODES[routine]:
        s = seeds_of(c, routine, mode, compared)
        L = sum((o * _T(s[name][idx], dtype)).sum() for o, name in zip(outs, seed_names))
        g = torch.autograd.grad(L, wrt, retain_graph=True, allow_unused=True)
        g = [torch.zeros_like(w) if t is None else t for t, w in zip(g, wrt)]
        r[mode] = tuple(t.numpy() for t in g[:-2]) + (full(g[-2].numpy()), full(g[-1].numpy()))
    return r


def _nudged(a, rng):
    """A copy of the float32 array whose non-zero components are moved by one ulp, each with probability 1/2, up or down."""
    a = np.asarray(a, np.float32)
    move = (rng.random(a.shape) < 0.5) & (a != 0)
    towards = np.where(rng.random(a.shape) < 0.5, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32)
    return np.where(move, np.nextafter(a, towards), a).astype(np.float32)


def inputs(seed):
    """The N_RUNS pairs (pos, vel) the yardstick's float32 runs start from: the configuration's, and four copies nudged by
    an ulp from a fixed generator per seed.  A nudge that takes a ray through other cells of the profile than the float32
    run at the inputs (a start exactly on a knot, as the third fixed ray's at r == radius) is withdrawn for that ray: across
    a knot n' jumps, so that run would measure the jump (measured on that ray: up to 0.4 of its gradient), not rounding,
    and one such ray would lift the bound of a whole configuration to its cap."""
    if seed not in _inputs:
        c, b = config(seed), base(seed)
        rng = np.random.default_rng(8800 + seed)
        runs = [(c["pos"], c["vel"])]
        for _ in range(N_RUNS - 1):
            pos, vel = _nudged(c["pos"], rng), _nudged(c["vel"], rng)
            same = (_records(c, b["j"], torch.float32, pos, vel)[3] == b["cells"])[:, None]
            runs.append((np.where(same, pos, c["pos"]), np.where(same, vel, c["vel"])))
        _inputs[seed] = runs
    return _inputs[seed]


def reference(seed, routine):
    """-> dict(hi, lo): float64 autograd of the restatement (the referee) and N_RUNS float32 runs of it (the yardstick's
    ensemble), from inputs(seed).  One fp32 run is one draw of a heavy-tailed rounding error; the largest of five against
    float64 is what an equally valid fp32 evaluation of these rays can give, and the nudged inputs put the march's own
    amplification of an input ulp into it."""
    if (seed, routine) in _refs:
        return _refs[seed, routine]
    c, b = config(seed), base(seed)
    hi = _autograd(c, routine, b["j"], b["compared"], c["pos"], c["vel"], torch.float64)
    lo = []
    for pos, vel in inputs(seed):
        lo.append(_autograd(c, routine, b["j"], b["compared"], pos, vel, torch.float32))
    _refs[seed, routine] = dict(hi=hi, lo=lo)
    return _refs[seed, routine]


# ---- the host build -------------------------------------------------------------------------------------------------
def host_forward(c, routine):
    if routine == "opl":
        return H.trace_cable_opl(c["prof"], c["radius"], c["length"], c["pos"], c["vel"], c["tg"], c["ds"])
    if routine == "field":
        return H.trace_cable_field(c["prof"], c["field"], c["radius"], c["length"], c["pos"], c["vel"], c["tg"], c["ds"])
    return HC.trace_cable(c["prof"], c["radius"], c["length"], c["pos"], c["vel"], c["tg"], c["ds"])


def host_back(c, routine, k, seeds, mode="all", sel=slice(None), field=None):
    """The host build of the routine's adjoint with the seeds of `mode` (those it leaves out: null pointers; the ray-state
    adjoint has no optional seed), on the rays `sel`; k: the record of base(seed)["k"] (xt, vt, rec_steps)."""
    s = [None if name in MODES[routine][mode] else seeds[name][sel] for name in ROUTINES[routine][1]]
    if routine == "rays":
        return HC.backtrace_cable_rays(c["prof"], c["radius"], c["length"], c["pos"][sel], c["vel"][sel], c["tg"][sel], *s,
                                       c["ds"])
    rec = (c["pos"][sel], k["xt"][sel], k["vt"][sel], k["rec_steps"][sel])
    if routine == "opl":
        return H.backtrace_cable_opl(c["prof"], c["radius"], c["length"], *rec, *s, c["ds"])
    return H.backtrace_cable_field(c["prof"], c["field"] if field is None else field, c["radius"], c["length"], *rec, *s,
                                   c["ds"])


def host(seed, routine):
    """(forward, adjoint with every seed set on every ray) of the host build: what the kernels must give bit for bit."""
    if (seed, routine) not in _hosts:
        c = config(seed)
        k = host_forward(c, routine)
        _hosts[seed, routine] = (k, host_back(c, routine, base(seed)["k"], c))
    return _hosts[seed, routine]


# ---- errors and the bound -------------------------------------------------------------------------------------------
def _out_err(x, x64, m):
    return float((np.abs(np.asarray(x, np.float64) - x64)[m] / np.abs(x64[m])).max())


def output_errors(seed, routine, got):
    """[(quantity, e_prod, e_ref, cap)] of the routine's integral `got` against the float64 run: the largest relative error
    over the compared rays with j > 0; e_ref the largest over the N_RUNS float32 runs."""
    b, ref = base(seed), reference(seed, routine)
    m = b["compared"] & (b["j"] > 0)
    x64 = ref["hi"]["out"]
    assert (x64[m] > 0).all()
    return [(ROUTINES[routine][2], _out_err(got, x64, m), max(_out_err(lo["out"], x64, m) for lo in ref["lo"]), CAPS["out"])]


def adjoint_errors(seed, routine, mode, dpos, dvel, grids):
    """[(quantity, e_prod, e_ref, cap, |gradient|)] of an adjoint's results against float64 autograd: the largest rel_err of
    (dpos, dvel) over the compared rays and the rel-L2 of every profile gradient; e_ref the largest over the N_RUNS float32
    runs."""
    b, ref = base(seed), reference(seed, routine)
    hi, los = ref["hi"][mode], [lo[mode] for lo in ref["lo"]]
    cmp_ = b["compared"]
    rows = [("rays", float(rel_err(dpos, dvel, hi[-2], hi[-1])[cmp_].max()),
             max(float(rel_err(lo[-2], lo[-1], hi[-2], hi[-1])[cmp_].max()) for lo in los), CAPS["rays"],
             float(np.abs(np.concatenate([hi[-2], hi[-1]], 1)[cmp_]).max()))]
    for i, (g, label) in enumerate(zip(grids, ROUTINES[routine][4])):
        norm = float(np.linalg.norm(hi[i]))
        if norm == 0:                                       # dL/dfield without dtau: exactly zero on every side
            assert not np.asarray(g).any() and not any(lo[i].any() for lo in los), label
            continue
        rows.append((label, cases.rel_l2(g, hi[i]), max(cases.rel_l2(lo[i], hi[i]) for lo in los), CAPS["grid"], norm))
    return rows


def report(tag, rows):
    """Prints e_prod, e_ref, their ratio and the bound per quantity; -> the rows that miss the bound."""
    bad = []
    for name, e_prod, e_ref, cap, *_ in rows:
        b = bound(e_ref, cap)
        print(f"{tag} {name}: e_prod {e_prod:.3e} e_ref {e_ref:.3e} ratio {e_prod / max(e_ref, FLOOR):.2f} bound {b:.3e}")
        if not e_prod <= b:
            bad.append((name, e_prod, e_ref, b))
    return bad


def cancellation(c, routine, k, seeds, mode, key):
    """sum_i |c_i| / |sum_i c_i| per profile entry, c_i the host build's contribution of ray i to the gradient `key`: how
    much of what the rays add to an entry cancels.  -> the largest over the entries that matter (|sum| above 1e-3 of the
    largest entry)."""
    seeded = np.any([seeds[name].reshape(N_RAYS, -1).any(1) for name in ROUTINES[routine][1]], 0)
    per_ray = np.stack([host_back(c, routine, k, seeds, mode, sel=slice(i, i + 1))[key] for i in np.nonzero(seeded)[0]])
    tot = per_ray.sum(0)
    big = np.abs(tot) > 1e-3 * np.abs(tot).max()
    return float((np.abs(per_ray).sum(0)[big] / np.abs(tot[big])).max())
