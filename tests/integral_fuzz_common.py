"""What tests/test_integral_fuzz.py is built from: the configurations (cases.fuzz_config plus the second fields and the
seeds on the integrals), the float64 and float32 torch.autograd runs of the four restatements (oracle/torch_ad.trace,
tests/integral_ad), the host build of the product's per-ray routines, the mask of compared rays
and the bound.  A plain module: no fixtures, no tests.  Everything is computed once per (seed, routine) and handed out
unchanged."""
import numpy as np
import torch

import cases
import hostcheck_lib as HC
import integral_ad
import integral_common as IC
import integral_host as OH
from oracle import torch_ad
from raygrad_common import GRAD_TOL, TIE_TOL, rel_err

SEEDS = tuple(range(16))
TWO_VOXEL = (0, 4, 7, 14)          # cases.fuzz_config(seed)["res"] has a 2-voxel axis: every cell is a boundary cell
FLOOR = 2.4e-7                     # 2^-22: a few fp32 roundings
MARGIN = 8.0                       # room for another, equally valid order of the fp32 operations
CAPS = dict(out=1e-4, rays=GRAD_TOL, grid=GRAD_TOL)      # the project's bars: never exceeded whatever the yardstick says
MAX_TAU = np.float32(5.5)          # tests/test_emission.py::_with_fields

# routine -> (names of its grids, names of its seeds, names of the host result's grid gradients, their labels)
ROUTINES = {
    "rays": (("rif",), ("dx", "dv"), (), ()),
    "opl": (("rif",), ("dx", "dv", "dopl"), ("grad",), ("dL/drif",)),
    "field": (("rif", "field"), ("dx", "dv", "dtau"), ("grad", "grad_field"), ("dL/drif", "dL/dfield")),
    "emission": (("rif", "emission", "absorption"), ("dx", "dv", "drad", "dtau"),
                 ("grad", "grad_emission", "grad_absorption"), ("dL/drif", "dL/de", "dL/da")),
}
# which seeds a mode leaves out (null pointers on the host build, zeros in autograd): tests/test_emission.py::MODES
NULLS = {"all": (), "noray": ("dx", "dv"), "drad": ("dx", "dv", "dtau"), "dtau": ("dx", "dv", "drad")}
MODES = {"rays": ("all",), "opl": ("all", "noray"), "field": ("all", "noray"), "emission": ("all", "noray", "drad", "dtau")}
OUTPUTS = {"rays": (), "opl": ("opl",), "field": ("tau",), "emission": ("rad", "tau")}

_configs, _masks, _ads, _hosts = {}, {}, {}, {}


def config(seed):
    """cases.fuzz_config(seed) with what the integrals need, drawn from a generator of this module's own: the seeds on opl,
    tau and rad, a second field, an emission and an absorption (tests/integral_common.py::make_field), the absorption
    scaled as tests/test_emission.py::_with_fields scales it (the largest tau of a ray that leaves the box is 5.5)."""
    if seed in _configs:
        return _configs[seed]
    c = dict(cases.fuzz_config(seed))
    rng = np.random.default_rng(seed + 7100)
    n = len(c["pos"])
    for key in ("dopl", "dtau", "drad"):
        c[key] = rng.normal(size=n).astype(np.float32)
    f_seed, e_seed, a_seed = (int(v) for v in rng.integers(0, 1 << 20, 3))
    c["field"] = IC.make_field(c["rif"].shape, f_seed)
    c["emission"] = IC.make_field(c["rif"].shape, e_seed)
    unit = IC.make_field(c["rif"].shape, a_seed)
    k = OH.trace_field(c["rif"], unit, c["res"], c["pos"], c["vel"], c["h"], c["ds"])
    ok = k["steps"] < IC.max_steps_fwd(c["res"], c["h"], c["ds"])
    c["absorption"] = (unit * (MAX_TAU / k["tau"][ok].max())).astype(np.float32)
    assert n == 600 and IC.max_steps_fwd(c["res"], c["h"], c["ds"]) <= 164
    assert min(c[key].min() for key in ("field", "emission")) > 0.5 and c["absorption"].min() > 0
    _configs[seed] = c
    return c


def _T(a, dtype):
    return torch.tensor(np.asarray(a), dtype=dtype)


def _march(routine, grids, p, v, h, ds):
    """-> the restatement's differentiable outputs, in the order of the routine's seeds."""
    if routine == "rays":
        return torch_ad.trace(*grids, p, v, h, ds)
    fn = dict(opl=integral_ad.trace_opl, field=integral_ad.trace_field, emission=integral_ad.trace_emission)[routine]
    return fn(*grids, p, v, h, ds)[:-1]


def masks(oracle, seed):
    """-> dict(k, ms, compared, nonzero, failed, tau64): the host fp32 forward, the float64 tau of the absorption, and the
    rays that are tie-free for both the product and the yardstick: the fp32 host build and the fp64 oracle leave on the same
    iteration with exit samples within TIE_TOL (tests/integral_common.py::reference), and so do the float32 and the float64 torch
    runs.  `nonzero`: compared rays whose float64 opl is not zero (they sampled inside the box, so every integral of a
    positive field is non-zero)."""
    if seed in _masks:
        return _masks[seed]
    c = config(seed)
    k, tie_prod, opl64, ms = IC.reference(oracle, c, ("integral_fuzz", seed))
    with torch.no_grad():
        lo, hi = (integral_ad.trace_opl(_T(c["rif"], dt), _T(c["pos"], dt), _T(c["vel"], dt), c["h"], c["ds"])
                  for dt in (torch.float32, torch.float64))
        tau64 = integral_ad.trace_field(*(_T(c[key], torch.float64) for key in ("rif", "absorption", "pos", "vel")),
                                        c["h"], c["ds"])[2].numpy()
    ms_ad = int(4 * c["h"] * max(c["rif"].shape) / c["ds"])
    close = lambda a, b: (a.double() - b).abs().max(1).values <= TIE_TOL      # noqa: E731
    tie_ref = ((lo[3] < ms_ad) & (lo[3] == hi[3]) & close(lo[0], hi[0]) & close(lo[1], hi[1])).numpy()
    compared = tie_prod & tie_ref
    assert np.array_equal(hi[3].numpy()[compared], k["steps"][compared].astype(np.int64))
    assert np.array_equal(hi[2].numpy(), opl64)
    _masks[seed] = dict(k=k, ms=ms, compared=compared, nonzero=compared & (opl64 != 0), failed=k["steps"] >= ms, tau64=tau64)
    return _masks[seed]


def seeds_of(c, routine, mode, compared):
    """{name: array}: the seeds of a mode, those of the rays that are not compared zeroed, those the mode leaves out zero."""
    out = {}
    for name in ROUTINES[routine][1]:
        a = c[name] * (compared[:, None] if c[name].ndim == 2 else compared)
        out[name] = np.zeros_like(a) if name in NULLS[mode] else a.astype(np.float32)
    return out


def autograd(oracle, seed, routine):
    """{dtype: dict(out={name: array}, mode: (grid gradients..., dpos, dvel))} for torch.float64 (the referee) and
    torch.float32 (the yardstick): torch.autograd of L = sum <seed, output> through the routine's restatement, one forward
    and one backward per mode.  Only the compared rays are marched: the seeds of the others are zero, so they add nothing to
    any gradient, and without the rays at rest the loop ends when the last compared ray has left.  Their rows of the
    per-ray results are zero."""
    if (seed, routine) in _ads:
        return _ads[seed, routine]
    c, m = config(seed), masks(oracle, seed)
    grids, seed_names = ROUTINES[routine][:2]
    idx = np.nonzero(m["compared"])[0]
    n = len(c["pos"])

    def full(a):
        out = np.zeros((n,) + a.shape[1:], a.dtype)
        out[idx] = a
        return out
    res = {}
    for dt in (torch.float64, torch.float32):
        leaves = [_T(c[key], dt).requires_grad_(True) for key in grids] + \
                 [_T(c[key][idx], dt).requires_grad_(True) for key in ("pos", "vel")]
        outs = _march(routine, leaves[:-2], leaves[-2], leaves[-1], c["h"], c["ds"])
        r = dict(out={name: full(o.detach().numpy()) for name, o in zip(OUTPUTS[routine], outs[2:])})
        for mode in MODES[routine]:
            s = seeds_of(c, routine, mode, m["compared"])
            L = sum((o * _T(s[name][idx], dt)).sum() for o, name in zip(outs, seed_names))
            wrt = leaves[-2:] if routine == "rays" else leaves
            g = torch.autograd.grad(L, wrt, retain_graph=True)
            r[mode] = tuple(t.numpy().reshape(-1) for t in g[:-2]) + (full(g[-2].numpy()), full(g[-1].numpy()))
        res[dt] = r
    _ads[seed, routine] = res
    return res


def host_forward(c, routine):
    if routine == "rays":
        return HC.trace(c["rif"], c["res"], c["pos"], c["vel"], c["h"], c["ds"])
    if routine == "opl":
        return OH.trace_opl(c["rif"], c["res"], c["pos"], c["vel"], c["h"], c["ds"])
    if routine == "field":
        return OH.trace_field(c["rif"], c["field"], c["res"], c["pos"], c["vel"], c["h"], c["ds"])
    return OH.trace_emission(c["rif"], c["emission"], c["absorption"], c["res"], c["pos"], c["vel"], c["h"], c["ds"])


def host_back(c, routine, k, seeds, mode="all", sel=slice(None), **kw):
    """The host build of the routine's adjoint with the seeds of `mode` (those it leaves out: null pointers), on the rays
    `sel`."""
    s = [None if name in NULLS[mode] else seeds[name][sel] for name in ROUTINES[routine][1]]
    rays = [c["pos"][sel], c["vel"][sel], k["xt"][sel], k["vt"][sel], k["steps"][sel]]
    if routine == "rays":
        return HC.backtrace_rays(c["rif"], c["res"], *rays, *s, c["h"], c["ds"], **kw)
    if routine == "opl":
        return OH.backtrace_opl(c["rif"], c["res"], *rays, *s, c["h"], c["ds"], **kw)
    if routine == "field":
        return OH.backtrace_field(c["rif"], c["field"], c["res"], *rays, *s, c["h"], c["ds"], **kw)
    return OH.backtrace_emission(c["rif"], c["emission"], c["absorption"], c["res"], *rays, k["tau"][sel], *s, c["h"],
                                 c["ds"], **kw)


def host(seed, routine):
    """(forward, adjoint with every seed set on every ray and the flag on) of the host build: what the kernels must give."""
    if (seed, routine) not in _hosts:
        c = config(seed)
        k = host_forward(c, routine)
        kw = {} if routine == "rays" else dict(corrected_h=True)
        _hosts[seed, routine] = (k, host_back(c, routine, k, c, **kw))
    return _hosts[seed, routine]


def bound(e_ref, cap):
    return min(MARGIN * max(e_ref, FLOOR), cap)


def out_err(x, x64, nonzero):
    return float((np.abs(np.asarray(x, np.float64) - x64)[nonzero] / np.abs(x64[nonzero])).max())


def output_errors(oracle, seed, routine, got):
    """[(quantity, e_prod, e_ref, cap)] of the routine's outputs `got` ({name: array}) against the float64 run, over the
    compared rays with a non-zero integral."""
    m, ad = masks(oracle, seed), autograd(oracle, seed, routine)
    hi, lo = ad[torch.float64]["out"], ad[torch.float32]["out"]
    return [(name, out_err(got[name], hi[name], m["nonzero"]), out_err(lo[name], hi[name], m["nonzero"]), CAPS["out"])
            for name in OUTPUTS[routine]]


def adjoint_errors(oracle, seed, routine, mode, dpos, dvel, grids):
    """[(quantity, e_prod, e_ref, cap, |gradient|)] of an adjoint's results against float64 autograd: the largest rel_err of
    (dpos, dvel) over the compared rays, and the rel-L2 of every grid gradient."""
    m, ad = masks(oracle, seed), autograd(oracle, seed, routine)
    hi, lo = ad[torch.float64][mode], ad[torch.float32][mode]
    cmp_ = m["compared"]
    rows = [("rays", float(rel_err(dpos, dvel, hi[-2], hi[-1])[cmp_].max()),
             float(rel_err(lo[-2], lo[-1], hi[-2], hi[-1])[cmp_].max()), CAPS["rays"],
             float(np.abs(np.concatenate([hi[-2], hi[-1]], 1)[cmp_]).max()))]
    for i, (g, label) in enumerate(zip(grids, ROUTINES[routine][3])):
        rows.append((label, cases.rel_l2(g, hi[i]), cases.rel_l2(lo[i], hi[i]), CAPS["grid"], float(np.linalg.norm(hi[i]))))
    return rows


def report(tag, rows):
    """Prints e_prod, e_ref and their ratio per quantity; -> the rows that miss the bound."""
    bad = []
    for name, e_prod, e_ref, cap, *_ in rows:
        b = bound(e_ref, cap)
        print(f"{tag} {name}: e_prod {e_prod:.3e} e_ref {e_ref:.3e} ratio {e_prod / max(e_ref, FLOOR):.2f} bound {b:.3e}")
        if not e_prod <= b:
            bad.append((name, e_prod, e_ref, b))
    return bad


def _quiet_rays(c):
    """(rays at rest outside the box, rays outside the box that point away from it), from the geometry alone; the far faces
    with a margin, so that no rounding of (res - 1) h decides."""
    ext = (np.array(c["res"], np.float64) - 1) * c["h"]
    pos, vel = c["pos"].astype(np.float64), c["vel"].astype(np.float64)
    below, above = pos < 0, pos > ext * (1 + 1e-6)
    rest = ~vel.any(1) & (below | above).any(1)
    away = ((below & (vel < 0)) | (above & (vel > 0))).any(1)
    return rest, away
