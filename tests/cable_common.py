"""What the fibre-march test files (test_cable_raygrad.py, test_cable_opl.py, test_cable_field.py, test_cable_fuzz.py) and
cable_fuzz_common.py share: the profiles, scenes and ray sets, the host build of the ray-state adjoint, the second profile,
the seed modes and the bars.  A plain module: no fixtures, no tests."""
import itertools

import numpy as np

import cases
import hostcheck_lib as HC
from raygrad_common import _unit

MAX_DROPPED = 0.20      # share of a scene's rays that may be left out as not tie-free


def profile(kind):
    if kind == "luneburg65":                               # the profile of test_cable_variants
        return np.sqrt(2.0 - np.linspace(0, 1, 65) ** 2).astype(np.float32)
    if kind == "random33":
        return (1.0 + 0.5 * np.random.default_rng(9).random(33)).astype(np.float32)
    if kind == "two":
        return np.array([1.5, 1.3], np.float32)
    raise KeyError(kind)


SCENES = {
    # name: (profile, radius, length, ds in radial samples h = radius / (rres - 1), or None for radius / rres / 2)
    # The lengths keep every march within about 300 iterations: over more, the fp32 state drifts past TIE_TOL from the
    # fp64 one on most rays (65 samples and 780 iterations: 88 % of the rays) and nothing is left to compare.
    "luneburg65_half": ("luneburg65", 1.0, 2.0, None),
    "random33_half": ("random33", 1.0, 1.2, 0.25),
    "two_samples": ("two", 0.7, 2.5, 0.012),
    # 1.7 samples a step: a march down y = 0..7 also stays within 300 iterations, but then the fp32 rounding of y alone
    # (half an ulp of 4..8 an iteration) passes TIE_TOL on a fifth of the rays; half that length keeps them
    "luneburg65_multi": ("luneburg65", 1.0, 3.5, 1.7),
}


def ray_sets(radius, length, ds, seed):
    """-> {name: (pos, vel)}: inside, on the axis, beyond the radius, before y = 0 and past the far end."""
    rng = np.random.default_rng(seed)
    n = 96
    out = {}

    def disc(rmax, rmin=0.0):
        ang = rng.uniform(0, 2 * np.pi, n)
        rad = radius * np.sqrt(rng.uniform((rmin / rmax) ** 2, 1, n)) * rmax
        return radius + rad * np.cos(ang), radius + rad * np.sin(ang)

    def fwd(spread=0.08, sign=1.0):
        d = rng.normal(0, spread, (n, 3)); d[:, 1] = sign
        return _unit(d)
    x, z = disc(0.8)
    out["inside"] = (np.stack([x, np.full(n, 0.37 * ds), z], -1), fwd())
    # on the axis heading straight down it (r < 1e-6 throughout), starting anywhere along the fibre; the last 8 do not
    # move at all: they use every step the forward allows and keep the record they started with
    p = np.stack([np.full(n, radius), rng.uniform(0, 0.5, n) * length, np.full(n, radius)], -1)
    d = np.tile([[0.0, 1.0, 0.0]], (n, 1)); d[-8:] = 0.0
    out["axis"] = (p, d)
    # beyond the radius: half heading inwards (they enter), half outwards (they stop on the first iteration)
    x, z = disc(1.2, 1.02)
    p = np.stack([x, rng.uniform(0.05, 0.5, n) * length, z], -1)
    d = fwd(0.05)
    inward = np.stack([radius - x, np.zeros(n), radius - z], -1) / radius
    d = _unit(d + np.where(np.arange(n)[:, None] < n // 2, 0.6, -0.6) * inward)
    out["beyond"] = (p, d)
    # before y = 0 heading in, and past the far end: half heading on (first-iteration stop), half heading back in
    x, z = disc(0.7)
    out["before"] = (np.stack([x, -rng.uniform(0.5, 20, n) * ds, z], -1), fwd())
    x, z = disc(0.7)
    out["past"] = (np.stack([x, length + rng.uniform(0.5, 20, n) * ds, z], -1),
                   fwd(sign=np.where(np.arange(n) < n // 2, 1.0, -1.0)))
    return {k: (a.astype(np.float32), b.astype(np.float32)) for k, (a, b) in out.items()}


def scene(name, seed=0):
    kind, radius, length, step = SCENES[name]
    prof = profile(kind)
    ds = radius / len(prof) / 2 if step is None else step * radius / (len(prof) - 1)      # core/fiber_opt.py:156
    ds = float(np.float32(ds))
    sets = ray_sets(radius, length, ds, seed)
    pos = np.concatenate([s[0] for s in sets.values()])
    vel = np.concatenate([s[1] for s in sets.values()])
    labels = np.concatenate([[k] * len(s[0]) for k, s in sets.items()])
    rng = np.random.default_rng(seed + 11)
    n = len(pos)
    # targets behind the start (the record stays the input, j* = 0), near the path ahead (interior j*), and far beyond
    # the end of the march along the ray's heading (the last state is the closest, j* = K)
    kind_t = rng.integers(0, 3, n)
    t_on = rng.uniform(0.15, 0.6, n) * length
    along = np.where(kind_t == 0, -0.3 * length, np.where(kind_t == 1, t_on, 20.0 * length))
    tg = pos + along[:, None] * vel + (kind_t == 1)[:, None] * rng.normal(0, 0.02 * radius, (n, 3))
    tg[vel.any(1) == 0] += [0.0, 0.5, 0.0]                 # the rays that never move: any target, j* = 0
    dx = rng.normal(size=pos.shape).astype(np.float32)
    dv = rng.normal(size=pos.shape).astype(np.float32)
    return dict(prof=prof, radius=radius, length=length, ds=ds, pos=pos, vel=vel, tg=tg.astype(np.float32),
                labels=labels, dx=dx, dv=dv)


def host(s):
    return HC.backtrace_cable_rays(s["prof"], s["radius"], s["length"], s["pos"], s["vel"], s["tg"], s["dx"], s["dv"],
                                    s["ds"])


def _fuzz(seed, rres=None):
    c = cases.fuzz_cable_config(seed)
    s = dict(prof=c["prof"], radius=c["radius"], length=c["length"], ds=c["ds"], pos=c["pos"], vel=c["vel"], tg=c["tg"],
             dx=c["dx"], dv=c["dv"])
    if rres is not None:       # a profile above kCableMaxRes (4096): the kernels read it from global memory
        s["prof"] = (1.5 - 0.4 * np.linspace(0, 1, rres) ** 2 + 0.01 * np.sin(np.arange(rres))).astype(np.float32)
        s["ds"] = float(np.float32(s["radius"] / (rres - 1) * 40.0))
    return s


# ---- the integrals ----------------------------------------------------------------------------------------------------
ATOMIC_TOL = 2e-5       # profile gradients, kernel vs host build: only the order of the sums differs (tests/test_gpu_parity.py's bar)
OPL_MODES = {"all": (), "dopl": ("dx", "dv"), "rays": ("dopl",)}      # mode: the seeds it leaves out (null pointers / zeros)
FIELD_MODES = {"all": (), "dtau": ("dx", "dv"), "rays": ("dtau",)}      # mode: the seeds it leaves out (null pointers / zeros)


def field_profile(rres, seed):
    """The second profile: positive (0.25 .. 1.05), not monotone, of `rres` samples."""
    rng = np.random.default_rng(7300 + seed)
    return (0.6 + 0.3 * np.sin(7.0 * np.linspace(0, 1, rres) + seed) + 0.1 * rng.random(rres) - 0.05).astype(np.float32)


COMBOS = [c for c in itertools.product((True, False), repeat=3) if any(c)]      # (want_rif, want_field, want_rays): seven
