"""Seeded fuzz of the fibre march's three exact adjoints against float64 autograd: backtrace_cable_rays, trace_cable_opl /
backtrace_cable_opl and trace_cable_field / backtrace_cable_field on the 16 configurations of tests/cable_fuzz_common.py --
profiles of 2, 3, 5, 9, 17, 33, 64, 127 and 200 samples that fall (Luneburg), are random, rise outwards or are not monotone,
steps of 0.3 .. 3 radial samples (on 2 and 3 samples a ray crosses the fibre in two steps), 400 rays of which a sixth start
beyond the radius (i0 == i1 == rres - 1, w0 from the clamped index), a tenth have x == radius or z == radius, a quarter head
towards -y and the last 8 start from rest -- where the fixed scenes of tests/test_cable_raygrad.py have 65, 33 and 2 samples,
falling or random profiles and ray sets built so that nothing awkward happens.

Referee: float64 torch.autograd through tests/cable_ad, the record's iteration j
handed in.  A ray is compared when (1) the float32 and float64 restatement records agree within TIE_TOL, (2) the host build's
record is within TIE_TOL of the float64 one, (3) no sample in front of its record lies within 0.02 radius of the axis without
being on it, (4) its float64 ray gradient is at most 30 times its seed; the seeds of every other ray are zero on all sides.
1, 3 and 4 come from the restatement alone.  Yardstick: e_ref, the largest error against float64 among five float32 runs of
the same restatement, one at the inputs and four at inputs nudged by an ulp.  The bound is integral_fuzz_common.bound:
    e_prod <= 8 max(e_ref, 2.4e-7),   and never above 1e-4 (opl, tau) or GRAD_TOL = 1e-3 (rays, profile gradients).
A nudge that takes a ray through other cells of the profile is withdrawn for that ray (cable_fuzz_common.inputs): the third
fixed ray starts exactly on the knot r == radius, and with it nudged inwards the yardstick stood at up to 0.4 and the bounds
of the configuration at their caps.
SEEDS is the first 16 of range(64) that keep 85 % of their rays under 1, 3 and 4 (test_seed_rule): 0, 12, 13 and 17 do not.
Two things were added to the generator so that the mutations below are seen: 15 % of the rays inside start at 0.025 .. 0.05
radius, just outside the band of criterion 3, and every seventh configuration (seed 6 here) is a thin fibre of radius
0.01 .. 0.02, where the product's absolute on-axis threshold is no longer far below that band.

CPU tier: the host build of the per-ray routines against the referee, the identities the fixed scenes assert, bit for bit.
GPU tier: the kernels against the host build (per-ray results and statistics bit for bit), their profile gradients against
the referee under the same bound and against the host build within ATOMIC_TOL, every output combination of the field adjoint,
launches of 1, 63, 65 and 257 rays on 2 and 200 samples, and the three autograd classes end to end.

Compared rays per seed of SEEDS (of 400; at least 320 asked for), criterion 2 alone removing 0 or 1 ray everywhere:
  seed      1   2   3   4   5   6   7   8   9  10  11  14  15  16  18  19
  samples   3   5   9  17  33  64 127 200   2   3   5  33  64 127   2   3
  compared 373 395 365 387 388 357 377 390 346 394 373 390 388 376 392 395
and 39 compared rays from rest have a record that moved (8 asked for).

Largest e_prod / max(e_ref, 2.4e-7) per quantity over the 16 seeds and all modes (8 allowed):
  host build   backtrace_cable_rays  rays 1.42 (seed 1)
               opl     opl 1.00 (14)   rays 1.68 (1)   dL/dprofile 3.02 (9, dopl alone: 1.55e-5 against 5.1e-6)
               field   tau 0.92 (14)   rays 1.54 (1)   dL/dprofile 2.45 (9, dtau alone)   dL/dfield 1.70 (14)
  kernels      opl     rays 1.66 (1)   dL/dprofile 2.25 (9)
  (MI355X)     field   rays 1.55 (1)   dL/dprofile 2.62 (9)   dL/dfield 1.61 (14)
  classes      rays 1.40 (1)   opl 1.80 (7)   opl rays 1.66 (1)   field rays 1.50 (1)   every profile gradient below 0.9
The kernels' profile gradients are at most 1.3e-7 rel-L2 from the host build's (ATOMIC_TOL = 2e-5): no configuration misses
it, so the cancellation report of test_kernel_gradients_match_float64_autograd has had nothing to say.  On seed 19 (3
samples, a step of 2.2 of them) the yardstick of (dpos, dvel) stands at 5e-3, above the cap: ray 57 bounces past the axis at
0.04 radius under kicks of 0.6 in v per step, and an ulp on its start moves its gradient by that much in float64 too (its
first-order amplification is 1.3: criterion 4 cannot see it).  The cap (1e-3) is the bound there; the product is at 4.6e-6.

Mutation checks (each applied by hand to a scratch copy of csrc/drrt_device.h, the 194 tests of the CPU tier run on it):
  * sH of cable_adj_recur scaled by 1 + 1e-3: 107 of the 112 cases of test_adjoint_matches_float64_autograd fail, all 80
    with ray seeds and at least 5 of the 7 cases of every seed.
  * the sign of gvh swapped on the i1 tap (both reverse marches): all 96 opl and field cases fail (the ray-state adjoint
    has no profile gradient).
  * CableOplTerm::dn without 2 dopl n: the 32 opl cases with dopl fail (modes `all` and `dopl` on every seed).
  * the field sink's two weights swapped: the 32 field cases with dtau fail.
  * c.tiny tested against 1e-3f: test_enough_rays_are_compared[6] fails -- on the thin fibre the product loses the records
    of 34 rays that start within 1e-3 of the axis, and criterion 2 may remove 20.  With the radii the generator first had
    (0.1 .. 2 everywhere) nothing failed: every ray the mutation touches lies inside the band criterion 3 leaves out.
  * w0 of cyl_locate from the unclamped index: nothing fails, and nothing can.  The clamp acts only beyond the radius, where
    i0 == i1: both taps read the same sample v, n = v w0 + v (1 - w0), n' = 0, and the two contributions of a tap pair land
    on one entry as val (w0 + (1 - w0)).  Whatever w0 is, the results differ by roundings: the mutant is equivalent."""
import numpy as np
import pytest
import torch

from cable_common import ATOMIC_TOL, COMBOS
from cable_fuzz_common import LENGTHS, MODES, N_RAYS, ROUTINES, SEEDS, config
import cable_fuzz_common as CF
import cases
import hostcheck_lib as HC
from raygrad_common import _t

INTEGRALS = ("opl", "field")
ADJOINTS = [(seed, routine, mode) for seed in SEEDS for routine in ROUTINES for mode in MODES[routine]]
_bits = lambda a: np.ascontiguousarray(a).view(np.uint32)      # noqa: E731


# ---- CPU tier: the configurations -----------------------------------------------------------------------------------
def test_seed_rule():
    """SEEDS is the first 16 of range(64) whose configuration keeps at least 85 % of its rays under the criteria that come
    from the restatement alone, in order; it has 2 and 3 samples at least twice each and every other length at least once."""
    picked = []
    for seed in range(64):
        share = CF.ref_share(seed)
        print(f"seed {seed}: rres {config(seed)['rres']}, share under criteria 1, 3, 4: {share:.3f}")
        if share >= CF.MIN_REF_SHARE:
            picked.append(seed)
        if len(picked) == 16:
            break
    assert tuple(picked) == SEEDS
    count = {rres: sum(config(seed)["rres"] == rres for seed in SEEDS) for rres in LENGTHS}
    assert count[2] >= 2 and count[3] >= 2 and min(count.values()) >= 1, count
    assert {config(seed)["shape"] for seed in SEEDS} == set(CF.SHAPES)
    assert any(config(seed)["radius"] < 0.02 for seed in SEEDS)      # a thin fibre: 1e-3 is then 5 % of the radius or more


@pytest.mark.parametrize("seed", SEEDS)
def test_enough_rays_are_compared(seed):
    """Conditions on a configuration, not measurements: what the fuzz is there for is in it (the profile length and shape of
    its seed, rays beyond the radius, on-axis coordinates, rays heading back and at rest), at least 80 % of its rays are
    compared, criterion 2 alone removes at most 5 %, and every kind of record and of ray has 10 compared rays."""
    c, b = config(seed), CF.base(seed)
    assert len(c["prof"]) == LENGTHS[seed % 9] and c["shape"] == CF.SHAPES[seed % 4] and len(c["pos"]) == N_RAYS
    d = np.diff(c["prof"].astype(np.float64))
    assert {"luneburg": (d < 0).all(), "rising": d.sum() > 0.25, "random": True,
            "wavy": len(d) < 3 or ((d > 0).any() and (d < 0).any())}[c["shape"]]
    assert 40 <= c["beyond"].sum() <= 100 and c["back"].sum() >= 60 and c["on_axis"].sum() >= 20
    assert c["rest"].sum() == 8 and not c["vel"][c["rest"]].any() and (~c["beyond"] & c["rest"]).sum() >= 6
    j, K, cmp_ = b["j"], b["K"], b["compared"]
    only_product = b["ref_ok"] & ~b["tie_prod"]
    print(f"seed {seed}: rres {c['rres']} {c['shape']}, step {c['ds'] * (c['rres'] - 1) / c['radius']:.2f} samples, iterations "
          f"max {K.max()}, j max {j.max()}; compared {cmp_.sum()} of {N_RAYS} (tie-free yardstick {b['tie_ref'].sum()}, off axis "
          f"{b['off_axis'].sum()}, tame {b['tame'].sum()}, removed by the product alone {only_product.sum()})")
    assert cmp_.mean() >= 1 - CF.MAX_DROPPED and only_product.mean() <= CF.MAX_PRODUCT_ONLY
    groups = {"j = 0": j == 0, "0 < j < K": (j > 0) & (j < K), "j = K > 0": (j == K) & (j > 0), "beyond": c["beyond"],
              "back": c["back"], "on axis": c["on_axis"]}
    for name, g in groups.items():
        assert (g & cmp_).sum() >= 10, name
    print(f"seed {seed}: compared rays that start at 0.025 .. 0.05 radius: {(c['close'] & cmp_).sum()} of {c['close'].sum()}")
    assert (c["close"] & cmp_).sum() >= 5
    # the yardstick's nudged runs are nudged: a ray keeps all six components with probability 2^-6, and the nudges withdrawn
    # because they change a ray's cells are a few rays, not a share of the configuration
    for pos, vel in CF.inputs(seed)[1:]:
        moved = (pos != c["pos"]).any(1) | (vel != c["vel"]).any(1)
        assert moved[cmp_].mean() >= 0.93, moved[cmp_].mean()


def test_rays_from_rest_that_moved():
    """Over the seed list at least 8 compared rays started from rest and have a record that moved (j > 0)."""
    moved = sum(int((config(seed)["rest"] & CF.base(seed)["compared"] & (CF.base(seed)["j"] > 0)).sum()) for seed in SEEDS)
    print(f"compared rays from rest with j > 0: {moved}")
    assert moved >= 8


# ---- CPU tier: identities, bit for bit ------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", SEEDS)
def test_forward_identities(seed):
    """The three forwards share the march: (xt, vt, dist2) and the iteration counts are cable_trace_ray's, the record's
    iteration is the one the ray-state adjoint replays; with field = profile tau is opl; j = 0 has a zero integral."""
    c = config(seed)
    t, o, f = (CF.host_forward(c, routine) for routine in ROUTINES)
    r = CF.host(seed, "rays")[1]
    for k in (o, f):
        for key in ("xt", "vt", "dist2"):
            assert np.array_equal(_bits(k[key]), _bits(t[key])), key
        assert k["ray_steps"] == t["steps_total"] and np.array_equal(k["rec_steps"], r["jstar"])
        assert np.array_equal(k["steps"], r["steps"] - r["jstar"])
    assert np.array_equal(_bits(r["xt"]), _bits(t["xt"])) and np.array_equal(_bits(r["vt"]), _bits(t["vt"]))
    same = CF.host_forward(dict(c, field=c["prof"]), "field")
    assert np.array_equal(_bits(same["tau"]), _bits(o["opl"])) and not np.array_equal(f["tau"], o["opl"])
    z = o["rec_steps"] == 0
    assert z.sum() >= 10 and not o["opl"][z].any() and not f["tau"][z].any() and (o["opl"][~z] > 0).all()


@pytest.mark.parametrize("seed", SEEDS)
def test_adjoint_identities(seed):
    """Without dtau the field adjoint is the OPL adjoint without dopl, and both give the ray-state adjoint's (dpos, dvel);
    rays with j = 0 return their seeds and add to no profile gradient: bit for bit."""
    c, k = config(seed), CF.base(seed)["k"]
    r = CF.host(seed, "rays")[1]
    o = CF.host_back(c, "opl", k, c, "rays")
    f = CF.host_back(c, "field", k, c, "rays")
    for b in (o, f):
        assert np.array_equal(b["dpos"], r["dpos"], equal_nan=True) and np.array_equal(b["dvel"], r["dvel"], equal_nan=True)
    assert np.array_equal(f["grad"], o["grad"], equal_nan=True) and np.nan_to_num(o["grad"]).any() and not f["grad_field"].any()
    z = k["rec_steps"] == 0
    for routine in ROUTINES:
        b = CF.host(seed, routine)[1] if routine == "rays" else CF.host_back(c, routine, k, c, sel=z)
        sel = z if routine == "rays" else slice(None)
        assert np.array_equal(_bits(b["dpos"][sel]), _bits(c["dx"][z])), routine
        assert np.array_equal(_bits(b["dvel"][sel]), _bits(c["dv"][z])), routine
        for key in ROUTINES[routine][3]:
            assert not b[key].any(), (routine, key)


# ---- CPU tier: against the referee ----------------------------------------------------------------------------------
@pytest.mark.parametrize("routine", INTEGRALS)
@pytest.mark.parametrize("seed", SEEDS)
def test_outputs_match_float64(seed, routine):
    """opl / tau of the host build against the float64 run over the compared rays with j > 0, under the bound."""
    k = CF.host_forward(config(seed), routine)
    assert CF.report(f"seed {seed} {routine}", CF.output_errors(seed, routine, k[ROUTINES[routine][2]])) == []


@pytest.mark.parametrize("seed,routine,mode", ADJOINTS)
def test_adjoint_matches_float64_autograd(seed, routine, mode):
    """(dpos, dvel) per ray and every profile gradient of the host build against float64 autograd, under the bound; every
    seed mode of tests/test_cable_opl.py and tests/test_cable_field.py.  Without dtau the field gradient is exactly zero."""
    c, b = config(seed), CF.base(seed)
    r = CF.host_back(c, routine, b["k"], CF.seeds_of(c, routine, mode, b["compared"]), mode)
    if routine != "rays":
        assert not r["failed"].any() and np.array_equal(r["steps"], b["j"])
    rows = CF.adjoint_errors(seed, routine, mode, r["dpos"], r["dvel"], [r[g] for g in ROUTINES[routine][3]])
    assert len(rows) == 1 + len(ROUTINES[routine][3]) - (routine == "field" and mode == "rays")
    assert all(row[4] > 0 for row in rows)
    assert CF.report(f"seed {seed} {routine} seeds={mode}", rows) == []


# ---- GPU tier -------------------------------------------------------------------------------------------------------
def _same(got, want):
    got = got.cpu().numpy()
    return np.array_equal(np.isfinite(got), np.isfinite(want)) and \
        np.array_equal(got.view(want.dtype).reshape(want.shape), want, equal_nan=True)


def _dev_forward(T, c, routine, dev, n=None):
    prof = [_t(c[key], dev) for key in (("prof",) if routine == "opl" else ("prof", "field"))]
    fn = T.trace_cable_opl if routine == "opl" else T.trace_cable_field
    return fn(*prof, c["radius"], c["length"], *(_t(c[key][:n], dev) for key in ("pos", "vel", "tg")), c["ds"])


def _dev_back(T, c, routine, k, seeds, mode, dev, n=None, **kw):
    """The routine's adjoint kernel on the first n rays -> (profile gradients [arrays, None where not asked for], dpos,
    dvel, stats)."""
    from adjointnonlinearraytracing_amd import drrt
    s = [None if name in MODES[routine][mode] else _t(seeds[name][:n], dev) for name in ROUTINES[routine][1]]
    if routine == "rays":
        out = T.backtrace_cable_rays(_t(c["prof"], dev), c["radius"], c["length"],
                                     *(_t(c[key][:n], dev) for key in ("pos", "vel", "tg")), *s, c["ds"])
    else:
        prof = [_t(c[key], dev) for key in (("prof",) if routine == "opl" else ("prof", "field"))]
        fn = T.backtrace_cable_opl if routine == "opl" else T.backtrace_cable_field
        out = fn(*prof, c["radius"], c["length"], _t(c["pos"][:n], dev), _t(k["xt"][:n], dev), _t(k["vt"][:n], dev),
                 _t(k["rec_steps"][:n].astype(np.int32), dev), *s, c["ds"], **kw)
    st = drrt.read_stats()
    return [None if g is None else g.cpu().numpy() for g in out[:-2]], out[-2], out[-1], st


def _check_against_host(c, routine, b, grads, dpos, dvel, st, want_rays=True):
    """Per-ray results bit for bit (non-finite values in the same places), the statistics equal, the profile gradients that
    were asked for within ATOMIC_TOL (cases.grads_agree: non-finite entries in the same places)."""
    if want_rays:
        assert _same(dpos, b["dpos"]) and _same(dvel, b["dvel"]), routine
    assert (st["ray_steps"], st["iters"], st["n_failed"]) == (b["ray_steps"], b["iters"], 0), routine
    for g, key in zip(grads, ROUTINES[routine][3]):
        assert g is None or (g.shape == b[key].shape and cases.grads_agree(g, b[key], ATOMIC_TOL)), (routine, key)


def _combo_kw(routine, combo):
    if routine == "opl":
        return dict(profile=combo[0], rays=combo[2])
    return dict(want_rif=combo[0], want_field=combo[1], want_rays=combo[2]) if routine == "field" else {}


@pytest.mark.gpu
@pytest.mark.parametrize("seed", SEEDS)
def test_kernels_match_host_build(gpu, seed):
    """trace_cable_opl, trace_cable_field, backtrace_cable_rays, backtrace_cable_opl and backtrace_cable_field with every
    seed set on every ray == the host build: per-ray results bit for bit, non-finite values in the same places, the
    iteration statistics equal, the profile gradients within ATOMIC_TOL.  The field adjoint runs with every output and with
    one other of COMBOS (seed % 6 of the rest: all seven over the seed list)."""
    from adjointnonlinearraytracing_amd import drrt
    c, k = config(seed), CF.base(seed)["k"]
    T = drrt.TracerC()
    other = [combo for combo in COMBOS if not all(combo)][seed % 6]
    with drrt.using(check_failed=False):
        for routine in INTEGRALS:
            h = CF.host_forward(c, routine)
            out = _dev_forward(T, c, routine, gpu)
            st = drrt.read_stats()
            for got, key in zip(out, ("xt", "vt", "dist2", ROUTINES[routine][2], "rec_steps")):
                assert _same(got, h[key]), (routine, key)
            assert (st["ray_steps"], st["iters"], st["n_failed"]) == (h["ray_steps"], h["iters"], h["n_failed"]), routine
        for routine in ROUTINES:
            b = CF.host(seed, routine)[1]
            _check_against_host(c, routine, b, *_dev_back(T, c, routine, k, c, "all", gpu))
        b = CF.host(seed, "field")[1]
        grads, dpos, dvel, st = _dev_back(T, c, "field", k, c, "all", gpu, **_combo_kw("field", other))
        assert [g is not None for g in grads] + [dpos is not None, dvel is not None] == [other[0], other[1], other[2], other[2]]
        _check_against_host(c, "field", b, grads, dpos, dvel, st, want_rays=other[2])


@pytest.mark.gpu
@pytest.mark.parametrize("seed,routine,mode", [a for a in ADJOINTS if a[1] != "rays"])
def test_kernel_gradients_match_float64_autograd(gpu, seed, routine, mode):
    """The comparison that counts: the kernels' profile gradients (atomic sums, in another order than the host build's) and
    their (dpos, dvel) against float64 autograd under the bound of the CPU tier, the seeds of the rays that are not compared
    zeroed; and the profile gradients against the host build's within ATOMIC_TOL.  Should ATOMIC_TOL be missed where the
    bound is met, the message carries the host build's own cancellation sum|c_i| / |sum c_i| over its per-ray gradients."""
    from adjointnonlinearraytracing_amd import drrt
    c, b = config(seed), CF.base(seed)
    seeds = CF.seeds_of(c, routine, mode, b["compared"])
    with drrt.using(check_failed=False):
        grads, dpos, dvel, _ = _dev_back(drrt.TracerC(), c, routine, b["k"], seeds, mode, gpu)
    rows = CF.adjoint_errors(seed, routine, mode, dpos.cpu().numpy(), dvel.cpu().numpy(), grads)
    assert CF.report(f"seed {seed} {routine} seeds={mode} kernel", rows) == []
    h = CF.host_back(c, routine, b["k"], seeds, mode)
    for g, key in zip(grads, ROUTINES[routine][3]):
        err = cases.rel_l2(g, h[key]) if h[key].any() else float(np.abs(g).max())
        print(f"seed {seed} {routine} seeds={mode} {key}: rel-L2 vs host {err:.3e}")
        if not err <= ATOMIC_TOL:
            pytest.fail(f"{key}: {err:.3e} from the host build (ATOMIC_TOL {ATOMIC_TOL}) with the float64 bound met; the host "
                        f"build's cancellation is {CF.cancellation(c, routine, b['k'], seeds, mode, key):.1f} to 1")


EDGE_SEEDS = [seed for seed in SEEDS if config(seed)["rres"] == 2][:2] + [seed for seed in SEEDS if config(seed)["rres"] == 200][:1]


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 65, 257])
@pytest.mark.parametrize("seed", EDGE_SEEDS)
def test_launch_edges(gpu, seed, n):
    """What the host build cannot see: the first 1, 63, 65 and 257 rays (a lone lane, a partial wave, a wave and a lane, a
    block and a lane) on 2 samples (a profile shorter than a wave in LDS) and on 200, through the three adjoints, against the
    host build as in test_kernels_match_host_build."""
    from adjointnonlinearraytracing_amd import drrt
    c, k = config(seed), CF.base(seed)["k"]
    assert c["rres"] in (2, 200) and len(EDGE_SEEDS) == 3
    T = drrt.TracerC()
    with drrt.using(check_failed=False):
        for routine in ROUTINES:
            b = CF.host_back(c, routine, k, c, sel=slice(0, n))
            _check_against_host(c, routine, b, *_dev_back(T, c, routine, k, c, "all", gpu, n=n))


CLASS_SEEDS = [next(seed for seed in SEEDS if config(seed)["rres"] == rres) for rres in (3, 127)]


@pytest.mark.gpu
@pytest.mark.parametrize("routine", list(ROUTINES))
@pytest.mark.parametrize("seed", CLASS_SEEDS)
def test_autograd_classes_end_to_end(gpu, seed, routine):
    """ADCableTracerC, CableOPLTracerC and CableFieldTracerC: apply -> linear loss with the module's seeds -> backward, on
    the first configuration with 3 samples and the first with 127: the integral and every .grad against the referee under
    the bound.  ADCableTracerC's profile gradient is the continuous adjoint's, which is no exact derivative
    (tests/test_gpu_fuzz.py referees it): its profile is frozen here."""
    from adjointnonlinearraytracing_amd import drrt, tracer
    c, b = config(seed), CF.base(seed)
    seeds = CF.seeds_of(c, routine, "all", b["compared"])
    cls = dict(rays=tracer.ADCableTracerC, opl=tracer.CableOPLTracerC, field=tracer.CableFieldTracerC)[routine]
    profs = [_t(c[key], gpu).requires_grad_(routine != "rays") for key in (("prof", "field") if routine == "field" else ("prof",))]
    x, v = (_t(c[key], gpu).requires_grad_(True) for key in ("pos", "vel"))
    with drrt.using(check_failed=False):
        out = cls.apply(*profs, c["radius"], c["length"], x, v, _t(c["tg"], gpu), c["ds"])
        outs = (out[0], out[1]) + tuple(out[3:])
        assert len(outs) == len(ROUTINES[routine][1])
        sum((o * _t(seeds[name], gpu)).sum() for o, name in zip(outs, ROUTINES[routine][1])).backward()
        torch.cuda.synchronize()
    rows = [] if routine == "rays" else CF.output_errors(seed, routine, outs[2].detach().cpu().numpy())
    grads = [p.grad.cpu().numpy() for p in profs] if routine != "rays" else []
    rows += CF.adjoint_errors(seed, routine, "all", x.grad.cpu().numpy(), v.grad.cpu().numpy(), grads)
    assert len(rows) == (routine != "rays") + 1 + len(ROUTINES[routine][3])
    assert CF.report(f"seed {seed} {routine} class", rows) == []
