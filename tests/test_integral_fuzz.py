"""Seeded fuzz of the integral operators and the ray adjoints on nasty grids: backtrace_rays, trace_opl / backtrace_opl,
trace_field / backtrace_field, trace_emission / backtrace_emission on cases.fuzz_config(seed), seed in range(16) -- non-cubic
grids of 2..24 voxels per axis (2-voxel axes on seeds 0, 4, 7, 14: every cell is a boundary cell), h in 0.05..2 and never a
power of two, steps of 0.2..1.7 cells, rough random media on seed % 3 == 0, 600 rays inside, outside and exactly on faces, at
rest and with |v| in 0.5..1.5 -- where the fixed scenes of tests/raygrad_common.py have cubic or one 7x11x5 grid, h in {1, 0.5}
and unit-speed rays.  What a configuration needs beyond fuzz_config (seeds on opl, tau and rad, the second field, emission and
absorption) is drawn in tests/integral_fuzz_common.py.

Referee: float64 torch.autograd through oracle/torch_ad.trace, tests/integral_ad.  Yardstick: the
same restatement run in float32.  A ray is compared when it is tie-free for the product (fp32 host build and fp64 oracle leave
on the same iteration, exit samples within TIE_TOL: tests/integral_common.py::reference) and for the yardstick (the same between the
float32 and the float64 torch runs); the seeds of every other ray are zero on all sides.  For every output (largest relative
error over the compared rays with a non-zero integral), for (dpos, dvel) (largest raygrad_common.rel_err over the compared
rays) and for every grid gradient (rel-L2, flag on), with e_prod = product against float64 and e_ref = float32 run against
float64, the bound is
    e_prod <= 8 max(e_ref, 2.4e-7),   and never above 1e-4 (outputs) or GRAD_TOL = 1e-3 (rays, grids):
2.4e-7 = 2^-22 is a few fp32 roundings, 8 the room for another, equally valid order of the fp32 operations.  The bound moves
with the conditioning of the configuration (rough media, long marches) and never with what the code under test gives.

CPU tier (the host build of the per-ray routines: hostcheck_lib, integral_host): forward identities bit
for bit, outputs and adjoints under the bound, flag off, failed and never-entered rays.  GPU tier: the kernels against the
host build with and without the pair copy (the forward sorts on even seeds and the adjoint takes its order; on odd seeds the
forward runs in caller order and the adjoint sorts for itself), TracerC.trace with the same pair setting, and the three
autograd classes end to end on seeds 4 (2-voxel axis) and 12 (rough medium) under the bound.

Compared rays per seed 0..15 (of 600; at least 510 asked for), those with a non-zero integral (at least 250 asked for), and
the largest float64 tau among them (>= 1 asked for everywhere, >= 3 on at least 8 seeds: the 11 of THICK):
  compared  547 562 585 533 572 570 582 593 592 564 565 556 564 557 576 532   (smallest: 532, seed 15)
  non-zero  322 333 346 299 327 301 338 336 331 303 305 337 305 335 290 304   (smallest: 290, seed 14)
  max tau   5.50 4.93 3.79 1.69 5.50 5.50 1.30 5.50 3.27 2.57 5.02 5.50 1.85 4.13 5.50 1.29

Largest e_prod / max(e_ref, 2.4e-7) per quantity over the 16 seeds and all modes, host build (8 allowed):
  backtrace_rays   rays 1.40 (seed 12: 2.5e-4 against 1.8e-4, the largest e_prod of all)
  opl              opl 1.44 (11)   rays 3.56 (3: 4.1e-5 against 1.2e-5)   dL/drif 2.46 (6)
  field            tau 1.29 (4)    rays 2.67 (6: 2.9e-4 against 1.1e-4)   dL/drif 2.41 (6)   dL/dfield 1.32 (9)
  emission         rad 1.25 (6)    tau 1.32 (8)   rays 3.12 (3, drad alone)   dL/drif 2.20 (6)   dL/de 1.30 (9)
                   dL/da 2.45 (9, drad alone)
trace_field and backtrace_rays, not measured before, behave like the other two: no ratio above 3.6, and e_ref tracks every
large e_prod (seeds 6 and 12: conditioning, not a defect).  The GPU tier's classes give the host build's figures: their ray
results are the host build's bit for bit and their grids differ from it by the order of the atomic sums.

Mutation checks (tried by hand on the host build, one at a time, each then undone; CPU tier):
  * tests/hostcheck/integral_rays.hip, the value weights of dL/dfield: in every boundary cell (Cell::interior false) the +z
    neighbour replaced by the cell itself (oz = 0): all 32 field cases of test_adjoint_matches_float64_autograd fail; of the
    fixed scenes, all ten cases of tests/test_field_integral.py::test_adjoint_matches_float64_autograd, its
    test_plane_source_on_host, test_consistent_with_opl (5) and tests/test_emission.py::test_consistent_with_field_integral
    (5) fail too: their rays cross boundary cells as well.
  * the same on a 2-voxel axis only (oz = 0 where D == 2, oy = 0 where H == 2): the 8 field cases of
    test_adjoint_matches_float64_autograd on seeds 0, 4, 7, 14 fail; no fixed-scene test fails.
  * tests/hostcheck/integral_rays.hip, grad_scale of the corrected_h path h instead of 1 / h: all 32 opl cases of
    test_adjoint_matches_float64_autograd and all 16 opl cases of test_flag_off_scales_the_gradient_splat fail; of the fixed
    scenes, the four h = 0.5 cases of tests/test_opl.py::test_adjoint_matches_float64_autograd and its
    test_flag_off_scales_the_gradient_splat fail, the six h = 1 cases pass (h = 1 / h).
  * csrc/drrt_device.h, opl_backtrace_ray: the free-flight prefix also skips a sample that lies exactly on a near face (p == 0
    on an axis), so the first sample of a ray that starts on a face is not accumulated: all 32 opl cases of
    test_adjoint_matches_float64_autograd fail; of the fixed scenes, all ten cases of
    tests/test_opl.py::test_adjoint_matches_float64_autograd and test_uniform_medium_closed_form fail."""
import numpy as np
import pytest
import torch

import cases
from integral_fuzz_common import MODES, ROUTINES, SEEDS, TWO_VOXEL, _quiet_rays, config
import integral_fuzz_common as IF
import integral_host as OH
from raygrad_common import _t

ATOMIC_TOL = 2e-5       # grid gradients, kernel vs host build: only the order of the atomic sums differs
THICK = (0, 1, 2, 4, 5, 7, 8, 10, 11, 13, 14)      # seeds whose largest tau over the compared rays is at least 3
assert len(THICK) >= 8
INTEGRALS = ("opl", "field", "emission")
ADJOINTS = [(seed, routine, mode) for seed in SEEDS for routine in ROUTINES for mode in MODES[routine]]
_bits = lambda a: np.ascontiguousarray(a).view(np.uint32)      # noqa: E731


def _is_pow2(h):
    return float(np.log2(h)).is_integer()


# ---- CPU tier -------------------------------------------------------------------------------------------------------
def test_configurations():
    """What the fuzz is there for: 2-voxel axes on seeds 0, 4, 7, 14; no h is a power of two; rays at rest, off unit speed
    and exactly on faces in every configuration."""
    for seed in SEEDS:
        c = cases.fuzz_config(seed)
        assert (min(c["res"]) == 2) == (seed in TWO_VOXEL) and not _is_pow2(c["h"]) and not _is_pow2(c["ds"])
        speed = np.linalg.norm(c["vel"], axis=1)
        assert (speed == 0).sum() >= 3 and (np.abs(speed - 1) > 0.2).sum() >= 200
        ext = (np.array(c["res"]) - 1) * c["h"]
        assert ((c["pos"] == 0) | (c["pos"] == ext.astype(np.float32))).any(1).sum() >= 100


@pytest.mark.parametrize("seed", SEEDS)
def test_forward_identities(seed):
    """(xt, vt, steps, n_failed) of trace_opl_ray, trace_field_ray and trace_emission_ray == hostcheck_lib.trace; the
    emission's tau == trace_field_ray's of the field a; with a = 0, rad == trace_field_ray's tau of the field e: bit for bit."""
    c = config(seed)
    t = IF.host_forward(c, "rays")
    fwd = {routine: IF.host_forward(c, routine) for routine in INTEGRALS}
    for routine, k in fwd.items():
        assert np.array_equal(_bits(k["xt"]), _bits(t["xt"])) and np.array_equal(_bits(k["vt"]), _bits(t["vt"])), routine
        assert np.array_equal(k["steps"].astype(np.int64), t["steps"].astype(np.int64)), routine
        assert k["n_failed"] == t["n_failed"] > 0, routine
    fa = OH.trace_field(c["rif"], c["absorption"], c["res"], c["pos"], c["vel"], c["h"], c["ds"])
    assert np.array_equal(_bits(fwd["emission"]["tau"]), _bits(fa["tau"])) and fa["tau"].max() > 1.0
    k0 = IF.host_forward(dict(c, absorption=np.zeros_like(c["absorption"])), "emission")
    fe = OH.trace_field(c["rif"], c["emission"], c["res"], c["pos"], c["vel"], c["h"], c["ds"])
    assert np.array_equal(_bits(k0["rad"]), _bits(fe["tau"])) and fe["tau"].max() > 1.0 and not k0["tau"].any()
    assert not np.array_equal(fwd["emission"]["rad"], k0["rad"]) and (fwd["emission"]["rad"] <= k0["rad"]).all()


@pytest.mark.parametrize("seed", SEEDS)
def test_enough_rays_are_compared(oracle, seed):
    """A condition on the configurations, not a measurement: at least 85 % of the 600 rays are compared, at least 250 of
    them have a non-zero integral, and the largest tau among them is >= 1 everywhere and >= 3 on the seeds of THICK."""
    m = IF.masks(oracle, seed)
    tau = m["tau64"][m["compared"]].max()
    print(f"seed {seed}: {m['compared'].sum()} rays compared, {m['nonzero'].sum()} with a non-zero integral, max tau {tau:.2f}")
    assert m["compared"].sum() >= 0.85 * 600 and m["nonzero"].sum() >= 250
    assert tau >= (3.0 if seed in THICK else 1.0)


@pytest.mark.parametrize("routine", INTEGRALS)
@pytest.mark.parametrize("seed", SEEDS)
def test_outputs_match_float64(oracle, seed, routine):
    """opl / tau / rad of the host build against the float64 run, under the bound the float32 run sets."""
    k = IF.host_forward(config(seed), routine)
    assert IF.report(f"seed {seed} {routine}", IF.output_errors(oracle, seed, routine, k)) == []


@pytest.mark.parametrize("seed,routine,mode", ADJOINTS)
def test_adjoint_matches_float64_autograd(oracle, seed, routine, mode):
    """Flag on: (dpos, dvel) per ray and every grid gradient against float64 autograd, under the bound float32 autograd sets;
    with all seeds, without ray seeds and, for the emission, with drad alone and dtau alone (backtrace_rays: (dpos, dvel)
    with its two seeds).  The signal is real: every gradient a seed reaches has |grad| > 0.1."""
    c, m = config(seed), IF.masks(oracle, seed)
    k = IF.host_forward(c, routine)
    kw = {} if routine == "rays" else dict(corrected_h=True)
    r = IF.host_back(c, routine, k, IF.seeds_of(c, routine, mode, m["compared"]), mode, **kw)
    rows = IF.adjoint_errors(oracle, seed, routine, mode, r["dpos"], r["dvel"], [r[g] for g in ROUTINES[routine][2]])
    bad = IF.report(f"seed {seed} {routine} seeds={mode}", rows)
    for (label, _, _, _, norm), key in zip(rows[1:], ROUTINES[routine][2]):
        if label == "dL/de" and mode == "dtau":                              # tau does not depend on e
            assert norm == 0 and not r[key].any()
        else:
            assert norm > 0.1, label
    assert rows[0][4] > 1e-3 and bad == []
    assert r["n_failed"] == int(m["failed"].sum()) == k["n_failed"] > 0


@pytest.mark.parametrize("routine", INTEGRALS)
@pytest.mark.parametrize("seed", SEEDS)
def test_flag_off_scales_the_gradient_splat(seed, routine):
    """h is no power of two here, so 1 / h and h are rounded: without DRRT_FLAG_CORRECTED_H dL/drif is the flag-on run's
    value part plus h times its gradient-splat part within 1e-6 rel-L2 (the bound of tests/test_opl.py's flag test: a few
    roundings of 2^-24 per corner); the grids without a gradient splat and the ray gradients are bit-identical."""
    c = config(seed)
    assert not _is_pow2(c["h"])
    k = IF.host_forward(c, routine)
    run = lambda **kw: IF.host_back(c, routine, k, c, **kw)      # noqa: E731
    off, on = run(corrected_h=False), run(corrected_h=True)
    val, spl = run(corrected_h=True, parts=1), run(corrected_h=True, parts=2)
    assert np.array_equal(val["grad"], run(corrected_h=False, parts=1)["grad"])
    assert cases.rel_l2(val["grad"] + spl["grad"], on["grad"]) <= 1e-6
    err = cases.rel_l2(val["grad"] + c["h"] * spl["grad"], off["grad"])
    print(f"seed {seed} {routine}: flag off vs value + h * splat: rel-L2 {err:.3e}; |value| {np.linalg.norm(val['grad']):.3e} "
          f"|splat| {np.linalg.norm(spl['grad']):.3e}")
    assert err <= 1e-6
    assert cases.rel_l2(off["grad"], on["grad"]) > 0.01 and np.linalg.norm(val["grad"]) > 0 and np.linalg.norm(spl["grad"]) > 0
    for g in ROUTINES[routine][2][1:]:                                      # value weights only
        assert np.array_equal(off[g], on[g]) and np.array_equal(val[g], on[g]) and not spl[g].any()
        assert np.linalg.norm(on[g]) > 0.1
    assert np.array_equal(_bits(off["dpos"]), _bits(on["dpos"])) and np.array_equal(_bits(off["dvel"]), _bits(on["dvel"]))


@pytest.mark.parametrize("routine", list(ROUTINES))
@pytest.mark.parametrize("seed", SEEDS)
def test_failed_and_never_entered_rays(seed, routine):
    """Rays at rest outside the box fail the forward: zeros, counted, no grid touched.  Rays outside that point away never
    enter: (dx, dv) bit for bit, no grid touched."""
    c = config(seed)
    k = IF.host_forward(c, routine)
    kw = {} if routine == "rays" else dict(corrected_h=True)
    r = IF.host_back(c, routine, k, c, **kw)
    failed = k["steps"] >= IF.IC.max_steps_fwd(c["res"], c["h"], c["ds"])
    rest, away = _quiet_rays(c)
    assert rest.sum() >= 1 and away.sum() >= 40 and failed[rest].all() and not failed[away].any()
    assert r["n_failed"] == int(failed.sum()) == k["n_failed"]
    assert not r["dpos"][failed].any() and not r["dvel"][failed].any()
    assert np.array_equal(_bits(r["dpos"][away]), _bits(c["dx"][away]))
    assert np.array_equal(_bits(r["dvel"][away]), _bits(c["dv"][away]))
    quiet = failed | away
    q = IF.host_back(c, routine, k, c, sel=quiet, **kw)
    assert q["ray_steps"] == 0 and r["ray_steps"] > 0 and q["n_failed"] == r["n_failed"]
    if routine != "rays":
        assert np.array_equal(r["failed"], failed) and not r["steps"][quiet].any()
        assert r["ray_steps"] == int(r["steps"].astype(np.int64).sum())
    for g in ROUTINES[routine][2]:
        assert not q[g].any() and np.abs(r[g]).max() > 0, g


# ---- GPU tier -------------------------------------------------------------------------------------------------------
def _same(got, want):
    got = got.cpu().numpy()
    return np.array_equal(np.isfinite(got), np.isfinite(want)) and np.array_equal(got, want, equal_nan=True)


def _gpu_pair(T, c, routine, dev, fwd_sorts):
    """The routine's forward and adjoint kernels on the configuration, every seed set on every ray.  The forward sorts or
    runs in caller order; the adjoint takes the forward's order, or (after a forward in caller order) sorts for itself.
    -> (outputs {name: tensor}, steps, forward stats, grid gradients, dpos, dvel, adjoint stats)"""
    from adjointnonlinearraytracing_amd import drrt
    grids = [_t(c[key], dev).reshape(-1) for key in ROUTINES[routine][0]]
    pos, vel = _t(c["pos"], dev), _t(c["vel"], dev)
    seeds = [_t(c[key], dev) for key in ROUTINES[routine][1]]
    args = (c["res"], pos, vel)
    with drrt.using(sort_rays=fwd_sorts):
        if routine == "rays":
            xt, vt = T.trace(*grids, *args, c["h"], c["ds"])
            more, steps = (), drrt.keep_steps(drrt.last_steps)
        else:
            fn = dict(opl=T.trace_opl, field=T.trace_field, emission=T.trace_emission)[routine]
            xt, vt, *more, steps = fn(*grids, *args, c["h"], c["ds"])
        st = drrt.read_stats()
        order = drrt.keep_order(drrt.last_order)
    assert (order is not None) == fwd_sorts
    with drrt.using(sort_rays=True):
        if routine == "rays":
            out = T.backtrace_rays(*grids, *args, xt, vt, steps, *seeds, c["h"], c["ds"], order=order)
        elif routine == "emission":
            out = T.backtrace_emission(*grids, *args, xt, vt, steps, more[1], *seeds, c["h"], c["ds"], order=order)
        else:
            fn = dict(opl=T.backtrace_opl, field=T.backtrace_field)[routine]
            out = fn(*grids, *args, xt, vt, steps, *seeds, c["h"], c["ds"], order=order)
        bst = drrt.read_stats()
    outs = dict(zip(("xt", "vt") + IF.OUTPUTS[routine], (xt, vt) + tuple(more)))
    return outs, steps, st, out[:-2], out[-2], out[-1], bst


@pytest.mark.gpu
@pytest.mark.parametrize("pair", [False, True])
@pytest.mark.parametrize("seed", SEEDS)
def test_kernels_match_host_build(gpu, seed, pair):
    """k_backtrace_rays and the kernels of drrt_integral.hip, with plain and pair-copy
    gathers of rif == the host build: outputs, steps, ray gradients and statistics bit for bit, every grid gradient to the
    order of its atomic sums.  And TracerC.trace with the same pair setting gives the same (xt, vt, steps): the seeds with
    a 2-voxel axis never ran the pair copy before."""
    from adjointnonlinearraytracing_amd import drrt
    c = config(seed)
    T = drrt.TracerC()
    fwd_sorts = seed % 2 == 0
    with drrt.using(pair_grid=pair, corrected_h=True, check_failed=False):
        for routine in ROUTINES:
            k, r = IF.host(seed, routine)
            outs, steps, st, grids, dpos, dvel, bst = _gpu_pair(T, c, routine, gpu, fwd_sorts)
            for name, got in outs.items():
                assert _same(got, k[name]), (routine, name)
            assert np.array_equal(steps.cpu().numpy().astype(np.int64), k["steps"].astype(np.int64)), routine
            assert st["n_failed"] == k["n_failed"] > 0 and st["ray_steps"] == int(k["steps"].astype(np.int64).sum()), routine
            assert _same(dpos, r["dpos"]) and _same(dvel, r["dvel"]), routine
            assert bst["ray_steps"] == r["ray_steps"] > 0 and bst["n_failed"] == r["n_failed"] > 0, routine
            assert len(grids) == len(ROUTINES[routine][2])
            for g, key, label in zip(grids, *ROUTINES[routine][2:]):
                err = cases.rel_l2(g.cpu().numpy(), r[key])
                print(f"seed {seed} pair={pair} {routine} {label}: rel-L2 vs host {err:.3e}")
                assert err <= ATOMIC_TOL, (routine, label)


def _class_grads(c, routine, dev, seeds):
    """The routine's autograd class on the configuration -> L = sum <seed, output> -> backward -> (outputs {name: array}, grid
    gradients, dpos, dvel).  The classes take rif.shape for the resolution (W, H, D), so the grids go in with that shape: the
    flat order is the library's either way."""
    from adjointnonlinearraytracing_amd import tracer
    cls = dict(opl=tracer.OPLTracerC, field=tracer.FieldIntegralTracerC, emission=tracer.EmissionTracerC)[routine]
    grids = [_t(c[key], dev).reshape(*c["res"]).requires_grad_(True) for key in ROUTINES[routine][0]]
    x, v = (_t(c[key], dev).requires_grad_(True) for key in ("pos", "vel"))
    out = cls.apply(*grids, x, v, c["h"], c["ds"])
    loss = sum((o * _t(seeds[name], dev)).sum() for o, name in zip(out, ROUTINES[routine][1]))
    loss.backward()
    torch.cuda.synchronize()
    outs = {name: o.detach().cpu().numpy() for name, o in zip(IF.OUTPUTS[routine], out[2:])}
    return outs, [g.grad.cpu().numpy().reshape(-1) for g in grids], x.grad.cpu().numpy(), v.grad.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("routine", INTEGRALS)
@pytest.mark.parametrize("seed", [4, 12])
def test_autograd_classes_end_to_end(gpu, oracle, seed, routine):
    """OPLTracerC, FieldIntegralTracerC and EmissionTracerC: apply -> loss on every output -> backward, on a configuration
    with a 2-voxel axis and on one with a rough medium, against float64 autograd under the bound of the CPU tier."""
    from adjointnonlinearraytracing_amd import drrt
    assert seed in TWO_VOXEL or seed % 3 == 0
    c, m = config(seed), IF.masks(oracle, seed)
    seeds = IF.seeds_of(c, routine, "all", m["compared"])
    with drrt.using(corrected_h=True, check_failed=False):
        outs, grids, dpos, dvel = _class_grads(c, routine, gpu, seeds)
    rows = IF.output_errors(oracle, seed, routine, outs) + IF.adjoint_errors(oracle, seed, routine, "all", dpos, dvel, grids)
    assert len(rows) == len(IF.OUTPUTS[routine]) + 1 + len(ROUTINES[routine][2])
    assert IF.report(f"seed {seed} {routine} class", rows) == []
