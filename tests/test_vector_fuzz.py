"""Seeded fuzz of the line integral of a vector field on nasty grids: trace_vector / backtrace_vector on
cases.fuzz_config(seed), seed in range(16) -- the configurations of tests/test_integral_fuzz.py (non-cubic grids of 2..24
voxels per axis, 2-voxel axes on seeds 0, 4, 7, 14, h never a power of two, steps of 0.2..1.7 cells, rough media on
seed % 3 == 0, 600 rays inside, outside and exactly on faces, at rest and with |v| in 0.5..1.5) with a vector field
(tests/test_vector_integral.py::make_vfield) and a seed on circ drawn here.

Referee, yardstick, compared rays, error measure and bound are those of tests/test_vector_integral.py (float64 and float32
torch.autograd through tests/integral_ad; e_prod <= 8 max(e_ref, 2.4e-7), never above 1e-4 for circ -- relative to the ray's
float64 S -- or GRAD_TOL for rays and grids).

CPU tier (the host build: tests/integral_host): the forward is trace bit for bit, circ and the adjoint (with and without seeds
on the rays) under the bound, flag off, failed and never-entered rays.  GPU tier: the kernels against the host build on seeds
4 (2-voxel axis) and 12 (rough medium), with and without the pair copy, and VectorIntegralTracerC end to end on the same two.

Compared rays per seed 0..15 (of 600; at least 510 asked for) and those with S > 0 (at least 250 asked for):
  compared  547 562 585 533 572 570 582 593 592 564 565 556 564 557 576 532   (smallest: 532, seed 15)
  S > 0     322 333 346 299 327 301 338 336 331 303 305 337 305 335 290 304   (smallest: 290, seed 14)

Largest e_prod / max(e_ref, 2.4e-7) per quantity over the 16 seeds and both modes, host build (8 allowed):
  circ 1.59 (seed 0: 3.5e-6 against 2.2e-6)   rays 1.65 (3)   dL/drif 2.11 (6)   dL/dux 1.19   dL/duy 1.22   dL/duz 1.30 (all 9)"""
import numpy as np
import pytest
import torch

import cases
import hostcheck_lib as HC
import integral_common as IC
from integral_fuzz_common import SEEDS, TWO_VOXEL
import integral_fuzz_common as IF
from vector_common import MODES
import vector_common as VC

ATOMIC_TOL = VC.ATOMIC_TOL
_bits = IC._bits
_configs = {}


def config(seed):
    """integral_fuzz_common.config(seed) with a vector field and a seed on circ from a generator of this module's own."""
    if seed not in _configs:
        c = dict(IF.config(seed))
        rng = np.random.default_rng(seed + 7300)
        c["dcirc"] = rng.normal(size=len(c["pos"])).astype(np.float32)
        c["vfield"] = VC.make_vfield(c["rif"].shape, int(rng.integers(0, 1 << 20)))
        _configs[seed] = c
    return _configs[seed]


def key(seed):
    return ("integral_fuzz", seed)      # tests/integral_common.py::reference is shared with tests/test_integral_fuzz.py


# ---- CPU tier -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", SEEDS)
def test_forward_is_trace(seed):
    c = config(seed)
    k = VC.host_forward(c)
    t = HC.trace(c["rif"], c["res"], c["pos"], c["vel"], c["h"], c["ds"])
    assert np.array_equal(_bits(k["xt"]), _bits(t["xt"])) and np.array_equal(_bits(k["vt"]), _bits(t["vt"]))
    assert np.array_equal(k["steps"].astype(np.int64), t["steps"].astype(np.int64)) and k["n_failed"] == t["n_failed"] > 0


@pytest.mark.parametrize("seed", SEEDS)
def test_enough_rays_are_compared(oracle, seed):
    """A condition on the configurations, not a measurement: at least 510 of the 600 rays are compared and at least 250 of
    them have S > 0."""
    y = VC.yard(oracle, config(seed), key(seed))
    print(f"seed {seed}: {y['compared'].sum()} rays compared, {y['scaled'].sum()} with S > 0")
    assert (min(config(seed)["res"]) == 2) == (seed in TWO_VOXEL)
    assert y["compared"].sum() >= 510 and y["scaled"].sum() >= 250


@pytest.mark.parametrize("seed", SEEDS)
def test_circ_matches_float64(oracle, seed):
    y = VC.yard(oracle, config(seed), key(seed))
    assert np.abs(y["circ64"][y["scaled"]]).max() > 0.1
    assert IF.report(f"seed {seed}", VC.circ_rows(y, y["k"]["circ"])) == []


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("seed", SEEDS)
def test_adjoint_matches_float64_autograd(oracle, seed, mode):
    """Flag on: (dpos, dvel) per ray, dL/drif and the three planes of dL/du against float64 autograd, under the bound float32
    autograd sets, with all seeds and without seeds on the rays."""
    c = config(seed)
    r = VC.check_adjoint(oracle, c, key(seed), mode, f"seed {seed}")
    y = VC.yard(oracle, c, key(seed))
    assert r["n_failed"] == int(y["failed"].sum()) == y["k"]["n_failed"] > 0


@pytest.mark.parametrize("seed", SEEDS)
def test_flag_off_scales_the_gradient_splat(seed):
    """h is no power of two here: without DRRT_FLAG_CORRECTED_H dL/drif is the flag-on run's value part plus h times its
    gradient-splat part within 1e-6 rel-L2; dL/du and the ray gradients are bit-identical."""
    c = config(seed)
    k = VC.host_forward(c)
    run = lambda **kw: VC.host_back(c, k, c["dx"], c["dv"], c["dcirc"], **kw)      # noqa: E731
    off, on = run(corrected_h=False), run(corrected_h=True)
    val, spl = run(corrected_h=True, parts=1), run(corrected_h=True, parts=2)
    assert np.array_equal(val["grad"], run(corrected_h=False, parts=1)["grad"])
    assert cases.rel_l2(val["grad"] + spl["grad"], on["grad"]) <= 1e-6
    err = cases.rel_l2(val["grad"] + c["h"] * spl["grad"], off["grad"])
    print(f"seed {seed}: flag off vs value + h * splat: rel-L2 {err:.3e}")
    assert err <= 1e-6 and cases.rel_l2(off["grad"], on["grad"]) > 0.01
    assert np.array_equal(off["grad_vfield"], on["grad_vfield"]) and np.array_equal(val["grad_vfield"], on["grad_vfield"])
    assert not spl["grad_vfield"].any() and np.linalg.norm(on["grad_vfield"]) > 0.1
    assert np.array_equal(_bits(off["dpos"]), _bits(on["dpos"])) and np.array_equal(_bits(off["dvel"]), _bits(on["dvel"]))


@pytest.mark.parametrize("seed", SEEDS)
def test_failed_and_never_entered_rays(seed):
    """Rays at rest outside the box fail the forward: zeros, counted, no grid touched.  Rays outside that point away never
    enter: (dx, dv) and circ = +0 bit for bit, no grid touched."""
    c = config(seed)
    k = VC.host_forward(c)
    r = VC.host_back(c, k, c["dx"], c["dv"], c["dcirc"])
    failed = k["steps"] >= IC.max_steps_fwd(c["res"], c["h"], c["ds"])
    rest, away = IF._quiet_rays(c)
    assert rest.sum() >= 1 and away.sum() >= 40 and failed[rest].all() and not failed[away].any()
    assert r["n_failed"] == int(failed.sum()) == k["n_failed"] and np.array_equal(r["failed"], failed)
    assert not r["dpos"][failed].any() and not r["dvel"][failed].any()
    assert np.array_equal(_bits(r["dpos"][away]), _bits(c["dx"][away]))
    assert np.array_equal(_bits(r["dvel"][away]), _bits(c["dv"][away]))
    assert not _bits(k["circ"][away]).any()
    quiet = failed | away
    q = VC.host_back(c, k, c["dx"], c["dv"], c["dcirc"], sel=quiet)
    assert q["ray_steps"] == 0 and r["ray_steps"] > 0 and not r["steps"][quiet].any()
    assert not q["grad"].any() and not q["grad_vfield"].any()
    assert np.abs(r["grad"]).max() > 0 and (np.abs(r["grad_vfield"].reshape(3, -1)).max(1) > 0).all()


# ---- GPU tier -------------------------------------------------------------------------------------------------------
_hosts = {}


def host(seed):
    if seed not in _hosts:
        c = config(seed)
        k = VC.host_forward(c)
        _hosts[seed] = (k, VC.host_back(c, k, c["dx"], c["dv"], c["dcirc"], corrected_h=True))
    return _hosts[seed]


@pytest.mark.gpu
@pytest.mark.parametrize("pair", [False, True])
@pytest.mark.parametrize("seed", [4, 12])
def test_kernels_match_host_build(gpu, seed, pair):
    """k_trace_vector / k_backtrace_vector on a configuration with a 2-voxel axis (every cell a boundary cell: no held taps)
    and on one with a rough medium: rays and statistics bit for bit, the grids to the order of their atomic sums.  The
    forward sorts on seed 4 and the adjoint takes its order; on seed 12 both run in caller order."""
    from adjointnonlinearraytracing_amd import drrt
    assert seed in TWO_VOXEL or seed % 3 == 0
    c = config(seed)
    k, r = host(seed)
    T = drrt.TracerC()
    with drrt.using(pair_grid=pair, corrected_h=True, check_failed=False, sort_rays=seed == 4):
        fw = VC.gpu_forward(T, c, gpu)
        assert (fw[5] is not None) == (seed == 4)
        assert IC._same(fw[0], k["xt"]) and IC._same(fw[1], k["vt"]) and IC._same(fw[2], k["circ"])
        assert np.array_equal(fw[3].cpu().numpy().astype(np.int64), k["steps"].astype(np.int64))
        assert fw[4]["n_failed"] == k["n_failed"] > 0 and fw[4]["ray_steps"] == int(k["steps"].astype(np.int64).sum())
        (grad, gvf, dpos, dvel), bst = VC.gpu_back(T, c, gpu, fw, order=fw[5])
    assert IC._same(dpos, r["dpos"]) and IC._same(dvel, r["dvel"])
    assert bst["ray_steps"] == r["ray_steps"] > 0 and bst["n_failed"] == r["n_failed"] > 0
    assert VC.grids_close(grad, gvf, r)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [4, 12])
def test_autograd_class_end_to_end(gpu, oracle, seed):
    """VectorIntegralTracerC: apply -> loss on every output -> backward against float64 autograd under the bound of the CPU
    tier; the grids go in with the shape of the (non-cubic) resolution."""
    from adjointnonlinearraytracing_amd import drrt
    c = config(seed)
    y = VC.yard(oracle, c, key(seed))
    seeds = VC.seeds_of(c, "all", y["compared"])
    N = lambda t: t.cpu().numpy()      # noqa: E731
    with drrt.using(corrected_h=True, check_failed=False):
        grif, gvf, gx, gvel, out = VC.ad_grads(c, gpu, seeds, shaped=True)
    assert tuple(gvf.shape) == (3,) + tuple(c["res"]) and tuple(grif.shape) == tuple(c["res"])
    rows = VC.circ_rows(y, N(out[2])) + VC.adjoint_rows(oracle, c, key(seed), "all", N(gx), N(gvel), N(grif).reshape(-1),
                                                        N(gvf))
    assert len(rows) == 6 and IF.report(f"seed {seed} class", rows) == []
