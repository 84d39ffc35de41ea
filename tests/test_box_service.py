"""The window service of the box-window adjoint (k_backtrace_flat, csrc/drrt_adjoint_box.hip): the vote, the flush of the
z-planes that lanes have held slots in (win_flush walks the marked planes only), and the re-anchor.

What can go wrong there, and what is exercised here on a 24 x 28 x 32 grid (the 9^3 window slides on every axis, all strides
differ), in a smooth medium that bends the rays, with 64, 65 and 4096 rays (one full wave, one wave and one lane, 64 waves):

  * a plane that was written and not marked stays in LDS at a flush and is lost: bundles travelling along +x, -x, +y, -y,
    +z, -z and oblique to all axes change the marked planes from flush to flush and take the flush walk through every
    z-wrap; every writer of a slot is covered -- one-face leaves, two-face leaves (the oblique set), rays that end by
    leaving the box inside the window (every set), rays that end on the sdf surface (MODE 1), and rays cut off by the step
    budget of a depth chunk, whose hand-over in the epilogue is the only writer of its planes (a chunk of two steps);
  * a bundle wider than the window: lanes miss, the window stays put for its cool-down, their leaves go to the grid;
  * the CHUNK instantiation, whose resumed lanes meet the service before their first leave: K = 3 chunks with the
    boundaries swept over a whole anchor period, so that some fall right behind a flush.

The referee is the one-atomic-per-tap kernel (DRRT_FLAG_DIRECT_ATOMICS) and the factored fp32 oracle; the bound is the
project's rel-L2 bound on dL/dn, 2e-5, with equal step totals.  The sum of the gradient is compared as well: every voxel is
a sum of a few hundred fp32 adds at most, each rounding by at most 2^-24 of the absolute mass, so the two sums agree to
2e-5 of sum |g|, while one plane missed in one flush of a wave is a deficit of per cents.  Every case forces the box kernel
(DRRT_FLAG_STATIC_WINDOW), sorted and unsorted, with and without the pair copy."""
import zlib

import numpy as np
import pytest
import torch

from box_common import COUNTS, FLAG_SETS, HV, SETS, D, H, W, _check, _Gpu

pytestmark = pytest.mark.gpu


_reference = {}


def _rays_and_reference(name, n, dev, oracle, sdf=False):
    """One ray set, its oracle gradient and the one-atomic-per-tap kernel's: computed once per session, never changed."""
    key = (name, n, sdf)
    if key not in _reference:
        G = _Gpu.get(dev)
        rng = np.random.default_rng(zlib.crc32(f"{name}/{n}".encode()))
        pos, vel, ds = SETS[name](n, rng)
        mag = 10.0 ** rng.uniform(-1.0, 1.0, (n, 1))                      # seeds over two decades from ray to ray
        dx, dv = (rng.normal(size=(n, 3)) * mag).astype(np.float32), (rng.normal(size=(n, 3)) * mag).astype(np.float32)
        host = (pos, vel, dx, dv)
        rays = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in host)
        with oracle.arith("factored"):
            ob = oracle.backtrace(G.rif_np, (W, H, D), *host, HV, ds, dtype=np.float32, sdf=G.sdf_np if sdf else None)
        g_direct, st_direct = G.backtrace(rays, ds, G.L.FLAG_DIRECT_ATOMICS, sdf=sdf)
        for a in (ob["grad"], g_direct):
            a.setflags(write=False)
        _reference[key] = dict(rays=rays, ds=ds, g_oracle=np.asarray(ob["grad"], np.float64).reshape(-1), steps=int(ob["steps_total"]),
                               g_direct=g_direct, steps_direct=st_direct)
    return _reference[key]


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("name", ["x+", "x-", "y+", "y-", "z+", "z-", "oblique", "wide_x"])
def test_box_service_equals_direct_atomics_and_oracle(gpu, oracle, name, n):
    """every travel direction (one-face leaves, ends at the box face inside the window), the oblique set (two-face leaves)
    and the bundle wider than the window, under every flag set"""
    G = _Gpu.get(gpu)
    ref = _rays_and_reference(name, n, gpu, oracle)
    for fname, fl in FLAG_SETS:
        g, st = G.backtrace(ref["rays"], ref["ds"], fl | G.L.FLAG_STATIC_WINDOW)
        _check((name, n, fname), g, st, ref)


@pytest.mark.parametrize("n", COUNTS)
def test_box_service_backtrace_sdf(gpu, oracle, n):
    """MODE 1: the rays end on the sdf surface, in the middle of the volume and of the window, with accumulators to hand over"""
    G = _Gpu.get(gpu)
    ref, full = _rays_and_reference("y+", n, gpu, oracle, sdf=True), _rays_and_reference("y+", n, gpu, oracle)
    assert 0 < ref["steps"] < full["steps"]                    # the sdf did end the rays early
    for fname, fl in FLAG_SETS:
        g, st = G.backtrace(ref["rays"], ref["ds"], fl | G.L.FLAG_STATIC_WINDOW, sdf=True)
        _check(("sdf", n, fname), g, st, ref)


@pytest.mark.parametrize("n", COUNTS)
def test_box_service_step_budget_epilogue(gpu, oracle, n):
    """A first chunk of two steps: no ray has left its first cell when the budget runs out, so the hand-over in the epilogue is
    the only writer of the window and of its planes in that launch, and what the launch's flush skips is lost."""
    G = _Gpu.get(gpu)
    ref = _rays_and_reference("inside_z", n, gpu, oracle)
    for fname, fl in FLAG_SETS:
        g_one, st_one = G.backtrace(ref["rays"], ref["ds"], fl | G.L.FLAG_STATIC_WINDOW)
        g, st = G.chunked(ref["rays"], ref["ds"], fl | G.L.FLAG_STATIC_WINDOW, (2,))
        assert st == st_one
        _check(("budget", n, fname), g, st, ref, others=(g_one,))


@pytest.mark.parametrize("fname,fl", FLAG_SETS)
def test_box_service_chunk_boundaries(gpu, oracle, fname, fl):
    """K = 3 chunks against one launch.  With half-cell steps along y and seven cells of window a wave re-anchors every 14
    iterations or so: the first boundary is swept over 18 consecutive iterations (the second follows 23 later), so boundaries
    fall on, right behind and well after an iteration in which a flush was due, for every wave."""
    G = _Gpu.get(gpu)
    ref = _rays_and_reference("y-", 4096, gpu, oracle)
    g_one, st_one = G.backtrace(ref["rays"], ref["ds"], fl | G.L.FLAG_STATIC_WINDOW)
    _check(("one launch", fname), g_one, st_one, ref)
    for b in range(5, 23):
        g, st = G.chunked(ref["rays"], ref["ds"], fl | G.L.FLAG_STATIC_WINDOW, (b, b + 23))
        _check(("chunks", b, b + 23, fname), g, st, ref, others=(g_one,))
