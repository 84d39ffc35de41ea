"""The loop control and the leave of the box-window adjoint (k_backtrace_flat, csrc/drrt_adjoint_box.hip).

The kernel keeps "still marching" in the integer that holds the lane's window slot (a third sentinel, kEnded, below kMiss and
kIrregular): the loop exit, the miss vote and the lane body's mask are compares of that integer, and the cool-down is a scalar.
A ray's leave is two regions, one behind the other: the hot one (both cells regular, the flat index moved: six one-face
cases and one emission) and the cold one (into or out of a clamped cell, which can share its flat index with its regular
neighbour; jumps over more than one face: all eight corners), with the new cell's window slot computed once behind both.

What can go wrong there, and what is exercised here on the 24 x 28 x 32 grid of test_box_service.py (same medium, same
referees, same bounds) with 64, 65 and 4096 rays:

  * an ended lane that still votes, is re-anchored, or hands over twice (the epilogue tests the same integer): bundles whose
    rays end at different iterations inside one wave ("stagger"), and waves in which all but one lane end at once and the
    last marches on alone through re-anchors ("lone"); both also cut into depth chunks, so that ended lanes meet the
    epilogue hand-over and the saved flag word, which must still say active / outside;
  * a cold leave that is dropped or taken for a hot one: rays that start in, graze along and end in clamped cells beyond
    the -x and +x faces and in the regular cells on the faces ("graze": regular <-> clamped with and without a change of
    the flat index, steps that stay in a face cell whose taps are not held), and oblique bundles with steps of 0.9, 1.3 and
    1.7 cells, where jumps over two and three faces are common;
  * every one-face case under the one predicate: bundles along +-x, +-y, +-z, and a bundle wider than the window, which
    misses at every vote and lives on the cool-down;
  * backtrace_sdf (MODE 1) and K = 3 depth chunks with the boundaries swept over consecutive iterations.

Every case forces the box kernel (DRRT_FLAG_STATIC_WINDOW), sorted and unsorted, with and without the pair copy, and is
judged against the one-atomic-per-tap kernel and the factored oracle: rel-L2 <= 2e-5, equal step totals, and the sum of the
gradient within 2e-5 of sum |g| (see test_box_service.py for why that bound holds for a correct kernel)."""
import zlib

import numpy as np
import pytest
import torch

import box_common as svc

pytestmark = pytest.mark.gpu

W, H, D, HV, EXT = svc.W, svc.H, svc.D, svc.HV, svc.EXT
COUNTS = svc.COUNTS
FLAG_SETS = svc.FLAG_SETS


def _oblique(step_cells):
    def make(n, rng):
        pos, vel, _ = svc._oblique(n, rng)
        return pos, vel, step_cells * HV
    return make


def _oblique_rev(step_cells):
    """the oblique bundle mirrored through the centre of the volume: on the way back it runs from the sdf's inside to its
    outside, so backtrace_sdf ends it there"""
    def make(n, rng):
        pos, vel, _ = svc._oblique(n, rng)
        return (EXT - pos).astype(np.float32), -vel, step_cells * HV
    return make


def _stagger(n, rng):
    """a bundle that travelled along +y, its rays standing at depths spread over the whole volume: on the way back they
    leave through the y = 0 face at different iterations of one wave"""
    pos = np.array([0.47, 0.0, 0.52]) * EXT + rng.uniform(-1.0, 1.0, (n, 3)) * 1.5 * HV
    pos[:, 1] = rng.uniform(0.08, 0.95, n) * EXT[1]
    vel = rng.normal(0.0, 0.03, (n, 3))
    vel[:, 1] = 1.0
    return pos.astype(np.float32), vel.astype(np.float32), HV / 2


def _lone(n, rng):
    """as _stagger, but 63 rays of every 64 stand two or three cells from the y = 0 face and end within a few iterations of
    each other, and one stands at the far end: it marches on alone"""
    pos = np.array([0.47, 0.0, 0.52]) * EXT + rng.uniform(-1.0, 1.0, (n, 3)) * 1.5 * HV
    pos[:, 1] = rng.uniform(2.0, 3.0, n) * HV
    pos[::64, 1] = 0.93 * EXT[1]
    vel = rng.normal(0.0, 0.03, (n, 3))
    vel[:, 1] = 1.0
    return pos.astype(np.float32), vel.astype(np.float32), HV / 2


def _graze(n, rng):
    """rays along +-y in the clamped cells beyond the x faces and in the regular cells on them, in steps of 0.3 cells: half
    start outside the box and drift inwards on the way back (clamped -> face cell with the same flat index -> interior), half
    start inside and drift out through the x face (and end there, or beyond the y face); most steps stay in their cell"""
    low = rng.random(n) < 0.5                                   # at the -x face, else at the +x face
    inward = rng.random(n) < 0.5                                # the backward march drifts into the box
    off = np.where(inward, rng.uniform(-0.9, 0.4, n), rng.uniform(0.2, 2.5, n)) * HV      # distance inside the face
    x = np.where(low, off, EXT[0] - off)
    sgn = np.where(rng.random(n) < 0.5, 1.0, -1.0)              # travel along +y or -y
    y = np.where(sgn > 0, EXT[1] + 0.1 * HV, -0.1 * HV) * np.ones(n)
    z = (0.52 * EXT[2] + rng.uniform(-1.5, 1.5, n) * HV)
    drift = rng.uniform(0.04, 0.12, n) * np.where(inward, 1.0, -1.0) * np.where(low, -1.0, 1.0)   # backward = -vel
    vel = np.stack([drift, sgn, rng.normal(0.0, 0.02, n)], axis=1)
    return np.stack([x, y, z], axis=1).astype(np.float32), vel.astype(np.float32), 0.3 * HV


SETS = dict(svc.SETS)
del SETS["inside_z"]
SETS.update({"oblique0.9": _oblique(0.9), "oblique1.3": _oblique(1.3), "oblique1.7": _oblique(1.7), "oblique_rev1.3": _oblique_rev(1.3),
             "stagger": _stagger, "lone": _lone, "graze": _graze})

_reference = {}


def _rays_and_reference(name, n, dev, oracle, sdf=False):
    """One ray set, its oracle gradient and the one-atomic-per-tap kernel's: computed once per session, never changed."""
    key = (name, n, sdf)
    if key not in _reference:
        G = svc._Gpu.get(dev)
        rng = np.random.default_rng(zlib.crc32(f"control/{name}/{n}".encode()))
        pos, vel, ds = SETS[name](n, rng)
        mag = 10.0 ** rng.uniform(-1.0, 1.0, (n, 1))
        dx, dv = (rng.normal(size=(n, 3)) * mag).astype(np.float32), (rng.normal(size=(n, 3)) * mag).astype(np.float32)
        host = (pos, vel, dx, dv)
        rays = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in host)
        with oracle.arith("factored"):
            ob = oracle.backtrace(G.rif_np, (W, H, D), *host, HV, ds, dtype=np.float32, sdf=G.sdf_np if sdf else None)
        g_direct, st_direct = G.backtrace(rays, ds, G.L.FLAG_DIRECT_ATOMICS, sdf=sdf)
        for a in (ob["grad"], g_direct):
            a.setflags(write=False)
        _reference[key] = dict(rays=rays, ds=ds, g_oracle=np.asarray(ob["grad"], np.float64).reshape(-1),
                               steps=int(ob["steps_total"]), g_direct=g_direct, steps_direct=st_direct)
    return _reference[key]


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("name", sorted(SETS))
def test_box_control_equals_direct_atomics_and_oracle(gpu, oracle, name, n):
    """every set in one launch, under every flag set"""
    G = svc._Gpu.get(gpu)
    ref = _rays_and_reference(name, n, gpu, oracle)
    for fname, fl in FLAG_SETS:
        g, st = G.backtrace(ref["rays"], ref["ds"], fl | G.L.FLAG_STATIC_WINDOW)
        svc._check((name, n, fname), g, st, ref)


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("name", ["y+", "oblique_rev1.3", "stagger"])
def test_box_control_backtrace_sdf(gpu, oracle, name, n):
    """MODE 1: rays end on the sdf surface in the middle of the window, at different iterations; the others march on"""
    G = svc._Gpu.get(gpu)
    ref, full = _rays_and_reference(name, n, gpu, oracle, sdf=True), _rays_and_reference(name, n, gpu, oracle)
    assert 0 < ref["steps"] < full["steps"]                    # the sdf did end rays early
    for fname, fl in FLAG_SETS:
        g, st = G.backtrace(ref["rays"], ref["ds"], fl | G.L.FLAG_STATIC_WINDOW, sdf=True)
        svc._check(("sdf", name, n, fname), g, st, ref)


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("name", ["stagger", "lone", "graze", "oblique1.7"])
def test_box_control_chunked_with_ended_lanes(gpu, oracle, name, n):
    """K = 3 depth chunks whose budgets run out while some lanes of a wave have ended and others march: the epilogue hands
    over the marching lanes' cells only, and the saved flag word restarts exactly those"""
    G = svc._Gpu.get(gpu)
    ref = _rays_and_reference(name, n, gpu, oracle)
    for fname, fl in FLAG_SETS:
        for bounds in ((3, 9), (7, 20)):
            g, st = G.chunked(ref["rays"], ref["ds"], fl | G.L.FLAG_STATIC_WINDOW, bounds)
            svc._check(("chunks", name, n, bounds, fname), g, st, ref)


@pytest.mark.parametrize("fname,fl", FLAG_SETS)
def test_box_control_chunk_boundaries(gpu, oracle, fname, fl):
    """K = 3 chunks against one launch, the first boundary swept over 12 consecutive iterations of the staggered bundle (its
    rays end from iteration 4 on, and its waves re-anchor every few iterations: it is wider than the window along y)"""
    G = svc._Gpu.get(gpu)
    ref = _rays_and_reference("stagger", 4096, gpu, oracle)
    g_one, st_one = G.backtrace(ref["rays"], ref["ds"], fl | G.L.FLAG_STATIC_WINDOW)
    svc._check(("one launch", fname), g_one, st_one, ref)
    for b in range(2, 14):
        g, st = G.chunked(ref["rays"], ref["ds"], fl | G.L.FLAG_STATIC_WINDOW, (b, b + 11))
        svc._check(("chunks", b, b + 11, fname), g, st, ref, others=(g_one,))
