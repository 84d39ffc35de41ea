"""CPU tier of the locality sort (csrc/drrt_keys.h, csrc/drrt_sort.hip): which rays share a wave is invisible to every
parity test, because results are written back in the caller's order.  Here the host build of the key functions
(tests/hostcheck) is compared with the referee oracle/sortkey_ref.py:

* the Hilbert index on all 2^22 cells: a bijection, equal to the reference, unit steps, aligned tiles contiguous;
* the 961 direction-cell frames: bit-equal to the fp32 restatement, orthonormal and right-handed in float64;
* the direction cells of the axes (cell centres) and of -z (a corner of the octahedral map);
* both keys on the fuzz rays, for the forward (+1) and the adjoint (-1) heading: bit-equal to the fp32 restatement, equal
  to the float64 referee wherever that is decided;
* the aligned plane source keeps perfect 8 x 8 tiles; resting rays, non-finite values, the zero-extent volume;
* the key functions under AddressSanitizer + UndefinedBehaviorSanitizer, as a stand-alone program.
The device's order is compared with the same host build and the same referee in tests/test_sort_order.py."""
import functools
import glob
import os
import subprocess

import numpy as np
import pytest

import cases
import hostcheck_lib as H
from oracle import sortkey_ref as S
from ray16_common import SEEDS

SIGNS = (1.0, -1.0)
CELL_SHIFT = 2 * S.POS_BITS
N_CELLS = S.DIR_CELLS * S.DIR_CELLS


def cell_of(keys):
    """(a, b) of light-field keys"""
    cell = np.asarray(keys).astype(np.int64) >> CELL_SHIFT
    return cell // S.DIR_CELLS - S.DIR_HALF, cell % S.DIR_CELLS - S.DIR_HALF


def offsets_of(keys):
    """(qu, qv) of light-field keys, by the reference's inverse Hilbert walk"""
    return S.d2xy(np.asarray(keys).astype(np.int64) & ((1 << CELL_SHIFT) - 1))


# ---- a. the Hilbert index ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def hilbert_grid():
    """x, y of all 2^22 cells (x major), the host build's index and the reference's; callers must not modify them."""
    g = np.arange(S.POS_CELLS, dtype=np.int64)
    x, y = (a.ravel() for a in np.meshgrid(g, g, indexing="ij"))
    return x, y, H.hilbert2(x, y).astype(np.int64), S.xy2d(x, y)


def test_hilbert_reference_round_trips():
    """The reference pair itself: d2xy(xy2d(x, y)) = (x, y) on all cells, xy2d(d2xy(d)) = d on all indices, and the 16 cells
    of the order-2 curve as drawn in the textbooks."""
    x, y, _, ref = hilbert_grid()
    bx, by = S.d2xy(ref)
    assert np.array_equal(bx, x) and np.array_equal(by, y)
    d = np.arange(1 << 16, dtype=np.int64)                          # the other way round on a smaller curve (a bijection either way)
    assert np.array_equal(S.xy2d(*S.d2xy(d, bits=8), bits=8), d)
    want = [(0, 0), (1, 0), (1, 1), (0, 1), (0, 2), (0, 3), (1, 3), (1, 2), (2, 2), (2, 3), (3, 3), (3, 2), (3, 1), (2, 1),
            (2, 0), (3, 0)]
    assert list(zip(*(v.tolist() for v in S.d2xy(np.arange(16), bits=2)))) == want
    assert S.xy2d(*np.array(want).T, bits=2).tolist() == list(range(16))


def test_hilbert2_is_the_hilbert_curve():
    """The host build of hilbert2 on all 2^22 cells: a bijection onto [0, 2^22), equal to the reference, consecutive
    indices one unit step apart in x or y, every aligned 2^k x 2^k tile (k = 1 .. 10) an aligned contiguous index range."""
    x, y, d, ref = hilbert_grid()
    n = 1 << CELL_SHIFT
    assert d.min() == 0 and d.max() == n - 1 and np.array_equal(np.bincount(d, minlength=n), np.ones(n, np.int64))
    bad = np.nonzero(d != ref)[0]
    assert bad.size == 0, (x[bad[:5]], y[bad[:5]], d[bad[:5]], ref[bad[:5]])
    along = np.empty(n, np.int64)
    along[d] = np.arange(n)
    sx, sy = np.abs(np.diff(x[along])), np.abs(np.diff(y[along]))
    assert np.array_equal(sx + sy, np.ones(n - 1, np.int64)), "consecutive indices must be neighbouring cells"
    grid = d.reshape(S.POS_CELLS, S.POS_CELLS)
    for k in range(1, S.POS_BITS):
        t, m = 1 << k, S.POS_CELLS >> k
        hi = (grid >> (2 * k)).reshape(m, t, m, t)
        # all 4^k cells of a tile share the index bits above 2k, so (a bijection) the tile IS the range [j 4^k, (j + 1) 4^k)
        assert np.array_equal(hi.min(axis=(1, 3)), hi.max(axis=(1, 3))), k


# ---- b. the frames -----------------------------------------------------------------------------------------------------
def test_frames_of_all_961_cells():
    """Host build bit-equal to the fp32 restatement; in float64 |c| = |t1| = |t2| = 1 and t2 = c x t1 to 1e-6 (a handful of
    fp32 roundings of unit-size numbers, 6e-8 each), the three dot products within 1e-6."""
    a, b = (v.ravel() for v in np.meshgrid(np.arange(-S.DIR_HALF, S.DIR_HALF + 1), np.arange(-S.DIR_HALF, S.DIR_HALF + 1),
                                           indexing="ij"))
    got = H.lf_cell_frame(a, b)
    want = tuple(v.reshape(-1, 3) for v in S.frames32())
    for g, w, name in zip(got, want, ("c", "t1", "t2")):
        assert g.dtype == w.dtype == np.float32
        bad = np.nonzero((g.view(np.uint32) != w.view(np.uint32)).any(axis=1))[0]
        assert bad.size == 0, (name, a[bad[:5]], b[bad[:5]], g[bad[:5]], w[bad[:5]])
    c, t1, t2 = (g.astype(np.float64) for g in got)
    for v in (c, t1, t2):
        assert np.abs(np.linalg.norm(v, axis=1) - 1.0).max() <= 1e-6
    for p, q in ((t1, t2), (t1, c), (t2, c)):
        assert np.abs((p * q).sum(1)).max() <= 1e-6
    assert np.abs(t2 - np.cross(c, t1)).max() <= 1e-6
    # the centre really is the centre of its cell: the octahedral map sends it back to (a, b).  Not asked of the outermost
    # ring |a| = 15 or |b| = 15: those are half cells on the edge of the octahedral square, where the map folds onto itself --
    # (15, b) and (15, -b) have the same centre direction, and all four corners have (0, 0, -1)
    inner = (np.abs(a) < S.DIR_HALF) & (np.abs(b) < S.DIR_HALF)
    ox, oy = S._octa(c, 1.0)
    assert np.abs(S.DIR_HALF * ox - a)[inner].max() < 1e-5 and np.abs(S.DIR_HALF * oy - b)[inner].max() < 1e-5
    corners = (np.abs(a) == S.DIR_HALF) & (np.abs(b) == S.DIR_HALF)
    assert np.array_equal(c[corners], np.tile([[0.0, 0.0, -1.0]], (4, 1)))


# ---- c. direction cells ------------------------------------------------------------------------------------------------
RES_C, H_C = (5, 4, 3), 0.37


def _cells(vel):
    vel = np.asarray(vel, np.float32)
    pos = np.tile(np.array([[0.4, 0.3, 0.2]], np.float32), (len(vel), 1))
    keys = H.lightfield_keys(RES_C, H_C, pos, vel)
    assert np.array_equal(keys, S.lightfield32(RES_C, H_C, pos, vel)["key"])
    return np.stack(cell_of(keys), -1)


def _disc(radius, n=4000, seed=5):
    """perturbations (n,2): random ones of length <= radius, 64 of length exactly radius, and the two axes' ends"""
    rng = np.random.default_rng(seed)
    ang = rng.uniform(0, 2 * np.pi, n)
    r = radius * np.sqrt(rng.random(n))
    ring = np.linspace(0, 2 * np.pi, 64, endpoint=False)
    e = np.concatenate([np.stack([r * np.cos(ang), r * np.sin(ang)], -1),
                        radius * np.stack([np.cos(ring), np.sin(ring)], -1),
                        radius * np.array([[1, 0], [-1, 0], [0, 1], [0, -1], [0, 0]], np.float64)])
    return e


@pytest.mark.parametrize("axis,sign,cell", [(0, 1, (15, 0)), (0, -1, (-15, 0)), (1, 1, (0, 15)), (1, -1, (0, -15)),
                                            (2, 1, (0, 0))], ids=["+x", "-x", "+y", "-y", "+z"])
def test_axis_directions_are_cell_centres(axis, sign, cell):
    """+-x, +-y and +z lie in the middle of a direction cell: a bundle around them, perturbed by up to 0.02 (any direction
    in the plane of the other two components), stays in that one cell.

    The cell around +-x and +-y is the diamond |e1| + |e2| < 1/29 = 0.0345 of the two other components (15 / (1 + s) >
    14.5), pinned below: 0.02 in BOTH components at once (s = 0.04) is outside it, so the perturbation here is bounded in
    length, not per component.  Around +z the cell is |e| / (1 + |e1| + |e2|) < 1/30 per component, and the whole box
    [-0.02, 0.02]^2 stays inside."""
    other = [k for k in range(3) if k != axis]
    e = _disc(0.02)
    if axis == 2:
        g = np.linspace(-0.02, 0.02, 41)
        e = np.concatenate([e, np.stack(np.meshgrid(g, g), -1).reshape(-1, 2)])
    vel = np.zeros((len(e), 3))
    vel[:, axis] = sign
    vel[:, other] = e
    for scale in (1.0, 0.37, 40.0):                      # the key does not depend on the speed
        got = _cells(vel * scale)
        assert (got == np.array(cell)).all(), (cell, np.unique(got, axis=0))
    if axis != 2:
        rng = np.random.default_rng(9)
        for s, inside in ((1 / 29 - 1e-4, True), (1 / 29 + 1e-4, False)):
            t = rng.uniform(-1, 1, 500)
            vel[:500, other[0]], vel[:500, other[1]] = s * t, s * (1 - np.abs(t)) * rng.choice([-1, 1], 500)
            got = (_cells(vel[:500]) == np.array(cell)).all(axis=1)
            assert got.all() if inside else not got.any(), (s, got.mean())


def test_minus_z_is_a_corner_of_the_direction_map():
    """(0, 0, -1) is pinned to the cell (15, 15), and it is a CORNER of the octahedral square, not a centre: a -z bundle with
    noise of either sign in x and y -- the exit rays of a +z view, which an adjoint that sorts for itself heads along --
    splits over the four cells (+-15, +-15), one per sign pair, each with its own frame.  Pinned, not fixed:
    moving the corner changes the key, which needs a measurement."""
    assert _cells([[0, 0, -1]]).tolist() == [[15, 15]]
    assert _cells([[-0.0, -0.0, -1]]).tolist() == [[15, 15]]
    for eps in (1e-6, 1e-3, 0.02):
        vel = np.array([[sx * eps, sy * eps, -1.0] for sx in (1, -1) for sy in (1, -1)])
        assert _cells(vel).tolist() == [[15, 15], [15, -15], [-15, 15], [-15, -15]]
    # the adjoint of a +z view of the aligned source: every exit ray heads along (0, 0, 1), the sort negates it
    vel = np.tile(np.array([[0.0, 0.0, 1.0]], np.float32), (4, 1))
    pos = np.zeros((4, 3), np.float32)
    assert np.stack(cell_of(H.lightfield_keys(RES_C, H_C, pos, vel, -1.0)), -1).tolist() == [[15, 15]] * 4


# ---- d. the keys of the fuzz rays --------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fuzz_keys(seed, sign):
    """The host build's keys of cases.fuzz_config(seed) heading along sign * vel, the fp32 restatement and the float64
    referee, once; callers must not modify them."""
    c = cases.fuzz_config(seed)
    a = (c["res"], c["h"], c["pos"], c["vel"], sign)
    lf32, ch32 = S.lightfield32(*a), S.chord32(*a)
    return dict(c=c, lf_host=H.lightfield_keys(*a), ch_host=H.chord_keys(*a), lf32=lf32, ch32=ch32,
                lf64=S.lightfield64(*a), ch64=S.chord64(*a, hit32=ch32["hit"]))


@pytest.mark.parametrize("sign", SIGNS)
@pytest.mark.parametrize("seed", SEEDS)
def test_keys_of_the_fuzz_rays(seed, sign):
    """Host-build keys bit-equal to the fp32 restatement, equal to the float64 referee on the decided rays, for both key
    kinds; the undecided share of the moving rays stays within the cap (so `decided` cannot hollow the comparison out)."""
    k = fuzz_keys(seed, sign)
    moving = ~k["lf32"]["rest"]
    assert np.array_equal(k["lf32"]["rest"], k["lf64"]["rest"]) and 0 < (~moving).sum() < 60
    for host, r32, r64, name in ((k["lf_host"], k["lf32"], k["lf64"], "light-field"), (k["ch_host"], k["ch32"], k["ch64"], "chord")):
        assert host.dtype == r32["key"].dtype == r64["key"].dtype
        bad = np.nonzero(host != r32["key"])[0]
        assert bad.size == 0, (name, "fp32 restatement", bad[:5], host[bad[:5]], r32["key"][bad[:5]])
        bad = np.nonzero((host != r64["key"]) & r64["decided"])[0]
        assert bad.size == 0, (name, "float64 referee", bad[:5], host[bad[:5]], r64["key"][bad[:5]], r64["dist"][bad[:5]])
        undecided = float((~r64["decided"])[moving].sum()) / moving.sum()
        assert undecided <= S.UNDECIDED_CAP, (name, undecided)
    assert (k["lf_host"][~moving] == 0).all()
    # the fuzz reaches what it is for: many direction cells, both hemispheres, chords that miss the box
    a, b = cell_of(k["lf_host"][moving])
    assert len(set(zip(a.tolist(), b.tolist()))) > 300 and 0.3 < k["ch32"]["hit"].mean() < 0.9
    assert S.order_consistent(S.visit_order(k["lf_host"]), k["lf64"]["key"], k["lf64"]["decided"])
    assert S.order_consistent(S.visit_order(k["ch_host"]), k["ch64"]["key"], k["ch64"]["decided"])


def test_adjoint_heading_is_minus_vt():
    """sign = -1 is the key of the reversed ray, not of the ray: equal to the host key of (pos, -vel) with sign = +1 (negation
    is exact), and different from the sign = +1 key on nearly every moving ray."""
    for seed in SEEDS[:3]:
        k, kp = fuzz_keys(seed, -1.0), fuzz_keys(seed, 1.0)
        c = k["c"]
        assert np.array_equal(k["lf_host"], H.lightfield_keys(c["res"], c["h"], c["pos"], -c["vel"], 1.0))
        assert np.array_equal(k["ch_host"], H.chord_keys(c["res"], c["h"], c["pos"], -c["vel"], 1.0))
        moving = ~k["lf32"]["rest"]
        assert (k["lf_host"] != kp["lf_host"])[moving].mean() > 0.99
        assert (k["ch_host"] != kp["ch_host"])[moving & k["ch32"]["hit"]].mean() > 0.9


def test_order_consistent_sees_what_it_should():
    """The helper itself: it accepts the stable order, refuses an unstable tie and a descent among decided rays, and looks
    away from undecided ones."""
    keys = np.array([5, 3, 5, 0, 3, 9], np.uint32)
    all_ = np.ones(6, bool)
    assert S.visit_order(keys).tolist() == [3, 1, 4, 0, 2, 5]
    assert S.order_consistent([3, 1, 4, 0, 2, 5], keys, all_)
    assert not S.order_consistent([3, 4, 1, 0, 2, 5], keys, all_)            # tie 1, 4 out of index order
    assert not S.order_consistent([3, 1, 4, 0, 5, 2], keys, all_)            # 9 before 5
    undecided = all_.copy(); undecided[5] = False
    assert S.order_consistent([3, 1, 4, 0, 5, 2], keys, undecided)


# ---- e. the aligned source ---------------------------------------------------------------------------------------------
RES_E, H_E, SIDE = (33, 33, 33), 0.37, 64


@functools.lru_cache(maxsize=None)
def lattice_rays(axis, sign, seed=11):
    """64 x 64 rays from the pixel centres (i + 0.5) E / 64 of the face the rays enter through, collimated along sign * axis,
    shuffled -> (pos, vel, pixel i, pixel j); callers must not modify them."""
    E = float(np.float32(RES_E[0] - 1) * np.float32(H_E))
    i, j = (v.ravel() for v in np.meshgrid(np.arange(SIDE), np.arange(SIDE), indexing="ij"))
    other = [k for k in range(3) if k != axis]
    pos = np.zeros((SIDE * SIDE, 3))
    pos[:, other[0]], pos[:, other[1]] = (i + 0.5) * E / SIDE, (j + 0.5) * E / SIDE
    pos[:, axis] = 0.0 if sign > 0 else E
    vel = np.zeros_like(pos)
    vel[:, axis] = sign
    perm = np.random.default_rng(seed).permutation(SIDE * SIDE)
    return pos[perm].astype(np.float32), vel[perm].astype(np.float32), i[perm], j[perm]


@pytest.mark.parametrize("axis,sign", [(a, s) for a in range(3) for s in (1, -1)], ids=["+x", "-x", "+y", "-y", "+z", "-z"])
def test_aligned_source_keeps_perfect_tiles(axis, sign):
    """33^3 grid, h = 0.37, a 64 x 64 plane source on pixel centres, shuffled: each group of 64 consecutive rays of the
    stable order is exactly one 8 x 8 pixel tile (the power-of-two offset scale keeps pixel boundaries on key-cell
    boundaries, and aligned 8 x 8 blocks of the Hilbert curve are contiguous).  A pixel is 16 key cells wide, so its centre
    lies ON a cell boundary and fp32 rounding picks the cell to either side -- the float64 referee cannot name the key, but
    it names the pixel: both cells are 8 cells from the pixel's edge, and the host build's cell lies in the referee's pixel."""
    pos, vel, i, j = lattice_rays(axis, sign)
    keys = H.lightfield_keys(RES_E, H_E, pos, vel)
    r64 = S.lightfield64(RES_E, H_E, pos, vel)
    assert np.array_equal(keys, S.lightfield32(RES_E, H_E, pos, vel)["key"])
    cont = r64["cont"][:, 2:]
    assert np.abs(cont / 16 - np.rint(cont / 16)).min() * 16 > 7.9          # key cells to the nearest pixel edge
    assert all(np.array_equal(got >> 4, np.floor(want / 16).astype(np.int64)) for got, want in zip(offsets_of(keys), cont.T))
    assert (r64["dist"][:, :2] == 0.5).all() and np.array_equal(np.stack(cell_of(keys)), np.stack(cell_of(r64["key"])))
    assert len(set(zip(*(v.tolist() for v in cell_of(keys))))) == 1 and len(np.unique(keys)) == SIDE * SIDE
    order = S.visit_order(keys)
    ti, tj = (i[order] >> 3).reshape(-1, 64), (j[order] >> 3).reshape(-1, 64)
    assert (ti == ti[:, :1]).all() and (tj == tj[:, :1]).all()
    pixels = (i[order] * SIDE + j[order]).reshape(-1, 64)
    assert all(len(set(row)) == 64 for row in pixels.tolist())
    assert len(set(zip(ti[:, 0].tolist(), tj[:, 0].tolist()))) == 64


# ---- f. edge cases -----------------------------------------------------------------------------------------------------
def _both(res, h, pos, vel, sign=1.0):
    """host keys of both kinds, asserted bit-equal to the restatement -> (light-field, chord)"""
    lf, ch = H.lightfield_keys(res, h, pos, vel, sign), H.chord_keys(res, h, pos, vel, sign)
    assert np.array_equal(lf, S.lightfield32(res, h, pos, vel, sign)["key"])
    assert np.array_equal(ch, S.chord32(res, h, pos, vel, sign)["key"])
    return lf, ch


def test_resting_and_non_finite_directions():
    """A ray at rest gives key 0; a NaN, Inf, 3e38 or 1e-40 direction component gives key 0 or a valid key."""
    pos = np.array([[0.4, 0.3, 0.2]], np.float32)
    lf, _ = _both(RES_C, H_C, pos, np.zeros((1, 3)))
    assert lf.tolist() == [0]
    lf, _ = _both(RES_C, H_C, pos, np.array([[-0.0, 0.0, -0.0]]), -1.0)
    assert lf.tolist() == [0]
    bad = [np.nan, np.inf, -np.inf, 3e38, -3e38, 1e-40, -1e-40, 1e-45]
    vel = []
    for v in bad:
        for comp in range(3):
            for base in ([0.3, -0.5, 0.8], [0.0, 0.0, 0.0]):
                d = list(base); d[comp] = v
                vel.append(d)
        vel.append([v, v, v])
    vel = np.array(vel, np.float32)
    for sign in SIGNS:
        lf, ch = _both(RES_C, H_C, np.tile(pos, (len(vel), 1)), vel, sign)
        assert ((lf >> CELL_SHIFT) < N_CELLS).all() and (ch >> np.uint64(60) == 0).all()
        big = ~np.isfinite(vel).all(axis=1) | (np.abs(vel) > 1e38).any(axis=1)
        assert (lf[big] == 0).all()                              # the length is not finite: "at rest"
        alone = (np.abs(vel) < 1e-39).all(axis=1)                # a denormal direction: its square underflows, length 0
        assert alone.any() and (lf[alone] == 0).all()
        mixed = ~big & ~alone                                    # a denormal beside ordinary components: an ordinary ray
        assert mixed.any() and (lf[mixed] != 0).all()


def test_non_finite_and_huge_positions_give_clamped_offsets():
    vel = np.array([[0.3, -0.5, 0.8]], np.float32)
    rows = []
    for v in (np.nan, np.inf, -np.inf, 3e38, -3e38, 1e30):
        for comp in range(3):
            p = [0.4, 0.3, 0.2]; p[comp] = v
            rows.append(p)
        rows.append([v, v, v])
    pos = np.array(rows, np.float32)
    for sign in SIGNS:
        lf, ch = _both(RES_C, H_C, pos, np.tile(vel, (len(pos), 1)), sign)
        assert (ch >> np.uint64(60) == 0).all()
        a, b = cell_of(lf)
        want = cell_of(H.lightfield_keys(RES_C, H_C, np.array([[0.4, 0.3, 0.2]], np.float32), vel, sign))
        assert (a == want[0]).all() and (b == want[1]).all()     # the direction part does not look at the position
        qu, qv = offsets_of(lf)
        assert np.isin(qu, (0, S.POS_CELLS - 1)).all() and np.isin(qv, (0, S.POS_CELLS - 1)).all()
        nan = np.isnan(pos).any(axis=1)
        assert (qu[nan] == 0).all() and (qv[nan] == 0).all()


def test_zero_extent_volume():
    """The 1 x 1 x 1 volume, which the march accepts: extent 0, so the offset scale is 0 and u = v = 0.5 for every ray with
    a finite position; the chord key's 1 / b is replaced by 0 and the key is 0."""
    c = cases.fuzz_config(3)
    for sign in SIGNS:
        lf, ch = _both((1, 1, 1), 0.25, c["pos"], c["vel"], sign)
        moving = (c["vel"] != 0).any(axis=1)
        assert (lf[~moving] == 0).all() and (ch == 0).all()
        qu, qv = offsets_of(lf[moving])
        assert (qu == S.POS_CELLS // 2).all() and (qv == S.POS_CELLS // 2).all()
        assert np.array_equal(np.stack(cell_of(lf[moving])), np.stack(cell_of(H.lightfield_keys(c["res"], c["h"], c["pos"], c["vel"], sign)[moving])))


def test_ties_keep_their_index_order():
    """Resting rays all have key 0: the stable order visits them first, in increasing ray index; equal keys of moving rays
    (duplicated rays) likewise."""
    c = cases.fuzz_config(5)
    pos, vel = np.concatenate([c["pos"], c["pos"][::-1]]), np.concatenate([c["vel"], c["vel"][::-1]])
    vel[::7] = 0.0
    keys = H.lightfield_keys(c["res"], c["h"], pos, vel)
    order = S.visit_order(keys)
    rest = np.nonzero((vel == 0).all(axis=1))[0]
    assert len(rest) > 170 and np.array_equal(order[:len(rest)], rest)
    r64 = S.lightfield64(c["res"], c["h"], pos, vel)
    assert S.order_consistent(order, r64["key"], r64["decided"])
    assert not S.order_consistent(order[::-1], r64["key"], r64["decided"])
    swapped = order.copy(); swapped[[0, 1]] = swapped[[1, 0]]
    assert not S.order_consistent(swapped, r64["key"], r64["decided"])


# ---- g. the key functions under sanitizers ------------------------------------------------------------------------------
def test_keys_under_sanitizers(tmp_path):
    """tests/hostcheck/keys_sanitize.hip: a stand-alone program over drrt_keys.h, compiled for the host with ASan + UBSan and
    run directly (nothing preloaded): the specials of the edge-case tests and a few thousand random rays through both
    keys, no report."""
    here = os.path.dirname(os.path.abspath(__file__))
    hipcc = "/opt/rocm/bin/hipcc"
    rt = glob.glob("/opt/rocm*/lib/llvm/lib/clang/*/lib/linux/libclang_rt.asan-x86_64.a")
    if not rt or not os.path.exists(hipcc):
        pytest.skip("no clang sanitizer runtime in this image")
    exe = str(tmp_path / "keys_sanitize")
    subprocess.run([hipcc, "--cuda-host-only", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-mfma",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                    os.path.join(here, "hostcheck", "keys_sanitize.hip")], check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "finished without reports" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
