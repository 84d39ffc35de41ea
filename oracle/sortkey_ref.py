"""Referee of the locality-sort keys (csrc/drrt_keys.h, csrc/drrt_sort.hip) and of the visit order they give.  numpy only,
imported by tests only (tests/test_sortkey_ref.py on the host, tests/test_sort_order.py on the GPU); it never calls the
library, its host build or the device.

Three layers:

* the Hilbert index `xy2d` from the curve's recursive definition, and its inverse `d2xy` by the classic bottom-up walk;
* `lightfield32` / `chord32`: the two keys restated in fp32 with the kernels' operation order (one IEEE operation per
  numpy operation; the one FMA of the chord key is emulated exactly).  The host build must equal them bit for bit;
* `lightfield64` / `chord64`: the same geometry in float64, returning next to the key the CONTINUOUS quantities that
  are rounded or truncated into it.  A ray is *decided* when every such quantity is farther than MARGIN key cells from
  the boundary at which its integer changes; on decided rays fp32 and float64 must give the same key, whatever the
  rounding of the fp32 operations.

The direction cell's frame is the one thing the float64 referee does not re-derive: where the cell's centre has two
components of equal magnitude in exact arithmetic (a = b = 5: cx = cz = 1/3) the "least aligned axis" is chosen by fp32
rounding, float64 picks the other axis, and both frames are valid.  `frames32()` is a function of the 961 integer pairs
only; tests check its orthonormality in float64 and the referee uses it for the float64 offsets.

MARGIN: 1e-3 key cells.  Measured with these restatements (fp32 against float64, nothing else) on cases.fuzz_config seeds
0..199, 120 000 rays per sign: the light-field keys differ on 10 rays (sign +1) / 13 rays (sign -1), the farthest 8.9e-5 /
9.5e-5 cell from a boundary; the chord keys on 8 / 12 rays, the farthest 3.7e-5 / 4.2e-5 cell (NOTES.md, "Sort-key
referee").  1e-3 is more than 10 x the largest.
"""
import numpy as np

F = np.float32
DIR_HALF = 15
DIR_CELLS = 2 * DIR_HALF + 1
POS_BITS = 11
POS_CELLS = 1 << POS_BITS
CHORD_BITS = 10
CHORD_CELLS = 1 << CHORD_BITS
MARGIN = 1e-3
UNDECIDED_CAP = 0.03          # of the non-resting rays of a seed


# ---- Hilbert curve ------------------------------------------------------------------------------------------------------
def xy2d(x, y, bits=POS_BITS):
    """Hilbert index of the cell (x, y) of a 2^bits x 2^bits grid, by the curve's recursive definition: the curve of order
    k visits its four quadrants in the order (0,0), (0,1), (1,1), (1,0) -- it starts at (0, 0), ends at (2^k - 1, 0) -- and
    inside them runs the curve of order k - 1: transposed in the first quadrant, as it is in the second and third,
    transposed about the anti-diagonal in the fourth."""
    x = np.asarray(x).astype(np.int32); y = np.asarray(y).astype(np.int32)          # 2 * bits <= 30
    d = np.zeros(x.shape, np.int32)
    for k in range(bits, 0, -1):
        half = 1 << (k - 1)
        right, upper = x >= half, y >= half
        quadrant = np.where(right, np.where(upper, 2, 3), np.where(upper, 1, 0))
        d += quadrant * half * half
        lx, ly = x - half * right, y - half * upper                  # coordinates inside the quadrant
        first, fourth = quadrant == 0, quadrant == 3
        x = np.where(first, ly, np.where(fourth, half - 1 - ly, lx))
        y = np.where(first, lx, np.where(fourth, half - 1 - lx, ly))
    return d.astype(np.int64)


def d2xy(d, bits=POS_BITS):
    """Inverse of xy2d: the classic bottom-up walk (two bits of the index per level, smallest square first)."""
    t = np.asarray(d).astype(np.int32)
    x = np.zeros(t.shape, np.int32); y = np.zeros(t.shape, np.int32)
    s = 1
    while s < (1 << bits):
        rx = 1 & (t // 2)
        ry = 1 & (t ^ rx)
        flip = (ry == 0) & (rx == 1)
        x, y = np.where(flip, s - 1 - x, x), np.where(flip, s - 1 - y, y)
        x, y = np.where(ry == 0, y, x), np.where(ry == 0, x, y)
        x += s * rx; y += s * ry
        t //= 4
        s *= 2
    return x.astype(np.int64), y.astype(np.int64)


# ---- helpers ----------------------------------------------------------------------------------------------------------
def box32(res, h):
    """(bx, by, bz) of the Vol that vol_finish builds: (float)(res - 1) * h in fp32."""
    return np.array([F(r - 1) * F(h) for r in res], F)


def _sgn(x, one):
    return np.where(x >= 0, one, -one)


def _fma32(a, b, c):
    """fmaf(a, b, c) for float32 arrays, exactly: the product is exact in float64, the sum is rounded to odd there (TwoSum
    tells which way it was rounded), so the final rounding to float32 is the single rounding of the exact value."""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    fix = np.isfinite(s) & np.isfinite(err) & (err != 0) & ((s.view(np.int64) & 1) == 0)
    s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return s.astype(F)


def _trunc_clamped(x, hi):
    """(uint32)fminf(fmaxf(x, 0), hi): NaN goes to 0."""
    return np.fmin(np.fmax(x, x.dtype.type(0)), x.dtype.type(hi)).astype(np.int64)


def _dist_half_integer(x):
    """distance of x to the nearest half-integer (where rint changes)"""
    return np.abs((x - 0.5) - np.rint(x - 0.5))


def _dist_interior_integer(x, cells):
    """distance of x to the nearest of 1 .. cells - 1 (where a truncation clamped to [0, cells - 1] changes)"""
    return np.abs(x - np.clip(np.rint(x), 1, cells - 1))


def _interleave6(q):
    """q: (n,6) integers of CHORD_BITS bits -> the 60-bit Morton key, coordinate 0 in the highest bit of each group"""
    key = np.zeros(len(q), np.uint64)
    for bit in range(CHORD_BITS):
        for j in range(6):
            key |= ((q[:, j].astype(np.uint64) >> np.uint64(bit)) & np.uint64(1)) << np.uint64(6 * bit + (5 - j))
    return key


def _lf_key(a, b, qu, qv):
    cell = (a + DIR_HALF) * DIR_CELLS + (b + DIR_HALF)
    return ((cell.astype(np.int64) << (2 * POS_BITS)) | xy2d(qu, qv)).astype(np.uint32)


def _octa(d, one):
    """octahedral map of unit directions d (n,3) -> (ox, oy) in [-1, 1]^2, in d's precision"""
    l1 = np.abs(d[:, 0]) + np.abs(d[:, 1]) + np.abs(d[:, 2])
    ox, oy = d[:, 0] / l1, d[:, 1] / l1
    fx, fy = (one - np.abs(oy)) * _sgn(ox, one), (one - np.abs(ox)) * _sgn(oy, one)
    low = d[:, 2] < 0
    return np.where(low, fx, ox), np.where(low, fy, oy)


# ---- the 961 frames (fp32) ----------------------------------------------------------------------------------------------
_frames = None


def frames32():
    """-> (c, t1, t2), each float32 (31, 31, 3), indexed [a + 15, b + 15]: lf_cell_frame restated in fp32."""
    global _frames
    if _frames is None:
        a, b = (g.ravel() for g in np.meshgrid(np.arange(-DIR_HALF, DIR_HALF + 1), np.arange(-DIR_HALF, DIR_HALF + 1),
                                               indexing="ij"))
        one = F(1)
        cx, cy = a.astype(F) / F(DIR_HALF), b.astype(F) / F(DIR_HALF)
        cz = one - np.abs(cx) - np.abs(cy)
        fx, fy = (one - np.abs(cy)) * _sgn(cx, one), (one - np.abs(cx)) * _sgn(cy, one)
        low = cz < 0
        cx, cy = np.where(low, fx, cx), np.where(low, fy, cy)
        cl = one / np.sqrt(cx * cx + cy * cy + cz * cz)
        c = np.stack([cx * cl, cy * cl, cz * cl], -1)
        n = np.arange(len(a))
        ax = np.zeros(len(a), np.int64)
        ax = np.where(np.abs(c[:, 1]) < np.abs(c[n, ax]), 1, ax)
        ax = np.where(np.abs(c[:, 2]) < np.abs(c[n, ax]), 2, ax)
        t1 = (-c[n, ax])[:, None] * c
        t1[n, ax] += one
        tl = one / np.sqrt(t1[:, 0] * t1[:, 0] + t1[:, 1] * t1[:, 1] + t1[:, 2] * t1[:, 2])
        t1 = t1 * tl[:, None]
        t2 = np.stack([c[:, 1] * t1[:, 2] - c[:, 2] * t1[:, 1], c[:, 2] * t1[:, 0] - c[:, 0] * t1[:, 2],
                       c[:, 0] * t1[:, 1] - c[:, 1] * t1[:, 0]], -1)
        assert c.dtype == t1.dtype == t2.dtype == F
        _frames = tuple(v.reshape(DIR_CELLS, DIR_CELLS, 3) for v in (c, t1, t2))
        for v in _frames:
            v.setflags(write=False)
    return _frames


# ---- light-field key ----------------------------------------------------------------------------------------------------
def lightfield32(res, h, pos, vel, sign=1.0):
    """lightfield_key restated in fp32 -> dict(key uint32, rest bool, a, b, qu, qv); a .. qv are 0 on resting rays."""
    with np.errstate(all="ignore"):
        p = np.asarray(pos, F)
        d = F(sign) * np.asarray(vel, F)
        one = F(1)
        ln = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
        rest = ~(ln > F(1e-30)) | ~(ln < F(3.0e38))
        il = one / ln
        d = d * il[:, None]
        ox, oy = _octa(d, one)
        a = np.clip(np.nan_to_num(np.rint(ox * F(DIR_HALF))), -DIR_HALF, DIR_HALF).astype(np.int64)
        b = np.clip(np.nan_to_num(np.rint(oy * F(DIR_HALF))), -DIR_HALF, DIR_HALF).astype(np.int64)
        _, T1, T2 = frames32()
        t1, t2 = T1[a + DIR_HALF, b + DIR_HALF], T2[a + DIR_HALF, b + DIR_HALF]
        bx = box32(res, h)
        w = p - F(0.5) * bx
        wd = w[:, 0] * d[:, 0] + w[:, 1] * d[:, 1] + w[:, 2] * d[:, 2]
        q = w - wd[:, None] * d
        ext = max(bx[0], max(bx[1], bx[2]))
        sc = F(0.5) / ext if ext > 0 else F(0)
        u = (q[:, 0] * t1[:, 0] + q[:, 1] * t1[:, 1] + q[:, 2] * t1[:, 2]) * sc + F(0.5)
        v = (q[:, 0] * t2[:, 0] + q[:, 1] * t2[:, 1] + q[:, 2] * t2[:, 2]) * sc + F(0.5)
        assert u.dtype == v.dtype == F
        qu, qv = _trunc_clamped(u * F(POS_CELLS), POS_CELLS - 1), _trunc_clamped(v * F(POS_CELLS), POS_CELLS - 1)
        key = np.where(rest, np.uint32(0), _lf_key(a, b, qu, qv))
    z = lambda arr: np.where(rest, 0, arr)
    return dict(key=key, rest=rest, a=z(a), b=z(b), qu=z(qu), qv=z(qv))


def lightfield64(res, h, pos, vel, sign=1.0, margin=MARGIN):
    """The float64 referee -> dict(key, rest, a, b, qu, qv, cont, dist, decided): `cont` (n,4) = 15 ox, 15 oy, 2048 u,
    2048 v before rounding / truncation, `dist` (n,4) their distances to the nearest boundary (half-integers for the two
    rounded ones; the interior integers 1 .. 2047 for the truncated ones, the clamped ends are no boundaries), `decided` =
    every distance above `margin`.  A resting ray (zero or non-finite direction) is decided with key 0; a direction of a
    length at which fp32 squares underflow or overflow, between resting and not, is undecided."""
    with np.errstate(all="ignore"):
        p = np.asarray(pos, F).astype(np.float64)
        d = float(sign) * np.asarray(vel, F).astype(np.float64)
        ln = np.sqrt((d * d).sum(1))
        rest = ~np.isfinite(ln) | (ln == 0)
        grey = ~rest & ((ln < 1e-15) | (ln > 1e18))
        d = d / ln[:, None]
        ox, oy = _octa(d, 1.0)
        ca, cb = DIR_HALF * ox, DIR_HALF * oy
        a = np.clip(np.nan_to_num(np.rint(ca)), -DIR_HALF, DIR_HALF).astype(np.int64)
        b = np.clip(np.nan_to_num(np.rint(cb)), -DIR_HALF, DIR_HALF).astype(np.int64)
        _, T1, T2 = frames32()
        t1, t2 = T1[a + DIR_HALF, b + DIR_HALF].astype(np.float64), T2[a + DIR_HALF, b + DIR_HALF].astype(np.float64)
        bx = box32(res, h).astype(np.float64)
        w = p - 0.5 * bx
        q = w - (w * d).sum(1)[:, None] * d
        ext = bx.max()
        sc = 0.5 / ext if ext > 0 else 0.0
        cu = ((q * t1).sum(1) * sc + 0.5) * POS_CELLS
        cv = ((q * t2).sum(1) * sc + 0.5) * POS_CELLS
        qu, qv = _trunc_clamped(cu, POS_CELLS - 1), _trunc_clamped(cv, POS_CELLS - 1)
        cont = np.stack([ca, cb, cu, cv], -1)
        dist = np.stack([_dist_half_integer(ca), _dist_half_integer(cb), _dist_interior_integer(cu, POS_CELLS),
                         _dist_interior_integer(cv, POS_CELLS)], -1)
        decided = np.where(rest, True, ~grey & (dist > margin).all(1))          # NaN distances compare false
        key = np.where(rest, np.uint32(0), _lf_key(a, b, qu, qv))
    z = lambda arr: np.where(rest, 0, arr)
    return dict(key=key, rest=rest, a=z(a), b=z(b), qu=z(qu), qv=z(qv), cont=cont, dist=dist, decided=decided)


# ---- chord key ----------------------------------------------------------------------------------------------------------
def _chord(p, d, bx, T, fma):
    """the slab test and the six end-point coordinates in the precision T of p, d, bx -> (hit, e (n,6) = e0 xyz, e1 xyz)"""
    n = len(p)
    zero = T(0)
    tmin, tmax = np.zeros(n, T), np.full(n, T(F(3.0e38)), T)
    hit = np.ones(n, bool)
    for a in range(3):
        moving = np.abs(d[:, a]) > T(F(1e-20))
        inv = T(1) / d[:, a]
        t1, t2 = (zero - p[:, a]) * inv, (bx[a] - p[:, a]) * inv
        tmin = np.where(moving, np.fmax(tmin, np.fmin(t1, t2)), tmin)
        tmax = np.where(moving, np.fmin(tmax, np.fmax(t1, t2)), tmax)
        hit &= moving | ~((p[:, a] < zero) | (p[:, a] > bx[a]))
    hit &= tmax >= tmin
    t0, t1 = np.where(hit, tmin, zero), np.where(hit, tmax, zero)
    e = []
    for t in (t0, t1):
        for a in range(3):
            inv_b = T(1) / bx[a] if bx[a] > 0 else zero
            e.append(fma(t, d[:, a], p[:, a]) * inv_b)
    return hit, np.stack(e, -1)


def chord32(res, h, pos, vel, sign=1.0):
    """chord_key restated in fp32 -> dict(key uint64, hit bool, q (n,6))."""
    with np.errstate(all="ignore"):
        p, d = np.asarray(pos, F), F(sign) * np.asarray(vel, F)
        hit, e = _chord(p, d, box32(res, h), F, _fma32)
        assert e.dtype == F
        e = np.fmin(np.fmax(e, F(0)), F(0.99999))
        q = (e * F(CHORD_CELLS)).astype(np.int64)
    return dict(key=_interleave6(q), hit=hit, q=q)


def chord64(res, h, pos, vel, sign=1.0, hit32=None, margin=MARGIN):
    """The float64 referee of the chord key -> dict(key, hit, q, cont, dist, decided): `cont` (n,6) the six e * 1024 before
    truncation, `dist` their distances to the interior integers 1 .. 1023 (the clamps at 0 and 0.99999 are no boundaries).
    Undecided: a distance within `margin`, a `hit` that differs from the fp32 restatement's (`hit32`), a direction
    component within a factor 10 of the 1e-20 threshold, a non-finite quantity."""
    with np.errstate(all="ignore"):
        p = np.asarray(pos, F).astype(np.float64)
        d = float(sign) * np.asarray(vel, F).astype(np.float64)
        hit, e = _chord(p, d, box32(res, h).astype(np.float64), np.float64, lambda t, dd, pp: t * dd + pp)
        cont = e * CHORD_CELLS
        clamped = np.fmin(np.fmax(e, 0.0), float(F(0.99999)))
        q = (clamped * CHORD_CELLS).astype(np.int64)
        dist = _dist_interior_integer(cont, CHORD_CELLS)
        grey = ((np.abs(d) > 1e-21) & (np.abs(d) < 1e-19)).any(1)
        decided = (dist > margin).all(1) & ~grey & np.isfinite(cont).all(1)
        if hit32 is not None:
            decided &= hit == np.asarray(hit32, bool)
    return dict(key=_interleave6(q), hit=hit, q=q, cont=cont, dist=dist, decided=decided)


# ---- orders -------------------------------------------------------------------------------------------------------------
def visit_order(keys):
    """The order a stable sort of the keys visits the rays in."""
    return np.argsort(np.asarray(keys), kind="stable")


def order_consistent(order, ref_keys, decided):
    """Is `order`, restricted to the decided rays, a stable sort by `ref_keys`: keys non-decreasing, equal keys in
    increasing ray index?"""
    order = np.asarray(order, np.int64)
    sub = order[np.asarray(decided, bool)[order]]
    k = np.asarray(ref_keys)[sub].astype(np.uint64)
    return bool(np.all(k[1:] >= k[:-1]) and np.all((sub[1:] > sub[:-1])[k[1:] == k[:-1]]))
