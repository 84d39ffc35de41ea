"""GPU tier of the locality sort: the order the device visits the rays in, for every entry point that sorts, against

  1. "it is a permutation";
  2. the stable argsort of the HOST BUILD's keys (tests/hostcheck over csrc/drrt_keys.h) -- exactly: the same key
     arithmetic, a stable sort;
  3. the float64 referee (oracle/sortkey_ref.py) on the rays it decides: keys non-decreasing, ties in ray-index order.

Results come back in the caller's ray order, so no parity test sees any of this: a wrong key or an unstable sort only makes
the windowed adjoints fall back to global atomics.  (2) failing while (3) holds means that the device and the host round
some operation of the key differently; (2) and (3) failing together, with the host tier (tests/test_sortkey_ref.py)
passing, points at the sort or at how an entry hands its rays and heading to it.

The forward marches leave their order in `drrt.last_order`.  The adjoints that sort for themselves do not refresh that
attribute (it is the hand-over from a forward call to its adjoint), so for them the test reads the same thing the
attribute is a view of: drrt_last_order() of the call just made, through the module's own view helper."""
import functools
import time

import numpy as np
import pytest
import torch

import cases
import hostcheck_lib as H
from oracle import sortkey_ref as S
from ray16_common import SEEDS, referee

pytestmark = pytest.mark.gpu

FORWARD = ("trace", "trace_pln", "trace_sdf", "trace_target")
ADJOINT = ("backtrace", "backtrace_sdf", "backtrace_rays", "backtrace_pln_rays", "backtrace_sdf_rays")
# which rays an entry makes its keys from, and which way they head (GridCall::place in csrc/drrt_api.hip)
HEADING = dict(trace=1.0, trace_pln=1.0, trace_sdf=1.0, trace_target=1.0, backtrace=-1.0, backtrace_sdf=-1.0,
               backtrace_rays=-1.0, backtrace_pln_rays=1.0, backtrace_sdf_rays=1.0)


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _np(t):
    return t.cpu().numpy()


def expected_order(res, h, pos, vel, sign, chord):
    """-> (host-build keys, their stable argsort)"""
    keys = (H.chord_keys if chord else H.lightfield_keys)(res, h, pos, vel, sign)
    return keys, S.visit_order(keys)


@functools.lru_cache(maxsize=None)
def fuzz_referee(seed, sign, chord):
    """The referee of the seed's input rays, once; callers must not modify it."""
    c = cases.fuzz_config(seed)
    return referee(c["res"], c["h"], c["pos"], c["vel"], sign, chord)


def check_order(order, res, h, pos, vel, sign, chord, what, ref=None):
    """The three assertions on a device order; `ref` = (float64 keys, decided), None: no referee for these rays."""
    n = len(pos)
    assert order is not None, (what, "the call left no order")
    order = _np(order) if isinstance(order, torch.Tensor) else np.asarray(order)
    assert order.shape == (n,) and order.dtype == np.int32, (what, order.shape, order.dtype)
    assert np.array_equal(np.sort(order), np.arange(n)), (what, "not a permutation")
    keys, want = expected_order(res, h, pos, vel, sign, chord)
    consistent = None if ref is None else S.order_consistent(order, *ref)
    bad = np.nonzero(order != want)[0]
    assert bad.size == 0, (what, "not the stable argsort of the host build's keys", f"{bad.size} of {n} places",
                           f"consistent with the float64 referee: {consistent}", bad[:5], order[bad[:5]], want[bad[:5]],
                           keys[order[bad[:5]]], keys[want[bad[:5]]])
    assert consistent is not False, (what, "not a stable sort by the float64 referee's keys on the decided rays")


def order_of_last_call(drrt, n, dev):
    """The visit order of the call just made, forward or adjoint: drrt_last_order() as a view of this stream's workspace
    (what drrt.last_order is after a forward march)."""
    return drrt._last_view(drrt._lib.load().drrt_last_order, n, dev)


def run_entry(drrt, T, entry, d, res, h, ds):
    """Make the call -> (order, key positions, key directions): device tensors of the order and of the rays whose keys the
    entry sorts by."""
    R, Sd, P, V, DX, DV = d["rif"], d["sdf"], d["pos"], d["vel"], d["dx"], d["dv"]
    n = P.shape[0]
    if entry in FORWARD:
        if entry == "trace":
            T.trace(R, res, P, V, h, ds)
        elif entry == "trace_pln":
            T.trace_pln(R, res, P, V, d["po"], d["pd"], h, ds)
        elif entry == "trace_sdf":
            T.trace_sdf(R, Sd, res, P, V, h, ds)
        else:
            T.trace_target(R, res, P, V, d["tg"], h, ds)
        return drrt.last_order, P, V
    if entry == "backtrace":                       # started from arbitrary rays, no order handed over: it sorts by (xt, -vt)
        T.backtrace(R, res, P, V, DX, DV, h, ds)
    elif entry == "backtrace_sdf":
        T.backtrace_sdf(R, Sd, res, P, V, DX, DV, h, ds)
    elif entry == "backtrace_pln_rays":            # replays the forward from (pos, vel): sorted as the forward sorts
        T.backtrace_pln_rays(R, res, P, V, d["po"], d["pd"], DX, DV, h, ds)
    elif entry == "backtrace_sdf_rays":
        T.backtrace_sdf_rays(R, Sd, res, P, V, DX, DV, h, ds)
    else:                                          # backtrace_rays: sorted by the forward's exit rays, heading back
        with drrt.using(sort_rays=False):
            xt, vt = T.trace(R, res, P, V, h, ds)
            steps = drrt.keep_steps(drrt.last_steps)
        T.backtrace_rays(R, res, P, V, xt, vt, steps, DX, DV, h, ds)
        return order_of_last_call(drrt, n, P.device), xt, vt
    return order_of_last_call(drrt, n, P.device), P, V


@functools.lru_cache(maxsize=None)
def device_config(seed, dev):
    c = cases.fuzz_config(seed)
    d = {k: _t(c[k], dev) for k in ("pos", "vel", "dx", "dv", "po", "pd", "tg")}
    d["rif"], d["sdf"] = _t(c["rif"], dev).reshape(-1), _t(c["sdf"], dev).reshape(-1)
    return c, d


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("entry", FORWARD + ADJOINT)
def test_order_of_every_sorting_entry(gpu, entry, seed):
    """Every entry that reaches GridCall::place with a sort, light-field and chord key, on the 600 fuzz rays of the seed
    (inside, outside and on the faces of a small non-cubic grid, any heading, 2 % at rest): permutation, stable argsort of
    the host build's keys, consistent with the float64 referee.  trace_target keeps its sort buffers behind its state slot;
    the adjoints head along -vt, the replaying ray-state adjoints along +vel."""
    from adjointnonlinearraytracing_amd import drrt
    c, d = device_config(seed, gpu)
    res, h, ds = c["res"], c["h"], c["ds"]
    T = drrt.TracerC()
    sign = HEADING[entry]
    for chord in (False, True):
        with drrt.using(sort_rays=True, check_failed=False, chord_key=chord):
            order, kp, kv = run_entry(drrt, T, entry, d, res, h, ds)
            order = None if order is None else _np(order).copy()
        if kp is d["pos"]:
            pos, vel, ref = c["pos"], c["vel"], fuzz_referee(seed, sign, chord)
        else:
            pos, vel = _np(kp), _np(kv)
            ref = referee(res, h, pos, vel, sign, chord)
        check_order(order, res, h, pos, vel, sign, chord, (entry, seed, "chord" if chord else "light-field"), ref)


# ---- sizes, on one entry ---------------------------------------------------------------------------------------------------
RES_S, H_S = (5, 4, 3), 0.37


@functools.lru_cache(maxsize=None)
def small_grid(seed=4):
    rng = np.random.default_rng(seed)
    return (1.0 + 0.1 * rng.random((RES_S[2], RES_S[1], RES_S[0]))).astype(np.float32)


def sized_rays(n, seed):
    """n rays around the 5 x 4 x 3 grid: any heading and position, a quarter of them one collimated bundle (one direction
    cell: their order is the Hilbert curve's), some at rest, some duplicated (ties)."""
    rng = np.random.default_rng(seed)
    ext = (np.array(RES_S) - 1) * H_S
    pos = rng.uniform(-0.15, 1.15, (n, 3)) * ext
    vel = rng.normal(size=(n, 3))
    bundle = rng.random(n) < 0.25
    vel[bundle] = [0.0, 0.0, 1.0]
    vel[rng.random(n) < 0.05] = 0.0
    dup = np.nonzero(rng.random(n) < 0.1)[0]
    src = rng.integers(0, n, len(dup))
    pos[dup], vel[dup] = pos[src], vel[src]
    return pos.astype(np.float32), vel.astype(np.float32)


@pytest.mark.parametrize("n", [2, 3, 63, 64, 65, 255, 256, 257, 4097])
def test_order_at_block_and_wave_edges(gpu, n):
    """trace with both keys at ray counts around the wave (64) and the key kernels' block (256), and beyond one block sort."""
    from adjointnonlinearraytracing_amd import drrt
    pos, vel = sized_rays(n, 100 + n)
    T = drrt.TracerC()
    R = _t(small_grid(), gpu).reshape(-1)
    for chord in (False, True):
        with drrt.using(sort_rays=True, check_failed=False, chord_key=chord):
            T.trace(R, RES_S, _t(pos, gpu), _t(vel, gpu), H_S, 0.5 * H_S)
            order = _np(drrt.last_order).copy()
        check_order(order, RES_S, H_S, pos, vel, 1.0, chord, (n, "chord" if chord else "light-field"),
                    referee(RES_S, H_S, pos, vel, 1.0, chord))


# ---- one large case: stability across rocPRIM's algorithm switch -------------------------------------------------------------
N_LARGE = (1 << 20) + 4097           # above radix_sort_config<>::merge_sort_limit (the comment in csrc/drrt_sort.hip)
H_L, SIDE = 2.96, 64                 # 5 x 4 x 3 voxels of 2.96: the largest extent, 11.84, is that of the host tier's 33^3 grid


@functools.lru_cache(maxsize=None)
def large_rays():
    """N_LARGE rays drawn with repetition from the 4096 rays of the aligned 64 x 64 plane source (pixel centres, collimated
    along +z): about 256 copies of every key, scattered over the whole array."""
    E = float(np.float32(RES_S[0] - 1) * np.float32(H_L))
    i, j = (v.ravel() for v in np.meshgrid(np.arange(SIDE), np.arange(SIDE), indexing="ij"))
    pos = np.stack([(i + 0.5) * E / SIDE, (j + 0.5) * E / SIDE, np.zeros(SIDE * SIDE)], -1).astype(np.float32)
    pick = np.random.default_rng(20).integers(0, SIDE * SIDE, N_LARGE)
    vel = np.zeros((N_LARGE, 3), np.float32)
    vel[:, 2] = 1.0
    return np.ascontiguousarray(pos[pick]), vel, pick


def test_stable_above_the_merge_sort_limit(gpu):
    """n = 2^20 + 4097: rocPRIM sorts this many pairs with another algorithm than the smaller calls.  4096 distinct keys,
    about 256 rays each: the order must still be the STABLE argsort -- exact equality, the only place where stability
    across the algorithm switch is seen.  The march is a few steps (ds = 1.7 h on 5 x 4 x 3 voxels)."""
    from adjointnonlinearraytracing_amd import drrt
    pos, vel, pick = large_rays()
    T = drrt.TracerC()
    R = _t(small_grid(), gpu).reshape(-1)
    P, V = _t(pos, gpu), _t(vel, gpu)
    for chord in (False, True):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with drrt.using(sort_rays=True, check_failed=False, chord_key=chord):
            T.trace(R, RES_S, P, V, H_L, 1.7 * H_L)
            order = _np(drrt.last_order).copy()
        print(f"large case, {'chord' if chord else 'light-field'} key: trace + order read-back {time.perf_counter() - t0:.3f} s")
        keys, want = expected_order(RES_S, H_L, pos, vel, 1.0, chord)
        if not chord:
            assert len(np.unique(keys)) == SIDE * SIDE and np.bincount(pick).min() > 150      # every key, many times over
        assert order.shape == (N_LARGE,) and np.array_equal(order, want.astype(np.int32)), \
            ("chord" if chord else "light-field", int((order != want).sum()))
