"""The progress block of the depth-chunked adjoint (drrt_backtrace_chunk_f32 / TracerC.backtrace_chunked, include/drrt_hip.h)
and what dist.SlabReducer builds on it, checked against evidence other than the block itself: snapshots of the running
gradient taken behind every chunk, the CPU oracle's per-ray step counts, and the exit velocities.

Grid (D, H, W) = (9, 17, 13) -- no two extents equal, so swapped axes show --, ds = h / 2 (68 adjoint iterations), 2003 rays
(neither a multiple of the wave nor of any block size: the tails are populated).  The adjoint is started directly from crafted
exit rays: a tilted plane of rays just beyond the face they left through, for every travel axis and both directions, so
negative and positive floats both go through the order-preserving key map in the position, velocity and sample boxes.

The rays are slow on purpose (|v| = cells / 24 along the travel axis: a crossing takes 48 of the 68 iterations whatever the
axis), so that with 8 chunks most planes are declared final while rays still march -- `test_plans_hold_on_the_cpu` checks
that estimate, and the parameters of the turning-ray cases, without a GPU."""
import numpy as np
import pytest
import torch

import cases

D_, H_, W_ = 9, 17, 13
RES = (W_, H_, D_)                       # the library's res = (W, H, D); the arrays are [z, y, x]
H = 1.0 / 16
DS = H / 2
N_RAYS = 2003
EXT = np.array([(W_ - 1) * H, (H_ - 1) * H, (D_ - 1) * H])
N_AX = {0: W_, 1: H_, 2: D_}
TOTAL = int(np.float32(2.0) * np.float32(H) * np.float32(max(RES)) / np.float32(DS))     # src/tracer.cpp:417
AXES = [(axis, sign) for axis in (0, 1, 2) for sign in (+1, -1)]
# turning rays (n = 1 + a * t along the travel axis): a, the axial and the transverse exit velocity per travel axis; chosen
# with _reverse_march64 (test_plans_hold_on_the_cpu states what they were chosen for)
TURN = {2: dict(a=0.8, v_ax=0.9, v_tr=0.1), 1: dict(a=0.6, v_ax=0.8, v_tr=0.1)}


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@pytest.fixture(scope="module")
def drrt_mod(gpu):
    from adjointnonlinearraytracing_amd import drrt
    drrt.options.check_failed = False
    return drrt


def _bounds(K):
    K = max(1, min(K, TOTAL))
    return [TOTAL * k // K for k in range(K + 1)]


def _field(kind="smooth"):
    if kind == "uniform":
        return cases.uniform((D_, H_, W_))
    # a weak field: the slow rays keep their heading (|dv| over a crossing stays well below their speed)
    return np.ascontiguousarray(cases.smooth_field(17, seed=3, amp=0.02)[:D_, :, :W_])


def _linear_field(axis, a):
    z, y, x = np.meshgrid(np.arange(D_) * H, np.arange(H_) * H, np.arange(W_) * H, indexing="ij")
    return (1.0 + a * (x, y, z)[axis]).astype(np.float32)


def _speed(axis):
    return (N_AX[axis] - 1) / 24.0


def _exit_rays(axis, sign, n=N_RAYS, tilt=0.08, seed=0):
    """Exit rays of a tilted plane source that travelled along `sign` * axis: just beyond the face they left through (0.3 of
    a step, away from ties of the termination test), transverse velocity components of both signs."""
    rng = np.random.default_rng(40 + 2 * axis + (sign < 0) + 10 * seed)
    s = _speed(axis)
    xt = rng.uniform(0.1, 0.9, (n, 3)) * EXT
    vt = rng.normal(0.0, tilt, (n, 3)) * s
    vt[:, axis] = sign * s
    xt[:, axis] = (EXT[axis] if sign > 0 else 0.0) + sign * 0.3 * DS * s
    dx, dv = rng.normal(size=(n, 3)), rng.normal(size=(n, 3))
    return tuple(a.astype(np.float32) for a in (xt, vt, dx, dv))


def _turning_rays(axis, n=1501, seed=0):
    """Obliquely incident exit rays beyond the far face of `axis`, for the field 1 + a * t: the reverse march decelerates
    them along the axis until they turn and leave through the face they started at."""
    p = TURN[axis]
    tr = (axis + 2) % 3                                      # z -> y, y -> x: the transverse axis the rays lean along
    rng = np.random.default_rng(70 + axis + 10 * seed)
    xt = rng.uniform(0.15, 0.85, (n, 3)) * EXT
    xt[:, tr] = rng.uniform(0.35, 0.65, n) * EXT[tr]
    vt = rng.normal(0.0, 0.01, (n, 3))
    vt[:, axis] = p["v_ax"] * (1.0 + rng.uniform(-0.02, 0.02, n))
    vt[:, tr] = p["v_tr"] * rng.choice([-1.0, 1.0], n)      # both signs: only the travel axis has all rays heading one way
    xt[:, axis] = EXT[axis] + 0.3 * DS * p["v_ax"]
    dx, dv = rng.normal(size=(n, 3)), rng.normal(size=(n, 3))
    return tuple(a.astype(np.float32) for a in (xt, vt, dx, dv))


def _reverse_march64(oracle, rif, xt, vt, iters):
    """The adjoint march's ray states in float64 (src/tracer.cpp:420-425): per iteration (x, v, active) of every ray."""
    x, v = xt.astype(np.float64), vt.astype(np.float64)
    esc = lambda p, w: (((p < 0) & (w < 0)) | ((p >= EXT) & (w > 0))).any(axis=1)
    active = ~esc(x, -v)
    ones, out = np.ones(len(x), np.uint8), []
    for _ in range(iters):
        x = x - DS * v
        n, g = oracle.eval_grad(rif, RES, H, x, mask=ones, dtype=np.float64)
        v = v - DS * n[:, None] * g
        active = active & ~esc(x, -v)
        out.append((x, v, active))
    return out


def _final_planes(p, a):
    """The planes of grid axis `a` that dist.SlabReducer.after_chunk takes for final from one progress block, as a range."""
    n = N_AX[a]
    if p["active"] == 0:
        return range(0, n)
    if p["vel_min"][a] > 0.0:
        return range(min(n, max(0, int(p["pos_max"][a] / H) + 2)), n)
    if p["vel_max"][a] < 0.0:
        return range(0, max(-1, min(n - 1, int(p["pos_min"][a] / H) - 1)) + 1)
    return range(0)


def _plane_index(a, planes):
    idx = [slice(None)] * 3
    idx[2 - a] = slice(planes.start, planes.stop)
    return tuple(idx)


# ---- CPU: the plans the GPU cases rest on ---------------------------------------------------------------------------------
def _straight_line_final(axis, sign, K):
    """Planes of `axis` final before the last chunk that still has marching rays, by the straight-line estimate (a ray moves
    ds * |v| per iteration): -> (planes, of)."""
    xt, vt, _, _ = _exit_rays(axis, sign)
    b = _bounds(K)
    x0, va = xt[:, axis].astype(np.float64), vt[:, axis].astype(np.float64)
    best = 0
    for k in range(K):
        x = x0 - b[k + 1] * DS * va
        if ((x < 0) | (x >= EXT[axis])).all():               # every ray has crossed: chunk k is the last that marches
            break
        p = dict(active=1, vel_min=[va.min()] * 3, vel_max=[va.max()] * 3, pos_min=[x.min()] * 3, pos_max=[x.max()] * 3)
        best = len(_final_planes(p, axis))
    return best, N_AX[axis]


def test_plans_hold_on_the_cpu(oracle):
    # 8 chunks: a third of the travel axis is final while rays still march, with two planes to spare
    assert 30 <= TOTAL <= 80
    for axis, sign in AXES:
        got, of = _straight_line_final(axis, sign, 8)
        print(f"straight-line estimate axis {'xyz'[axis]}{'+' if sign > 0 else '-'}: {got} of {of} planes final early")
        assert got >= of / 3.0 + 2, (axis, sign, got)
    # turning rays: at one chunk boundary of K = 8 every ray still heads down the axis and >= 3 planes are handed in (one to
    # spare); later the rays come back >= 3 planes into them (one to spare); all have left before the iterations run out
    b = _bounds(8)
    for axis, p in TURN.items():
        xt, vt, _, _ = _turning_rays(axis)
        states = _reverse_march64(oracle, _linear_field(axis, p["a"]), xt, vt, TOTAL)
        handed, first = 0, None
        for k in range(8):
            x, v, act = states[b[k + 1] - 1]
            if not act.all() or v[:, axis].min() <= 0.05:
                break
            first = int(x[:, axis].max() / H) + 2           # (the block holds the NEXT sample: never a larger bound)
            handed, at = N_AX[axis] - first, k
        back = max(int(np.floor(x[act, axis].max() / H)) + 1 for x, v, act in states[b[at + 1]:] if act.any())
        back = min(back, N_AX[axis] - 1) - first + 1
        left = max(i for i, s in enumerate(states) if s[2].any()) + 1
        angle = float(np.degrees(np.arctan2(p["v_tr"], p["v_ax"])))
        print(f"turning rays axis {'xyz'[axis]}: a = {p['a']}, incidence {angle:.1f} deg, K = 8: {handed} planes handed in "
              f"after chunk {at}, rays return {back} planes into them, all gone after {left} of {TOTAL} iterations")
        assert handed >= 4 and back >= 4 and left <= TOTAL - 4, (axis, handed, back, left)


# ---- GPU: the progress block against snapshots, step counts and exit velocities ------------------------------------------
_ref_cache = {}


def _reference(oracle, kind, axis, sign):
    """Oracle adjoint (the kernels' fp32 operation sequence) of a case, with per-ray contributing-step counts; computed once."""
    key = (kind, axis, sign)
    if key not in _ref_cache:
        rif = _field(kind)
        xt, vt, dx, dv = _exit_rays(axis, sign)
        with oracle.arith("factored"), oracle.trajectory_signatures(len(xt)) as ts:
            ob = oracle.backtrace(rif, RES, xt, vt, dx, dv, H, DS, dtype=np.float32)
        _ref_cache[key] = dict(rif=rif, rays=(xt, vt, dx, dv), grad=ob["grad"], steps_total=ob["steps_total"],
                               steps=ts.steps.copy())
    return _ref_cache[key]


def _run_chunked(drrt_mod, gpu, ref, K):
    snaps, blocks = [], []

    def on_chunk(k, grad, progress):
        snaps.append(grad.clone())                           # queued behind chunk k on the march's stream
        blocks.append(progress)

    xt, vt, dx, dv = (_t(a, gpu) for a in ref["rays"])
    g = drrt_mod.TracerC().backtrace_chunked(_t(ref["rif"], gpu), RES, xt, vt, dx, dv, H, DS, chunks=K, on_chunk=on_chunk)
    st = drrt_mod.read_stats()
    progs = [drrt_mod.decode_chunk_progress(p) for p in blocks]
    snaps = [s.cpu().view(D_, H_, W_) for s in snaps]
    return g.cpu().view(D_, H_, W_), st, snaps, progs


@pytest.mark.gpu
@pytest.mark.parametrize("K", [3, 8])
@pytest.mark.parametrize("axis,sign", AXES)
def test_progress_block_against_snapshots_and_step_counts(gpu, oracle, drrt_mod, axis, sign, K):
    ref = _reference(oracle, "smooth", axis, sign)
    final, st, snaps, progs = _run_chunked(drrt_mod, gpu, ref, K)
    # 1. the gradient: validates the snapshots the other checks use as evidence
    assert st["ray_steps"] == ref["steps_total"]
    assert cases.rel_l2(final.numpy(), ref["grad"]) <= 2e-5
    _check_blocks(ref, final, snaps, progs, K, axis, sign)


def _check_blocks(ref, final, snaps, progs, K, axis, sign):
    b = _bounds(K)
    assert len(snaps) == len(progs) == K
    assert torch.equal(snaps[-1], final)
    slack = [0, 0]
    prev = torch.zeros_like(final)
    for k, (snap, p) in enumerate(zip(snaps, progs)):
        delta = (snap != prev)
        prev = snap
        if not delta.any():
            assert p["sample_min"] is None and p["sample_max"] is None, (k, p)
            continue
        assert p["sample_min"] is not None, k
        for a in range(3):
            touched = torch.nonzero(delta.any(dim=tuple(d for d in range(3) if d != 2 - a))).flatten()
            lo, hi = int(touched.min()), int(touched.max())
            b_lo, b_hi = int(np.floor(p["sample_min"][a] / H)), int(np.floor(p["sample_max"][a] / H)) + 1
            # 2. sound: every voxel the chunk changed lies in the planes the sample box names (include/drrt_hip.h:347-349)
            assert b_lo <= lo and hi <= b_hi, (k, a, (lo, hi), (b_lo, b_hi), p)
            # 3. tight: at most one plane beyond what the chunk changed (the clamped tap at a face, an empty upper tap)
            assert lo - b_lo <= 1 and b_hi - hi <= 1, (k, a, (lo, hi), (b_lo, b_hi), p)
            slack = [max(slack[0], lo - b_lo), max(slack[1], b_hi - hi)]
    # 4. finality: what the reducer's rule takes for final after chunk k never changes again
    early = 0
    marching = [k for k, p in enumerate(progs) if p["active"]]
    for k, (snap, p) in enumerate(zip(snaps, progs)):
        planes = _final_planes(p, axis)
        idx = _plane_index(axis, planes)
        assert torch.equal(snap[idx], final[idx]), (k, planes)
        if marching and k <= marching[-1]:
            early = max(early, len(planes))
        for a in range(3):                                   # ... on the other axes too, whenever the rule speaks
            idx = _plane_index(a, _final_planes(p, a))
            assert torch.equal(snap[idx], final[idx]), (k, a)
    print(f"axis {'xyz'[axis]}{'+' if sign > 0 else '-'} K={K}: {early} of {N_AX[axis]} planes final while rays march; "
          f"sample-box slack {slack[0]} below / {slack[1]} above")
    if K == 8:
        assert early >= N_AX[axis] / 3.0, (early, [p["active"] for p in progs])
    # 5. the active count: a ray that still owes contributions cannot be inactive
    act = [p["active"] for p in progs]
    for k, n_act in enumerate(act):
        assert int((ref["steps"] > b[k + 1]).sum()) <= n_act <= N_RAYS, (k, n_act)
    assert all(y <= x for x, y in zip(act, act[1:])) and act[-1] == 0, act
    # the boxes of the marching rays are on the side of the key map the case aims at
    first = progs[0]
    assert first["active"] > 0 and first["vel_min"][(axis + 1) % 3] < 0.0 < first["vel_max"][(axis + 1) % 3]
    assert (first["vel_min"][axis] > 0.0) if sign > 0 else (first["vel_max"][axis] < 0.0)


@pytest.mark.gpu
@pytest.mark.parametrize("axis,sign", [(1, +1), (2, -1)])
def test_velocity_box_is_the_exit_velocities_box_in_a_uniform_medium(gpu, oracle, drrt_mod, axis, sign):
    """6. n = 1 everywhere: velocities never change, so after every chunk vel_min / vel_max are the exact minimum / maximum
    of vt over the rays still marching -- which pins the key map and its inverse for both signs, bit for bit."""
    ref = _reference(oracle, "uniform", axis, sign)
    vt = ref["rays"][1]
    for K in (3, 8):
        final, st, snaps, progs = _run_chunked(drrt_mod, gpu, ref, K)
        b = _bounds(K)
        assert st["ray_steps"] == ref["steps_total"] and cases.rel_l2(final.numpy(), ref["grad"]) <= 2e-5
        seen = 0
        for k, p in enumerate(progs):
            marching = ref["steps"] >= b[k + 1]              # contributed at the chunk's last iteration: not yet stopped
            assert p["active"] == int(marching.sum()), (K, k)
            if not marching.any():
                assert p["vel_min"] is None
                continue
            seen += 1
            assert p["vel_min"] == [float(v) for v in vt[marching].min(axis=0)], (K, k)
            assert p["vel_max"] == [float(v) for v in vt[marching].max(axis=0)], (K, k)
        assert seen >= 2


# ---- GPU: the real chunked kernel with the real SlabReducer, against a mirror rank ------------------------------------------
class _Handle:
    def __init__(self, t):
        self.ev = None
        if t.is_cuda:
            self.ev = torch.cuda.Event()
            self.ev.record(torch.cuda.current_stream(t.device))

    def wait(self):
        if self.ev is not None:
            torch.cuda.current_stream().wait_event(self.ev)


class _MirrorRank:
    """Stand-in for torch.distributed inside dist.py: a second rank that holds exactly what this one holds.  all_reduce(SUM)
    doubles the tensor in place on the current stream, all_reduce(MAX) leaves it; the handle's wait() orders the current
    stream behind the operation, as a collective's does."""
    ReduceOp = torch.distributed.ReduceOp

    def is_initialized(self):
        return True

    def get_world_size(self, group=None):
        return 2

    def get_backend(self, group=None):
        return "gloo"

    def all_reduce(self, t, op=torch.distributed.ReduceOp.SUM, group=None, async_op=False):
        if op == self.ReduceOp.SUM:
            t.mul_(2.0)
        return _Handle(t)


def _overlapped_with_mirror(gpu, rif, rays, chunks=8):
    """-> (grid of backtrace_allreduce_overlapped with a mirror rank, the SlabReducer it used, voxels handed in early)."""
    from adjointnonlinearraytracing_amd import dist as DD
    made = []

    class Recording(DD.SlabReducer):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            made.append(self)

        def after_chunk(self, progress, *a, **kw):
            super().after_chunk(progress, *a, **kw)
            if progress["active"]:                           # handed in while rays still march (not: once all have left)
                self.early_marching = sum(int(buf.numel()) for _, buf, _ in self.parts)

        def finish(self, *a, **kw):
            self.early = sum(int(buf.numel()) for _, buf, _ in self.parts)
            return super().finish(*a, **kw)

    xt, vt, dx, dv = (_t(a, gpu) for a in rays)
    real_dist, real_red = DD.dist, DD.SlabReducer
    DD.dist, DD.SlabReducer = _MirrorRank(), Recording
    try:
        g = DD.backtrace_allreduce_overlapped(_t(rif, gpu).reshape(-1), RES, xt, vt, dx, dv, H, DS, chunks=chunks)
        torch.cuda.synchronize()
    finally:
        DD.dist, DD.SlabReducer = real_dist, real_red
    assert len(made) == 1
    return g.cpu().numpy(), made[0], made[0].early


@pytest.mark.gpu
@pytest.mark.parametrize("axis", [2, 1])
def test_overlapped_reduce_of_a_plane_source_with_a_mirror_rank(gpu, drrt_mod, axis):
    """The side stream, the event wait, the packed slabs and the copy-back for real: twice the one-launch gradient, most of
    it handed in while rays still march (a plane reduced twice would be off by a factor of 2)."""
    rif = _field("smooth")
    rays = _exit_rays(axis, +1)
    one = drrt_mod.TracerC().backtrace(_t(rif, gpu), RES, *(_t(a, gpu) for a in rays), H, DS).cpu().numpy()
    g, red, early = _overlapped_with_mirror(gpu, rif, rays)
    assert red.on and not red.violated and red.choice == (axis, True), (red.choice, red.violated)
    assert red.early_marching >= D_ * H_ * W_ / 3.0, (red.early_marching, early)
    assert cases.rel_l2(g, 2.0 * one) <= 2e-5


@pytest.mark.gpu
@pytest.mark.parametrize("axis", [2, 1])
def test_overlapped_reduce_of_turning_rays_with_a_mirror_rank(gpu, drrt_mod, axis):
    """Rays that turn around and come back into planes already handed in: noticed (`violated`), the slab results dropped,
    and the whole grid reduced exactly once -- on z the packed slab used to be the grid itself, reduced twice."""
    rif = _linear_field(axis, TURN[axis]["a"])
    rays = _turning_rays(axis)
    one = drrt_mod.TracerC().backtrace(_t(rif, gpu), RES, *(_t(a, gpu) for a in rays), H, DS).cpu().numpy()
    g, red, early = _overlapped_with_mirror(gpu, rif, rays)
    assert red.choice == (axis, True) and red.violated and early > 0, (red.choice, red.violated, early)
    assert cases.rel_l2(g, 2.0 * one) <= 2e-5


# ---- GPU: ray sets too small to sort ---------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("sort", [True, False])
@pytest.mark.parametrize("n", [0, 1, 2, 65])
def test_chunked_adjoint_of_small_sets(gpu, drrt_mod, n, sort):
    """n < 2 rays are not sorted, so no order is left behind for the resumed chunks: they must neither be refused nor
    visit the rays in an earlier call's order."""
    from adjointnonlinearraytracing_amd import _lib
    rif = _t(_field("smooth"), gpu)
    T = drrt_mod.TracerC()
    drrt_mod.options.sort_rays = sort
    try:
        # an earlier, larger call leaves its order behind in the workspace
        T.backtrace(rif, RES, *(_t(a, gpu) for a in _exit_rays(0, +1, n=300)), H, DS)
        rays = [_t(a[:n], gpu) for a in _exit_rays(1, +1, n=max(n, 1), seed=1)]
        one = T.backtrace(rif, RES, *rays, H, DS)
        seen = []
        g = T.backtrace_chunked(rif, RES, *rays, H, DS, chunks=3,
                                on_chunk=lambda k, grad, prog: seen.append(drrt_mod.decode_chunk_progress(prog)))
        assert _lib.load().drrt_order_hint_pending() == 0
        assert len(seen) == 3 and seen[-1]["active"] == 0
        if n == 0:
            assert float(g.abs().max()) == 0.0 and all(p["active"] == 0 and p["sample_min"] is None for p in seen)
        else:
            assert float(one.abs().max()) > 0.0
            assert cases.rel_l2(g.cpu().numpy(), one.cpu().numpy()) <= 2e-5
    finally:
        drrt_mod.options.sort_rays = True
