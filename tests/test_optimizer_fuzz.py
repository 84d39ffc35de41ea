"""Float64-refereed fuzz of the two kernels that carry the optimisation loop, k_upres and k_adam_masked
(csrc/drrt_ops.hip, driven by optimizer.py), against the numpy restatements of oracle/optim_ref.py.

CPU tier (unmarked): pins the restatements -- `upres` to the recorded runs of tests/golden/upres.npz, its linspace to
torch.linspace bit for bit, `adam_step` to torch.optim.Adam in float64 with the reference's literal mask and clamp.

GPU tier: every comparison is per element, none against a norm of the array.

k_upres accumulates its eight products in double and rounds once, so it must be within 0.51 fp32 ulp of the float64
value (floor: the smallest fp32 subnormal); the sources mix magnitudes from 1e-30 to 1e30 and both signs.
Its sample points must be torch.linspace's to the last bit: where a point lands on a source node, x one float64 ulp
short of it flips `floor` and takes 1e-16 of the neighbouring voxel instead of none -- an error relative to the
neighbours (1e30 here), not to the result.  Destination sides with inexact steps (50, 94) reach that.

k_adam_masked must satisfy  |kernel - float64| <= C * eps_fp32 * S  per element, S the first-order error scale
optim_ref.adam_step returns with each output.  Each C is twice the worst ratio of the REFERENCE PATH -- torch's own
fp32 statements (`grad[mask] = 0`, torch.optim.Adam.step(), `clamp_`) on the same device and inputs --, rounded up to a
tidy number; the kernel's own ratio is recorded next to it and never sets the constant."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest
import torch

from oracle import optim_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EPS = R.EPS32
SUB = R.SUBNORMAL32

# C of each Adam output: twice the reference path's largest err / (eps_fp32 S) over the single-step cases below, rounded
# up; after each, that figure as measured on an MI355X: [torch's fp32 statements, k_adam_masked].  The kernel's figures
# over the trajectory, param-group and checkpoint tests are below these (p <= 0.481, m <= 0.406, v <= 0.352).
C_P = 1.0          # parameter      [0.498, 0.498]
C_M = 1.0          # first moment   [0.442, 0.442]
C_V = 1.0          # second moment  [0.363, 0.363]
C_OF = {"p": C_P, "m": C_M, "v": C_V}

BETAS = [(0.9, 0.999), (0.0, 0.0), (0.5, 0.999999)]


def _ulp32(x):
    """The fp32 spacing at |x| (x float64), 2^-149 in the subnormal range and at 0."""
    _, e = np.frexp(np.abs(x))
    return np.ldexp(1.0, np.where(x == 0, -149, np.maximum(e - 24, -149)))


def _check_ulp(name, got, ref, ulps=0.51):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    err, tol = np.abs(got - ref), np.maximum(ulps * _ulp32(ref), SUB)
    bad = ~(err <= tol)
    worst = float((err / _ulp32(ref)).max()) if err.size else 0.0
    print(f"\n[optimizer fuzz] {name}: max err = {worst:.3g} fp32 ulp")
    assert not bad.any(), f"{name}: {int(bad.sum())} of {bad.size} elements off by up to {worst:.3g} ulp, first at " \
                          f"{tuple(np.argwhere(bad)[0])}"


def _mixed(rng, shape, lo=-30.0, hi=30.0):
    """fp32 values of both signs with magnitudes log-uniform in 10^[lo, hi]."""
    return (rng.choice([-1.0, 1.0], shape) * 10.0 ** rng.uniform(lo, hi, shape)).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------
# CPU tier: the restatements themselves
# ---------------------------------------------------------------------------------------------------------------------

def test_ref_upres_matches_recorded_reference_runs():
    """optim_ref.upres against the three runs of the reference's upres_scene in upres.npz (float64, rounded once to
    fp32): within 0.51 fp32 ulp at |ref| per element."""
    z = np.load(os.path.join(GOLDEN, "upres.npz"))
    for tag in ("a", "b", "c"):
        src, dst = z[f"{tag}_src"], z[f"{tag}_dst"]
        _check_ulp(f"restatement vs recorded run {tag} {src.shape[0]}->{dst.shape[0]}", dst, R.upres(src, dst.shape))


def _same_bits(a, b):
    return a.dtype == b.dtype == np.float64 and np.array_equal(a.view(np.int64), b.view(np.int64))


def test_ref_linspace_is_torchs_bit_for_bit():
    """optim_ref.linspace01 against torch.linspace(0, 1, s, dtype=float64), s = 1..40.  torch rounds the upper half's
    1 - step * (s - 1 - i) once (a contracted multiply-add); the form with two roundings differs from s = 16 on."""
    for s in range(1, 41):
        assert _same_bits(R.linspace01(s), torch.linspace(0, 1, s, dtype=torch.float64).numpy()), s


@pytest.mark.gpu
def test_ref_linspace_is_torchs_bit_for_bit_on_the_device(gpu):
    """The reference builds its sample points with torch.linspace on the volume's device, in float64."""
    for s in range(1, 41):
        want = torch.linspace(0, 1, s, dtype=torch.float64, device=gpu).cpu().numpy()
        assert _same_bits(R.linspace01(s), want), s


@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 5, 7), (2, 2, 2), (3, 3, 3), (4, 6, 5)])
def test_ref_adam_matches_torch_float64(shape):
    """optim_ref.adam_step against torch.optim.Adam on float64 parameters with the reference's literal mask and clamp
    statements, 8 free-running steps: 1e-12 relative per element."""
    rng = np.random.default_rng(11)
    worst = 0.0
    for betas, wd, eps in itertools.product(BETAS, (0.0, 0.01), (1e-8, 1e-3)):
        p0 = 0.9 + 0.5 * rng.random(shape)
        n = torch.from_numpy(p0.copy()).requires_grad_(True)
        opto = torch.optim.Adam([n], lr=3e-2, betas=betas, eps=eps, weight_decay=wd)
        mask = torch.ones_like(n, dtype=torch.bool)
        mask[1:-1, 1:-1, 1:-1] = 0
        p, m, v = p0, np.zeros(shape), np.zeros(shape)
        for k in range(8):
            g = rng.normal(size=shape) * 10.0 ** rng.integers(-3, 3)
            n.grad = torch.from_numpy(g.copy())
            with torch.no_grad():
                n.grad[mask] = 0
            opto.step()
            with torch.no_grad():
                n.clamp_(min=1)
            (p, gm, m, v), _ = R.adam_step(p, g, m, v, k + 1, 3e-2, betas, eps, wd, True, 1.0)
            st = opto.state[n]
            for name, got, want in (("p", p, n.detach().numpy()), ("g", gm, n.grad.numpy()),
                                    ("m", m, st["exp_avg"].numpy()), ("v", v, st["exp_avg_sq"].numpy())):
                err = np.abs(got - want)
                assert (err <= 1e-12 * np.abs(want)).all(), (name, betas, wd, eps, k, float((err / np.abs(want)).max()))
                worst = max(worst, float(np.where(want != 0, err / np.where(want != 0, np.abs(want), 1.0), 0.0).max()))
    print(f"\n[optimizer fuzz] adam_step vs torch float64 {shape}: max relative difference {worst:.3g}")


def test_ref_adam_scales_cover_cancelling_weight_decay():
    """Where wd * p cancels g, the scale keeps |g| + wd |p|: it does not shrink with the result."""
    p, g = np.full((1, 1, 1), 2.0), np.full((1, 1, 1), -0.02)
    (p2, gm, m2, v2), (Sp, Sg, Sm, Sv) = R.adam_step(p, g, 0 * p, 0 * p, 1, 1e-2, (0.9, 0.999), 1e-8, 0.01, False, None)
    assert abs(m2[0, 0, 0]) <= 1e-17 and Sm[0, 0, 0] >= 0.1 * 0.04 and Sg[0, 0, 0] == 0.0 and np.isfinite(Sp).all()
    # eps = 0 on zero state: the denominator is undetermined, the parameter scale says so
    (_, _, _, _), (Sp, _, _, _) = R.adam_step(p, 0 * g, 0 * p, 0 * p, 1, 1e-2, (0.9, 0.999), 0.0, 0.0, False, None)
    assert np.isinf(Sp).all()


# ---------------------------------------------------------------------------------------------------------------------
# GPU tier: k_upres
# ---------------------------------------------------------------------------------------------------------------------

def _c_upres(gpu, src, dst_shape):
    """drrt_upres_volume_f32 itself (upres_scene only asks for cubes)."""
    from adjointnonlinearraytracing_amd import _lib
    s = torch.from_numpy(np.ascontiguousarray(src, dtype=np.float32)).to(gpu)
    d = torch.empty(tuple(dst_shape), dtype=torch.float32, device=gpu)
    _lib.check(_lib.load().drrt_upres_volume_f32(_lib._p(s), (C.c_int * 3)(*s.shape), _lib._p(d),
                                                 (C.c_int * 3)(*dst_shape), _lib._stream(gpu)))
    return d.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("r,s", [(1, 1), (1, 5), (2, 2), (2, 7), (5, 1), (5, 2), (5, 5), (9, 17), (17, 24), (24, 7),
                                 (33, 129), (3, 50), (5, 50), (8, 50), (7, 94)])
def test_upres_edge_shapes(gpu, r, s):
    """Sides 1 and 2, identity (bit for bit), down-sampling, ragged last blocks (7^3, 129^3), magnitudes from 1e-30 to
    1e30: within 0.51 fp32 ulp of the float64 value at every voxel.  s = 1 samples x = 0 (torch.linspace's one-step
    case): the first corner.  The sides 50 and 94 have inexact steps whose points land on source nodes: there the
    last bit of x decides `floor`, and a point one float64 ulp short of a node takes weight 1 - 1e-16 of the node and
    1e-16 of its neighbour -- 1e14 next to a 1e-30 node.  So the kernel's x must be torch.linspace's bit for bit: the
    upper half as `step * idx` fails at all four, the upper half rounded twice (not fused) at 8 -> 50."""
    from adjointnonlinearraytracing_amd import optimizer
    rng = np.random.default_rng(1000 * r + s)
    src = _mixed(rng, (r, r, r))
    out = optimizer.upres_scene(torch.from_numpy(src).to(gpu), s)
    assert out.shape == (s, s, s) and out.dtype == torch.float32
    got = out.cpu().numpy()
    _check_ulp(f"upres {r}->{s}", got, R.upres(src, (s, s, s)))
    if s == r:
        assert np.array_equal(got.view(np.uint32), src.view(np.uint32))
    if s == 1:
        assert got.view(np.uint32)[0, 0, 0] == src.view(np.uint32)[0, 0, 0]


@pytest.mark.gpu
@pytest.mark.parametrize("dst", [(1, 6, 13), (13, 1, 6), (6, 13, 1), (4, 300, 3)])
def test_upres_non_cubic_destination(gpu, dst):
    """The C entry with three different destination sides (size-1 axes included): axes swapped in the index
    decomposition, or a side taken from the wrong axis, cannot pass."""
    rng = np.random.default_rng(sum(dst))
    src = _mixed(rng, (5, 5, 5))
    _check_ulp(f"upres 5^3 -> {dst}", _c_upres(gpu, src, dst), R.upres(src, dst))


@pytest.mark.gpu
def test_upres_scene_input_handling(gpu):
    from adjointnonlinearraytracing_amd import optimizer
    rng = np.random.default_rng(3)
    src = _mixed(rng, (6, 6, 6), -4.0, 4.0)                              # inside fp16's range
    x = torch.from_numpy(src).to(gpu)
    base = optimizer.upres_scene(x, 11)
    _check_ulp("upres 6->11", base.cpu().numpy(), R.upres(src, (11,) * 3))
    # a permuted view is resampled as its contiguous copy
    view = x.permute(2, 0, 1)
    assert not view.is_contiguous()
    assert torch.equal(optimizer.upres_scene(view, 11), optimizer.upres_scene(view.contiguous(), 11))
    _check_ulp("upres of a permuted view", optimizer.upres_scene(view, 11).cpu().numpy(),
               R.upres(src.transpose(2, 0, 1), (11,) * 3))
    # other dtypes: the source narrowed (or widened) to fp32, the fp32 result cast back once
    for dt in (torch.float64, torch.float16, torch.bfloat16):
        xin = x.to(dt)
        out = optimizer.upres_scene(xin, 11)
        assert out.dtype == dt and out.shape == (11, 11, 11)
        mid = optimizer.upres_scene(xin.to(torch.float32), 11)
        _check_ulp(f"upres of a {dt} source", mid.cpu().numpy(),
                   R.upres(xin.to(torch.float32).cpu().numpy(), (11,) * 3))
        assert torch.equal(out, mid.to(dt))
    # 2-D and 4-D inputs are refused before anything is allocated
    for bad in (torch.zeros(4, 4, device=gpu), torch.zeros(2, 2, 2, 2, device=gpu)):
        before = torch.cuda.memory_stats(gpu)["allocation.all.allocated"]
        with pytest.raises(RuntimeError, match="3-D"):
            optimizer.upres_scene(bad, 4096)
        assert torch.cuda.memory_stats(gpu)["allocation.all.allocated"] == before


# ---------------------------------------------------------------------------------------------------------------------
# GPU tier: k_adam_masked
# ---------------------------------------------------------------------------------------------------------------------

def _c_adam(gpu, p, g, m, v, step, lr, betas, eps, wd, mask_boundary, clamp_min):
    """drrt_adam_step_f32 on fp32 arrays -> (p', g', m', v') as fp32 numpy arrays."""
    from adjointnonlinearraytracing_amd import _lib
    t = [torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(gpu) for a in (p, g, m, v)]
    flags = (_lib.ADAM_MASK_BOUNDARY if mask_boundary else 0) | (_lib.ADAM_CLAMP_MIN if clamp_min is not None else 0)
    _lib.check(_lib.load().drrt_adam_step_f32(*[_lib._p(a) for a in t], (C.c_int * 3)(*p.shape), float(step), float(lr),
                                              float(betas[0]), float(betas[1]), float(eps), float(wd),
                                              float(clamp_min if clamp_min is not None else 0.0), flags,
                                              _lib._stream(gpu)))
    return tuple(a.cpu().numpy() for a in t)


def _torch_adam(gpu, p, g, m, v, step, lr, betas, eps, wd, mask_boundary, clamp_min):
    """The reference path: the loop's three statements run by torch in fp32 on the device, from the same state."""
    P, G, M, V = (torch.from_numpy(np.array(a, dtype=np.float32)).to(gpu) for a in (p, g, m, v))
    P.requires_grad_(True)
    P.grad = G
    opto = torch.optim.Adam([P], lr=lr, betas=betas, eps=eps, weight_decay=wd)
    opto.state[P] = {"step": torch.tensor(float(step - 1)), "exp_avg": M, "exp_avg_sq": V}
    with torch.no_grad():
        if mask_boundary:
            mask = torch.ones_like(P, dtype=torch.bool)
            mask[1:-1, 1:-1, 1:-1] = 0
            P.grad[mask] = 0
    opto.step()
    with torch.no_grad():
        if clamp_min is not None:
            P.clamp_(min=clamp_min)
    st = opto.state[P]
    return tuple(a.detach().cpu().numpy() for a in (P, P.grad, st["exp_avg"], st["exp_avg_sq"]))


class _Worst:
    """Largest err / (eps_fp32 S) per output, over the cases of one test."""

    def __init__(self, path):
        self.path, self.ratio, self.where = path, {"p": 0.0, "m": 0.0, "v": 0.0}, {}

    def add(self, case, got, ref, scales):
        """got, ref: (p', g', m', v').  The masked gradient is exact.  An output is judged where its scale and its
        float64 value are finite (they are not where the state holds planted non-finite values or the denominator is
        undetermined); there a non-finite kernel value counts as an infinite error."""
        assert np.array_equal(got[1].astype(np.float64), ref[1]), f"{self.path} {case}: the gradient is not the masked input"
        for name, a, b, S in (("p", got[0], ref[0], scales[0]), ("m", got[2], ref[2], scales[2]),
                              ("v", got[3], ref[3], scales[3])):
            keep = np.isfinite(S) & np.isfinite(b)
            with np.errstate(all="ignore"):
                err = np.where(np.isfinite(a), np.abs(a.astype(np.float64) - b), np.inf)
                ratio = np.where(keep, err / (EPS * S), 0.0)
            if ratio.size and float(ratio.max()) > self.ratio[name]:
                self.ratio[name], self.where[name] = float(ratio.max()), (case, tuple(np.argwhere(ratio == ratio.max())[0]))

    def report(self, test):
        print(f"\n[optimizer fuzz] {test} {self.path}: max err / (eps S): " +
              ", ".join(f"{k} = {self.ratio[k]:.3g}" for k in "pmv"))

    def check(self):
        for k in "pmv":
            assert self.ratio[k] <= C_OF[k], f"{self.path}: {k} off by {self.ratio[k]:.3g} eps S > C = {C_OF[k]} at " \
                                             f"{self.where[k]}"


def _adam_state(rng, shape, zero_fraction=0.1):
    """A parameter around the clamp values, a state as after reload_opto (moments not zero), gradients from 1e-30 to
    1e15 -- and voxels where gradient and state are exactly zero."""
    p = rng.uniform(0.8, 1.5, shape).astype(np.float32)
    g = _mixed(rng, shape, -30.0, 15.0)
    m = _mixed(rng, shape, -30.0, 8.0)
    v = np.abs(_mixed(rng, shape, -30.0, 16.0))
    zero = rng.random(shape) < zero_fraction
    if zero.size > 1:
        zero.flat[rng.integers(zero.size)] = True
    for a in (g, m, v):
        a[zero] = 0.0
    return p, g, m, v, zero


HYPERS = list(itertools.product(BETAS, (1e-8, 1e-3, 0.0), (0.0, 0.01), (0.0, 3e-2), (1.0, 2.0, 1000.0, 1e6)))
FLAGS = list(itertools.product((True, False), (None, 1.0, 0.0, 1.25)))
ADAM_SHAPES = [(1, 1, 1), (1, 5, 7), (7, 1, 5), (2, 3, 300), (3, 3, 3), (20, 18, 16), (7, 9, 33)]
PER_CELL = 6          # hyper-parameter sets per (shape, flags): 7 * 8 * 6 = 336 calls walk the 144 sets more than twice


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ADAM_SHAPES)
def test_adam_single_step_from_random_state(gpu, shape):
    """One call of drrt_adam_step_f32 from a random state, every (mask_boundary, clamp_min) with six hyper-parameter
    sets each (betas, eps, weight_decay, lr, step; all 144 sets are walked over the shapes), per element against the
    float64 referee; torch's fp32 statements are measured on the same inputs."""
    order = np.random.default_rng(7).permutation(len(HYPERS))
    rng = np.random.default_rng(100 + ADAM_SHAPES.index(shape))
    kernel, ref_path = _Worst("k_adam_masked"), _Worst("torch fp32")
    for f, (mask, cmin) in enumerate(FLAGS):
        cell = ADAM_SHAPES.index(shape) * len(FLAGS) + f
        for k in range(PER_CELL):
            betas, eps, wd, lr, step = HYPERS[order[(cell * PER_CELL + k) % len(HYPERS)]]
            p, g, m, v, zero = _adam_state(rng, shape)
            args = (step, lr, betas, eps, wd, mask, cmin)
            ref, scales = R.adam_step(p, g, m, v, *args)
            got = _c_adam(gpu, p, g, m, v, *args)
            kernel.add(args, got, ref, scales)
            ref_path.add(args, _torch_adam(gpu, p, g, m, v, *args), ref, scales)
            # exactness: gradients are masked or untouched, bit for bit
            shell = R.boundary_mask(shape) if mask else np.zeros(shape, dtype=bool)
            assert np.array_equal(got[1][~shell].view(np.uint32), g[~shell].view(np.uint32)), args
            assert not got[1][shell].view(np.uint32).any(), args
            # a zero gradient on zero state does not move the parameter
            if wd == 0.0 and eps > 0.0:
                still = zero | (shell & (m == 0) & (v == 0))
                want = p if cmin is None else np.maximum(p, np.float32(cmin))
                assert np.array_equal(got[0][still].view(np.uint32), want[still].view(np.uint32)), args
            # the clamp: nothing finite ends below clamp_min; what the float64 update leaves clearly below it IS clamp_min
            if cmin is not None:
                free, fs = R.adam_step(p, g, m, v, step, lr, betas, eps, wd, mask, None)
                assert (got[0][np.isfinite(got[0])] >= np.float32(cmin)).all(), args
                with np.errstate(all="ignore"):
                    below = np.isfinite(fs[0]) & (free[0] < cmin - C_P * EPS * fs[0])
                assert (got[0][below] == np.float32(cmin)).all(), args
    kernel.report(f"single step {shape}"); ref_path.report(f"single step {shape}")
    ref_path.check()
    kernel.check()


@pytest.mark.gpu
@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_adam_zero_betas_are_exact(gpu, wd):
    """betas = (0, 0): the first moment is the effective gradient g + wd p and the second its square, each to one
    rounding -- whatever the state held (lerp_ weighs from the nearer end, so nothing of the old moment remains)."""
    rng = np.random.default_rng(21)
    shape = (7, 9, 33)
    p, g, m, v, _ = _adam_state(rng, shape)
    got = _c_adam(gpu, p, g, m, v, 3.0, 3e-2, (0.0, 0.0), 1e-8, wd, True, 1.0)
    gm = got[1]
    if wd == 0.0:
        assert np.array_equal(got[2].view(np.uint32), gm.view(np.uint32))
    else:
        ge = gm.astype(np.float64) + wd * p.astype(np.float64)
        # one rounding of the sum, and the rounding of wd itself to fp32
        assert (np.abs(got[2] - ge) <= 0.5 * _ulp32(ge) + 0.5 * EPS * wd * np.abs(p) + SUB).all()
    assert np.array_equal(got[3].view(np.uint32), (got[2] * got[2]).view(np.uint32))


def _plant(shape):
    """(array index in (p, g, m, v), voxel, value): interior and boundary voxels, one plant per voxel."""
    z, y, x = shape
    return [(1, (3, 4, 5), np.nan), (1, (3, 4, 6), np.inf), (1, (3, 4, 7), -np.inf), (1, (0, 2, 2), np.nan),
            (1, (z - 1, y - 1, x - 1), np.inf), (0, (2, 2, 2), np.nan), (0, (2, 2, 3), np.inf), (0, (2, 2, 4), -np.inf),
            (0, (0, 0, 0), np.nan), (0, (3, 0, 9), -np.inf), (2, (4, 4, 4), np.nan), (2, (4, 4, 5), np.inf),
            (2, (4, 4, 6), -np.inf), (2, (5, y - 1, 3), np.inf), (3, (5, 5, 5), np.nan), (3, (5, 5, 6), np.inf),
            (3, (6, 0, 0), np.inf)]


@pytest.mark.gpu
@pytest.mark.parametrize("betas,wd", [((0.9, 0.999), 0.0), ((0.9, 0.999), 0.01), ((0.0, 0.0), 0.0), ((0.5, 0.999999), 0.01)])
def test_adam_contains_non_finite_values(gpu, betas, wd):
    """NaN and +-Inf planted in g, p, m and v: every other voxel is bit-identical to the clean run, a NaN parameter
    stays NaN through the clamp, and which outputs are NaN / +Inf / -Inf is what torch's statements give on the device."""
    rng = np.random.default_rng(31)
    shape = (7, 9, 33)
    p, g, m, v, _ = _adam_state(rng, shape)
    args = (2.0, 3e-2, betas, 1e-8, wd, True, 1.0)
    clean = _c_adam(gpu, p, g, m, v, *args)
    dirty_in = [a.copy() for a in (p, g, m, v)]
    touched = np.zeros(shape, dtype=bool)
    for which, voxel, value in _plant(shape):
        assert not touched[voxel]
        dirty_in[which][voxel] = value
        touched[voxel] = True
    got = _c_adam(gpu, *dirty_in, *args)
    want = _torch_adam(gpu, *dirty_in, *args)
    for name, a, b, c in zip("pgmv", got, want, clean):
        assert np.array_equal(a[~touched].view(np.uint32), c[~touched].view(np.uint32)), name
        assert np.array_equal(np.isnan(a), np.isnan(b)), (name, np.argwhere(np.isnan(a) != np.isnan(b)))
        assert np.array_equal(np.isposinf(a), np.isposinf(b)) and np.array_equal(np.isneginf(a), np.isneginf(b)), name
    # planted voxels whose outputs stay finite (a masked gradient, a clamped -Inf, ...) are judged like any other
    ref, scales = R.adam_step(*dirty_in, *args)
    for name, a, b, S in (("p", got[0], ref[0], scales[0]), ("m", got[2], ref[2], scales[2]), ("v", got[3], ref[3], scales[3])):
        keep = touched & np.isfinite(S) & np.isfinite(b)
        assert np.isfinite(a[keep]).all() and (np.abs(a[keep] - b[keep]) <= C_OF[name] * EPS * S[keep]).all(), name
    for which, voxel, value in _plant(shape):
        if which == 0 and np.isnan(value):
            assert np.isnan(got[0][voxel])
    assert got[1][0, 2, 2] == 0.0 and got[1][-1, -1, -1] == 0.0          # planted boundary gradients are masked away


def _state_np(opto, p):
    st = opto.state[p]
    if len(st) == 0:
        return np.zeros(tuple(p.shape), np.float32), np.zeros(tuple(p.shape), np.float32)
    return st["exp_avg"].cpu().numpy().copy(), st["exp_avg_sq"].cpu().numpy().copy()


def _hyper(group, masked):
    return (group["lr"], group["betas"], group["eps"], group["weight_decay"],
            group["mask_boundary"] if masked else True, group["clamp_min"] if masked else 1.0)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(7, 9, 33), (3, 3, 3)])
def test_adam_trajectory_step_by_step(gpu, shape):
    """12 steps of MaskedAdam with weight decay; the referee restarts every step from the device's previous fp32 output,
    so each step is judged on its own arithmetic.  Step counter and state keys are torch.optim.Adam's."""
    from adjointnonlinearraytracing_amd import optimizer
    rng = np.random.default_rng(41)
    p0 = (1.0 + 0.4 * rng.random(shape)).astype(np.float32)
    a = torch.from_numpy(p0.copy()).to(gpu).requires_grad_(True)
    b = torch.from_numpy(p0.copy()).to(gpu).requires_grad_(True)
    oa = torch.optim.Adam([a], lr=3e-2, weight_decay=0.01)
    ob = optimizer.MaskedAdam([b], lr=3e-2, weight_decay=0.01)
    kernel = _Worst("MaskedAdam")
    for k in range(12):
        g = (rng.normal(size=shape) * 10.0 ** (k % 6 - 3)).astype(np.float32)
        p = b.detach().cpu().numpy().copy()
        m, v = _state_np(ob, b)
        a.grad = torch.from_numpy(g.copy()).to(gpu)
        b.grad = torch.from_numpy(g.copy()).to(gpu)
        oa.step()
        ob.step()
        m2, v2 = _state_np(ob, b)
        ref, scales = R.adam_step(p, g, m, v, k + 1, 3e-2, (0.9, 0.999), 1e-8, 0.01, True, 1.0)
        kernel.add(k, (b.detach().cpu().numpy(), b.grad.cpu().numpy(), m2, v2), ref, scales)
        sa, sb = oa.state[a], ob.state[b]
        assert set(sa) == set(sb) == {"step", "exp_avg", "exp_avg_sq"}
        assert float(sa["step"]) == float(sb["step"]) == k + 1
        assert sa["step"].dtype == sb["step"].dtype and sa["step"].device == sb["step"].device
    kernel.report(f"trajectory {shape}")
    kernel.check()


@pytest.mark.gpu
def test_masked_adam_param_groups_and_missing_grads(gpu):
    """Two groups with different lr, betas, mask_boundary and clamp_min each get their own; a parameter without a
    gradient is skipped and gets no state."""
    from adjointnonlinearraytracing_amd import optimizer
    rng = np.random.default_rng(51)
    shapes = [(5, 6, 7), (4, 4, 9), (3, 3, 3)]
    start = [rng.uniform(0.8, 1.5, s).astype(np.float32) for s in shapes]
    a, b, c = (torch.from_numpy(x.copy()).to(gpu).requires_grad_(True) for x in start)
    opto = optimizer.MaskedAdam([dict(params=[a, c], lr=3e-2, betas=(0.8, 0.95), mask_boundary=True, clamp_min=None),
                                 dict(params=[b], lr=1e-3, betas=(0.5, 0.9), mask_boundary=False, clamp_min=1.25)],
                                weight_decay=0.01)
    kernel = _Worst("MaskedAdam")
    for k in range(2):
        grads = [rng.normal(size=s).astype(np.float32) for s in shapes[:2]]
        before = [(t.detach().cpu().numpy().copy(),) + _state_np(opto, t) for t in (a, b)]
        a.grad, b.grad = (torch.from_numpy(x.copy()).to(gpu) for x in grads)
        opto.step()
        for t, g, (p, m, v), group in zip((a, b), grads, before, opto.param_groups):
            ref, scales = R.adam_step(p, g, m, v, k + 1, *_hyper(group, True))
            kernel.add((k, tuple(t.shape)), (t.detach().cpu().numpy(), t.grad.cpu().numpy()) + _state_np(opto, t), ref, scales)
        assert float(opto.state[a]["step"]) == float(opto.state[b]["step"]) == k + 1
    assert len(opto.state[c]) == 0 and c.grad is None
    assert np.array_equal(c.detach().cpu().numpy().view(np.uint32), start[2].view(np.uint32))
    assert float(b.detach().min()) >= 1.25 and float(a.detach().min()) < 1.0          # clamp_min is per group
    kernel.report("param groups")
    kernel.check()


@pytest.mark.gpu
def test_adam_checkpoints_are_interchangeable(gpu):
    """torch.optim.Adam -> state_dict() -> MaskedAdam.load_state_dict() -> step continues from that state (the saved
    groups carry no mask_boundary / clamp_min: the defaults apply), and the same the other way round."""
    from adjointnonlinearraytracing_amd import optimizer
    rng = np.random.default_rng(61)
    shape = (6, 7, 9)
    hyper = dict(lr=2e-2, betas=(0.8, 0.95), eps=1e-6, weight_decay=0.01)
    a = torch.from_numpy((1.0 + 0.4 * rng.random(shape)).astype(np.float32)).to(gpu).requires_grad_(True)
    oa = torch.optim.Adam([a], **hyper)
    mask = torch.ones_like(a, dtype=torch.bool)
    mask[1:-1, 1:-1, 1:-1] = 0

    def literal_step(n, opto, g):
        n.grad = torch.from_numpy(g.copy()).to(gpu)
        with torch.no_grad():
            n.grad[mask] = 0
        opto.step()
        with torch.no_grad():
            n.clamp_(min=1)

    for k in range(3):
        literal_step(a, oa, rng.normal(size=shape).astype(np.float32))
    # torch -> MaskedAdam
    b = a.detach().clone().requires_grad_(True)
    ob = optimizer.MaskedAdam([b])
    ob.load_state_dict(oa.state_dict())
    group = ob.param_groups[0]
    assert (group["lr"], tuple(group["betas"]), group["eps"], group["weight_decay"]) == (2e-2, (0.8, 0.95), 1e-6, 0.01)
    assert group["mask_boundary"] is True and group["clamp_min"] == 1.0
    p, (m, v) = b.detach().cpu().numpy().copy(), _state_np(ob, b)
    assert np.array_equal(m, oa.state[a]["exp_avg"].cpu().numpy()) and float(ob.state[b]["step"]) == 3
    g = rng.normal(size=shape).astype(np.float32)
    b.grad = torch.from_numpy(g.copy()).to(gpu)
    ob.step()
    ref, scales = R.adam_step(p, g, m, v, 4, *_hyper(group, True))
    kernel = _Worst("MaskedAdam after torch's state")
    kernel.add("torch -> MaskedAdam", (b.detach().cpu().numpy(), b.grad.cpu().numpy()) + _state_np(ob, b), ref, scales)
    assert float(ob.state[b]["step"]) == 4
    # MaskedAdam -> torch
    c = b.detach().clone().requires_grad_(True)
    oc = torch.optim.Adam([c])
    oc.load_state_dict(ob.state_dict())
    p, (m, v) = c.detach().cpu().numpy().copy(), _state_np(oc, c)
    g = rng.normal(size=shape).astype(np.float32)
    literal_step(c, oc, g)
    ref, scales = R.adam_step(p, g, m, v, 5, *_hyper(oc.param_groups[0], False))
    back = _Worst("torch after MaskedAdam's state")
    back.add("MaskedAdam -> torch", (c.detach().cpu().numpy(), c.grad.cpu().numpy()) + _state_np(oc, c), ref, scales)
    assert float(oc.state[c]["step"]) == 5
    kernel.report("checkpoint"); back.report("checkpoint")
    kernel.check()
    back.check()


@pytest.mark.gpu
def test_masked_adam_refuses_what_it_cannot_step(gpu):
    from adjointnonlinearraytracing_amd import optimizer
    bad = [torch.ones(3, 4, 5, device=gpu).permute(2, 1, 0).requires_grad_(True),            # not contiguous
           torch.ones(3, 4, 5, device=gpu, dtype=torch.float64, requires_grad=True),
           torch.ones(3, 4, 5, requires_grad=True)]                                           # on the host
    for n in bad:
        before = n.detach().clone()
        opto = optimizer.MaskedAdam([n], lr=0.1)
        n.grad = torch.ones_like(n)
        with pytest.raises(RuntimeError, match="MaskedAdam expects"):
            opto.step()
        assert torch.equal(n.detach(), before) and len(opto.state[n]) == 0
