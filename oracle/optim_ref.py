"""Float64 restatements of the two operators that carry the optimisation loop -- TEST INFRASTRUCTURE ONLY.

`upres` restates the reference's multires up-sampling (core/grid.py upres_volume -> Grid.GetLinear), `adam_step` the
three statements of its loop tail (core/optimizer.py: `n.grad[mask] = 0`, torch.optim.Adam.step(), `n.clamp_(min=1)`)
with the update of torch/optim/adam.py _single_tensor_adam (amsgrad = maximize = False).  Plain numpy, written from
the formulas; no torch in the arithmetic.  tests/test_optimizer_fuzz.py pins both on the CPU (the recorded runs of
tests/golden/upres.npz, torch.linspace, torch.optim.Adam in float64) and referees the HIP kernels with them.
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np

EPS32 = float(np.finfo(np.float32).eps)          # 2^-23
SUBNORMAL32 = 2.0 ** -149                        # the smallest fp32 subnormal
# one fp32 rounding moves a result r by at most EPS32 * (|r| + TINY): the second term is the subnormal range's fixed step
TINY = SUBNORMAL32 / EPS32
# the denominator of the update counts as undetermined once 64 of its first-order errors reach it
ILL = 64.0


def linspace01(s: int) -> np.ndarray:
    """torch.linspace(0, 1, s, dtype=float64): step * i from the start for the first half, 1 - step * (s - 1 - i) from
    the end for the second -- evaluated as ONE fused multiply-add, i.e. rounded once (torch's kernels are compiled with
    contraction; the two-rounding form differs in the last bit from s = 16 on) --, and the start alone for one step."""
    s = int(s)
    if s == 1:
        return np.zeros(1)
    step = 1.0 / (s - 1)
    exact = Fraction(step)
    # float(Fraction) is the correctly rounded quotient of two integers: the single rounding of a fused multiply-add
    return np.array([step * i if i < s // 2 else float(1 - exact * (s - 1 - i)) for i in range(s)], dtype=np.float64)


def upres(src, dst_shape) -> np.ndarray:
    """Trilinear resampling of the cubic volume `src` (R, R, R) at linspace(0, 1, s)^3, per axis s of `dst_shape`:
    nx = x / h with h = 1 / max(R - 1, 1), cell floor(nx), weight nx - floor(nx) clipped to [0, 1], both cell indices
    clipped to [0, R - 1].  Evaluated one axis at a time (the eight-term sum factorises), in float64."""
    out = np.asarray(src, dtype=np.float64)
    if out.ndim != 3 or len(set(out.shape)) != 1:
        raise ValueError("upres expects a cubic 3-D source")
    R = out.shape[0]
    h = 1.0 / max(R - 1, 1)
    for axis, s in enumerate(dst_shape):
        nx = linspace01(s) / h
        cell = np.floor(nx)
        w = np.clip(nx - cell, 0.0, 1.0)
        cell = cell.astype(np.int64)
        lo, hi = np.clip(cell, 0, R - 1), np.clip(cell + 1, 0, R - 1)
        bshape = [1, 1, 1]
        bshape[axis] = -1
        w = w.reshape(bshape)
        out = (1.0 - w) * np.take(out, lo, axis=axis) + w * np.take(out, hi, axis=axis)
    return out


def boundary_mask(shape) -> np.ndarray:
    """True on the outermost voxel layer (`mask = ones; mask[1:-1, 1:-1, 1:-1] = 0`)."""
    shell = np.ones(shape, dtype=bool)
    shell[1:-1, 1:-1, 1:-1] = False
    return shell


def adam_step(p, g, m, v, step, lr, betas, eps, weight_decay, mask_boundary, clamp_min):
    """One iteration's tail on the values given (fp32 data is taken as it is; all arithmetic in float64).

    -> (p', g_masked, m', v'), (Sp, Sg, Sm, Sv).  S* are first-order error scales per element: an fp32 evaluation of the
    same statements, in any grouping, is expected within c * EPS32 * S of the float64 value, c a small constant.  Each is
    the sum of the magnitudes of the terms a rounding acts on, carried through the later statements by their
    derivatives; every rounding also adds TINY (the subnormal step).  Where weight decay may cancel the gradient the
    scale keeps |g| + wd |p|, not |g + wd p|.  The square root is carried as min(dv / sqrt v, sqrt dv): at v ~ 0 its
    derivative is unbounded but the root moves by no more than sqrt dv.  Sp is inf where the denominator
    sqrt(v') / sqrt(bias_correction2) + eps is not determined to first order (ILL of its errors reach it; only when
    eps is 0 or tiny): the update is then noise in any fp32 evaluation.  Sg is 0: the mask is exact."""
    p, g, m, v = (np.array(a, dtype=np.float64) for a in (p, g, m, v))
    b1, b2 = float(betas[0]), float(betas[1])
    w1, w2 = 1.0 - b1, 1.0 - b2
    wd, lr, eps, step = float(weight_decay), float(lr), float(eps), float(step)
    with np.errstate(all="ignore"):
        gm = g.copy()
        if mask_boundary:
            gm[boundary_mask(g.shape)] = 0.0
        if wd != 0.0:                                         # grad = grad.add(param, alpha=weight_decay)
            ge = gm + wd * p
            Se = np.abs(gm) + 2.0 * wd * np.abs(p) + TINY
        else:
            ge, Se = gm, np.zeros_like(gm)
        d = ge - m                                            # exp_avg.lerp_(grad, 1 - beta1)
        # lerp weighs from the nearer end, m + w d for w < 0.5 and g - (1 - w) d otherwise (beta1 = 0 leaves exactly g):
        # the roundings of d, the weight and the product
        m2 = m + w1 * d if w1 < 0.5 else ge - (1.0 - w1) * d
        Sm = w1 * Se + 3.0 * min(w1, b1) * np.abs(d) + np.abs(m2) + TINY
        v2 = b2 * v + w2 * ge * ge                            # exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
        Sv = 2.0 * b2 * np.abs(v) + 3.0 * w2 * ge * ge + 2.0 * w2 * np.abs(ge) * Se + np.abs(v2) + 3.0 * TINY
        bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
        step_size, bc2_sqrt = lr / bc1, bc2 ** 0.5
        sv = np.sqrt(v2)
        Ssv = np.minimum(Sv / sv, np.sqrt(Sv / EPS32)) + sv
        den = sv / bc2_sqrt + eps                             # (exp_avg_sq.sqrt() / bias_correction2_sqrt).add_(eps)
        Sden = (Ssv + 2.0 * sv) / bc2_sqrt + eps + np.abs(den) + TINY
        q = m2 / den
        p2 = p - step_size * q                                # param.addcdiv_(exp_avg, denom, value=-step_size)
        Sq = Sm / den + np.abs(q) * Sden / den + np.abs(q)
        Sp = abs(step_size) * (Sq + 2.0 * np.abs(q)) + np.abs(p2) + TINY
        Sp = np.where(ILL * EPS32 * Sden < den, Sp, np.inf)
        if clamp_min is not None:                             # n.clamp_(min=...): NaN stays NaN
            p2 = np.where(p2 < float(clamp_min), float(clamp_min), p2)
    return (p2, gm, m2, v2), (Sp, np.zeros_like(gm), Sm, Sv)
