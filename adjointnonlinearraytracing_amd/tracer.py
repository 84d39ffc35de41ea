"""Counterpart of the reference's ``core/tracer.py``: the ``torch.autograd.Function`` classes the
``*_opt.py`` scripts call, with identical names, argument order and return arity
(``/root/reference/core/tracer.py:294-526``), backed by ``drrt.TracerC`` (HIP kernels).

Contract reproduced from the reference:
  * forward inputs are detached, flattened C-order and narrowed to fp32 (``:299-301``);
  * forward keeps ``rif``, the exit rays and the scalars for backward and returns fresh tensors.  The reference
    snapshots the grid (``FloatC(rif.flatten())`` copies, ``:299``); here ``rif`` and the exit rays are kept with
    ``ctx.save_for_backward`` -- no copies, and autograd's version check turns an in-place update of ``rif`` (or of
    the returned exit rays) between forward and backward into a RuntimeError instead of a silently wrong gradient;
  * backward returns ``drif`` reshaped to ``rif.shape`` and ``None`` for every other input
    (no gradient w.r.t. ``x``, ``v``: ``:335,386,432,479,526``) -- ADTracerC, ADCableTracerC, ADRayPlaneTracerC,
    ADRaySDFTracerC and ADRayTargetTracerC (below) are the classes with ray gradients;
  * ``BackPlaneTracerC`` / ``BackTargetTracerC`` backward run the GENERIC ``backtrace`` from the
    recorded state (``:376,422``); ``BackPlaneTracerC.backward`` zeroes ``grad_x`` on
    rays whose ``outmask`` gradient is set, as written (``:366-367``).
The enoki pool trim (``enoki.cuda_malloc_trim()``, ``:314``) has no counterpart: outputs are
torch allocations.
"""
from __future__ import annotations

import dataclasses

import torch

from . import drrt


# ---- what the classes of a march family share --------------------------------------------------------------------------
# A family is one forward march (trace, trace_pln, trace_target, trace_sdf, trace_cable) with its Back* class, its AD* class
# (ray gradients too) and, for trace, dist.ShardedBackTracerC.  Its forward and its dL/drif are written once, below; a class
# adds what is its own: the signature of apply(), the mask of the plane march, the ray-state adjoint of an AD* class.
def _ray_grad_wanted(ctx, name, ix, iv, x, v):
    """Whether x or v (at positions ix, iv of apply()) requires grad; the ray-state adjoints take fp32 rays only."""
    wanted = ctx.needs_input_grad[ix] or ctx.needs_input_grad[iv]
    if wanted and (x.dtype != torch.float32 or v.dtype != torch.float32):
        raise RuntimeError(f"{name}: gradients w.r.t. x, v need float32 rays")
    return wanted


def _keep_rays(ctx, x, v, device, *extra):
    """Private fp32 copies on the march's `device` of the forward's ray inputs (x, v, *extra) -> ``ctx.rays``."""
    ctx.ray_devices = (x.device, v.device)
    ctx.rays = tuple(t.detach().to(device=device, dtype=torch.float32).clone() for t in (x, v) + extra)


def _grid_forward(ctx, march, rif, sdf, x, v, extra, h, ds, ad=None):
    """Forward of a grid family: ``march(flat rif, [flat sdf], rif.shape, x, v, *extra, h, ds) -> (outputs, order, steps)``
    (a ``TracerC._trace*``) on detached inputs -> (outputs, steps).  ``ctx`` gets the shape and the scalars, a private copy
    of the march's own visit order (the adjoint visits rays in the forward's bundle order; other tracer calls may come
    before backward) and, saved, ``rif``, the SDF and the exit rays.  `ad` = (class name, positions of x and v in apply())
    for an AD* class: private copies of (x, v, *extra) are kept when x or v requires grad, and only then."""
    ctx.shape, ctx.h, ctx.ds = rif.shape, h, ds
    ray_grad = ad is not None and _ray_grad_wanted(ctx, *ad, x, v)
    grids = (rif,) if sdf is None else (rif, sdf)
    out, order, steps = march(*[g.detach().flatten() for g in grids], ctx.shape, x.detach(), v.detach(),
                              *[t.detach() for t in extra], h, ds)
    ctx.order = drrt.keep_order(order)
    if ray_grad:
        _keep_rays(ctx, x, v, out[0].device, *extra)
    ctx.save_for_backward(*grids, out[0], out[1])
    return out, steps


def _grid_rif_grad(ctx, grad_x, grad_v):
    """dL/drif of a grid family from the recorded state: ``backtrace_sdf`` for the SDF march, the generic ``backtrace``
    for every other (core/tracer.py:376,422), in the forward's visit order."""
    rif, *sdf, outx, outv = ctx.saved_tensors
    adjoint = drrt.TracerC().backtrace_sdf if sdf else drrt.TracerC().backtrace
    return adjoint(rif.detach().flatten(), *[s.detach().flatten() for s in sdf], ctx.shape, outx, outv, grad_x, grad_v,
                   ctx.h, ctx.ds, order=ctx.order).reshape(*ctx.shape)


def _cable_forward(ctx, rif, radius, length, x, v, sp, ds, ad=None):
    """Forward of the fibre family, as `_grid_forward` (the fibre march has no visit order)."""
    ctx.radius, ctx.length, ctx.ds = radius, length, ds
    ray_grad = ad is not None and _ray_grad_wanted(ctx, *ad, x, v)
    out = drrt.TracerC().trace_cable(rif.detach().flatten(), radius, length, x.detach(), v.detach(), sp.detach(), ds)
    if ray_grad:
        _keep_rays(ctx, x, v, out[0].device, sp)
    ctx.save_for_backward(rif, out[0], out[1])
    return out


def _cable_rif_grad(ctx, grad_x, grad_v):
    rif, outx, outv = ctx.saved_tensors
    return drrt.TracerC().backtrace_cable(rif.detach().flatten(), ctx.radius, ctx.length, outx, outv,
                                          grad_x, grad_v, ctx.ds).reshape(rif.shape)


def _plane_mask(ctx, out):
    """(xt, vt, failmask uint8) -> (xt, vt, failmask bool, not differentiable)."""
    outmask = out[2].to(torch.bool)
    ctx.mark_non_differentiable(outmask)
    return out[0], out[1], outmask


def _mask_plane_seed(grad_x, outmask):
    """The plane classes' incoming position seed, zeroed on the rays whose ``outmask`` gradient is set (as written,
    core/tracer.py:366-367)."""
    if outmask is not None and outmask.dtype == torch.bool:
        grad_x = grad_x.clone()
        grad_x[outmask] = 0
    return grad_x


def _ad_grads(ctx, ix, iv, rif_grad, ray_adjoint, grad_x, grad_v):
    """(dL/drif, dL/dx, dL/dv) of an AD* class: each adjoint runs only for the inputs that ask for a gradient, so with
    neither ray input requiring grad the launches are the Back* class's.  ``ray_adjoint() -> (dpos, dvel)``; the ray
    gradients go back to the callers' devices, None where not asked for."""
    drif = rif_grad(ctx, grad_x, grad_v) if ctx.needs_input_grad[0] else None
    dx0 = dv0 = None
    if ctx.needs_input_grad[ix] or ctx.needs_input_grad[iv]:
        dpos, dvel = ray_adjoint()
        dx0 = dpos.to(ctx.ray_devices[0]) if ctx.needs_input_grad[ix] else None
        dv0 = dvel.to(ctx.ray_devices[1]) if ctx.needs_input_grad[iv] else None
    return drif, dx0, dv0


class BackTracerC(torch.autograd.Function):
    """core/tracer.py:294-335 -- ``apply(rif, x, v, h, ds) -> (xt, vt)``."""

    @staticmethod
    def forward(ctx, rif, x, v, h, ds):
        return _grid_forward(ctx, drrt.TracerC()._trace, rif, None, x, v, (), h, ds)[0]

    @staticmethod
    def backward(ctx, grad_x, grad_v):
        return _grid_rif_grad(ctx, grad_x, grad_v), None, None, None, None


class BackPlaneTracerC(torch.autograd.Function):
    """core/tracer.py:338-386 -- ``apply(rif, x, v, sp, sn, h, ds) -> (xt, vt, failmask bool)``."""

    @staticmethod
    def forward(ctx, rif, x, v, sp, sn, h, ds):
        return _plane_mask(ctx, _grid_forward(ctx, drrt.TracerC()._trace_pln, rif, None, x, v, (sp, sn), h, ds)[0])

    @staticmethod
    def backward(ctx, grad_x, grad_v, outmask):
        return _grid_rif_grad(ctx, _mask_plane_seed(grad_x, outmask), grad_v), None, None, None, None, None, None


class BackTargetTracerC(torch.autograd.Function):
    """core/tracer.py:389-432 -- ``apply(rif, x, v, sp, h, ds) -> (xt, vt, dist2)``."""

    @staticmethod
    def forward(ctx, rif, x, v, sp, h, ds):
        return _grid_forward(ctx, drrt.TracerC()._trace_target, rif, None, x, v, (sp,), h, ds)[0]

    @staticmethod
    def backward(ctx, grad_x, grad_v, outdist):
        return _grid_rif_grad(ctx, grad_x, grad_v), None, None, None, None, None


class BackSDFTracerC(torch.autograd.Function):
    """core/tracer.py:435-479 -- ``apply(rif, sdf, x, v, h, ds) -> (xt, vt)``."""

    @staticmethod
    def forward(ctx, rif, sdf, x, v, h, ds):
        return _grid_forward(ctx, drrt.TracerC()._trace_sdf, rif, sdf, x, v, (), h, ds)[0]

    @staticmethod
    def backward(ctx, grad_x, grad_v):
        return _grid_rif_grad(ctx, grad_x, grad_v), None, None, None, None, None


class BackCableTracerC(torch.autograd.Function):
    """core/tracer.py:482-526 -- ``apply(rif (Rr,), radius, length, x, v, sp, ds) -> (xt, vt, dist2)``."""

    @staticmethod
    def forward(ctx, rif, radius, length, x, v, sp, ds):
        return _cable_forward(ctx, rif, radius, length, x, v, sp, ds)

    @staticmethod
    def backward(ctx, grad_x, grad_v, outdist):
        return _cable_rif_grad(ctx, grad_x, grad_v), None, None, None, None, None, None


class ADTracerC(torch.autograd.Function):
    """core/tracer.py:16-66 -- ``apply(rif, x, v, h, ds) -> (xt, vt)`` with gradients for ``rif`` AND the rays.

    The reference differentiates its enoki march (``enoki.gradient(ctx.x)``, ``ctx.v``); here the forward and dL/drif are
    BackTracerC's and dL/dx, dL/dv come from the ray-state adjoint ``TracerC.backtrace_rays`` (drrt_backtrace_rays_f32),
    which needs the forward's inputs and per-ray iteration counts: those are kept (private copies) only when ``x`` or
    ``v`` requires grad.  Rays that failed the forward (ran out of steps) get a zero ray gradient.  fp32 rays only when
    ray gradients are asked for."""

    @staticmethod
    def forward(ctx, rif, x, v, h, ds):
        out, steps = _grid_forward(ctx, drrt.TracerC()._trace, rif, None, x, v, (), h, ds, ad=("ADTracerC", 1, 2))
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            steps = drrt.keep_steps(steps)
            if steps is None:
                raise RuntimeError("ADTracerC: the forward march left no iteration counts")
            ctx.rays += (steps,)
        return out

    @staticmethod
    def backward(ctx, grad_x, grad_v):
        rif, outx, outv = ctx.saved_tensors

        def ray_adjoint():
            x0, v0, steps = ctx.rays
            return drrt.TracerC().backtrace_rays(rif.detach().flatten(), ctx.shape, x0, v0, outx, outv, steps,
                                                 grad_x, grad_v, ctx.h, ctx.ds, order=ctx.order)
        return (*_ad_grads(ctx, 1, 2, _grid_rif_grad, ray_adjoint, grad_x, grad_v), None, None)


class ADCableTracerC(torch.autograd.Function):
    """core/tracer.py:237-291 -- ``apply(rif (Rr,), radius, length, x, v, sp, ds) -> (xt, vt, dist2)`` with gradients for
    ``rif`` AND the rays that enter the fibre march.

    The forward and dL/drif are BackCableTracerC's and dL/dx, dL/dv come from the ray-state adjoint
    ``TracerC.backtrace_cable_rays`` (drrt_backtrace_cable_rays_f32).  That call replays the forward from its inputs, so
    the inputs (x, v, sp) are kept (private copies) only when ``x`` or ``v`` requires grad.  The iteration of the
    closest-approach record is held fixed, and the gradient arriving on ``dist2`` is ignored, as in the reference
    (``:268-272``) and in BackCableTracerC; no gradient flows to ``sp``.  A ray that ran out of steps still has a record
    and a gradient.  fp32 rays only when ray gradients are asked for."""

    @staticmethod
    def forward(ctx, rif, radius, length, x, v, sp, ds):
        return _cable_forward(ctx, rif, radius, length, x, v, sp, ds, ad=("ADCableTracerC", 3, 4))

    @staticmethod
    def backward(ctx, grad_x, grad_v, outdist):
        rif = ctx.saved_tensors[0]
        drif, dx0, dv0 = _ad_grads(ctx, 3, 4, _cable_rif_grad, lambda: drrt.TracerC().backtrace_cable_rays(
            rif.detach().flatten(), ctx.radius, ctx.length, *ctx.rays, grad_x, grad_v, ctx.ds), grad_x, grad_v)
        return drif, None, None, dx0, dv0, None, None


class ADRayPlaneTracerC(torch.autograd.Function):
    """``apply(rif, x, v, sp, sn, h, ds) -> (xt, vt, failmask bool)`` with gradients for ``rif`` AND the rays: what the
    reference's ADPlaneTracerC (core/tracer.py:122-178, broken upstream) is meant to be.  The name is new because
    ``ADPlaneTracerC`` stays the alias of BackPlaneTracerC it has always been here.

    The forward and dL/drif are BackPlaneTracerC's and dL/dx, dL/dv come from the ray-state adjoint
    ``TracerC.backtrace_pln_rays`` (drrt_backtrace_pln_rays_f32), which replays the forward from its inputs: (x, v, sp, sn)
    are kept (private copies) only when ``x`` or ``v`` requires grad.  The incoming seeds are treated as
    BackPlaneTracerC.backward treats them and the same seeds go to both adjoints.  Rays that failed the forward get a zero
    ray gradient; no gradient flows to the plane or to ``failmask``.  fp32 rays only when ray gradients are asked for."""

    @staticmethod
    def forward(ctx, rif, x, v, sp, sn, h, ds):
        return _plane_mask(ctx, _grid_forward(ctx, drrt.TracerC()._trace_pln, rif, None, x, v, (sp, sn), h, ds,
                                              ad=("ADRayPlaneTracerC", 1, 2))[0])

    @staticmethod
    def backward(ctx, grad_x, grad_v, outmask):
        rif = ctx.saved_tensors[0]
        grad_x = _mask_plane_seed(grad_x, outmask)
        return (*_ad_grads(ctx, 1, 2, _grid_rif_grad, lambda: drrt.TracerC().backtrace_pln_rays(
            rif.detach().flatten(), ctx.shape, *ctx.rays, grad_x, grad_v, ctx.h, ctx.ds, order=ctx.order),
            grad_x, grad_v), None, None, None, None)


class ADRaySDFTracerC(torch.autograd.Function):
    """``apply(rif, sdf, x, v, h, ds) -> (xt, vt)`` with gradients for ``rif`` AND the rays (the reference's ADSDFTracerC,
    core/tracer.py:181-234; ``ADSDFTracerC`` stays the alias of BackSDFTracerC here).

    The forward and dL/drif are BackSDFTracerC's and dL/dx, dL/dv come from ``TracerC.backtrace_sdf_rays``
    (drrt_backtrace_sdf_rays_f32), which replays the forward from (x, v): private copies of those are kept only when
    ``x`` or ``v`` requires grad (the SDF is saved anyway).  A ray that never crosses the surface has its input as its
    record and the identity as its ray gradient; no gradient flows to the SDF.  fp32 rays only when ray gradients are
    asked for."""

    @staticmethod
    def forward(ctx, rif, sdf, x, v, h, ds):
        return _grid_forward(ctx, drrt.TracerC()._trace_sdf, rif, sdf, x, v, (), h, ds, ad=("ADRaySDFTracerC", 2, 3))[0]

    @staticmethod
    def backward(ctx, grad_x, grad_v):
        rif, sdf = ctx.saved_tensors[:2]
        drif, dx0, dv0 = _ad_grads(ctx, 2, 3, _grid_rif_grad, lambda: drrt.TracerC().backtrace_sdf_rays(
            rif.detach().flatten(), sdf.detach().flatten(), ctx.shape, *ctx.rays, grad_x, grad_v, ctx.h, ctx.ds,
            order=ctx.order), grad_x, grad_v)
        return drif, None, dx0, dv0, None, None


class ADRayTargetTracerC(torch.autograd.Function):
    """``apply(rif, x, v, sp, h, ds) -> (xt, vt, dist2)`` with all three outputs differentiable w.r.t. ``rif``, the rays AND
    the target ``sp`` (the reference binds trace_target on its enoki autodiff tracer, src/drrt.cpp:34, and has no class).

    The forward is BackTargetTracerC's.  With ``g`` the gradient arriving on ``dist2 = |xt - sp|^2``, the position seed of
    both adjoints is ``grad_x + 2 g (xt - sp)``:
      * dL/drif: the generic ``backtrace`` from the record with that seed and ``grad_v``; with a zero ``g`` it
        is BackTargetTracerC's gradient.  For a record written after the ray left the box the generic ``backtrace`` samples
        clamped cells on its way back to the box (Q12 again): that part of dL/drif is not exact, here as there;
      * dL/dx, dL/dv: ``TracerC.backtrace_target_rays`` (drrt_backtrace_target_rays_f32), which replays the forward from
        (x, v, sp) -- private copies, kept only when ``x`` or ``v`` requires grad -- and forms the seed itself from
        ``grad_x`` and ``g``; the iteration of the record is held fixed.  A ray that ran out of steps keeps its record and
        its gradient;
      * dL/dsp = ``-2 g (xt - sp)``, without a launch.
    fp32 rays only when ray gradients are asked for."""

    @staticmethod
    def forward(ctx, rif, x, v, sp, h, ds):
        out = _grid_forward(ctx, drrt.TracerC()._trace_target, rif, None, x, v, (sp,), h, ds,
                            ad=("ADRayTargetTracerC", 1, 2))[0]
        ctx.sp_like = (sp.device, sp.dtype)
        ctx.target = sp.detach().to(device=out[0].device, dtype=torch.float32).clone()
        return out

    @staticmethod
    def backward(ctx, grad_x, grad_v, grad_d):
        rif, outx, _ = ctx.saved_tensors
        pull = (2 * grad_d)[:, None] * (outx - ctx.target)               # d(g dist2)/d(xt)
        drif, dx0, dv0 = _ad_grads(ctx, 1, 2, _grid_rif_grad, lambda: drrt.TracerC().backtrace_target_rays(
            rif.detach().flatten(), ctx.shape, *ctx.rays, grad_x, grad_v, ctx.h, ctx.ds, ddist2=grad_d, order=ctx.order),
            grad_x + pull, grad_v)
        dsp = (-pull).to(device=ctx.sp_like[0], dtype=ctx.sp_like[1]) if ctx.needs_input_grad[3] else None
        return drif, dx0, dv0, dsp, None, None


def _integral_forward(ctx, name, march, rif, fields, x, v, h, ds, keep=0):
    """The forward of the integral operators' classes -> (xt, vt, *integrals): `march` (``TracerC._trace_opl``, ...) on
    `rif`, the further grids `fields` (((argument name, grid), ...), each of rif's shape, or ((argument name, grid, lead),
    ...) for a grid of shape ``lead + rif.shape``: the component planes of a vector field) and the rays.  When any input
    requires grad, what the ONE backward launch needs is kept: the options in effect now (autograd runs backward on a thread
    of its own), the visit order, private copies of (x, v), the iteration counts and, saved with the grids and the exit
    rays, the last `keep` integrals."""
    ctx.set_materialize_grads(False)
    leads = tuple(tuple(f[2]) if len(f) > 2 else () for f in fields)
    fields = tuple((f[0], f[1]) for f in fields)
    for (fname, field), lead in zip(fields, leads):
        if tuple(field.shape) != lead + tuple(rif.shape):
            want = f"rif {tuple(rif.shape)}" if not lead else f"rif {tuple(rif.shape)} behind {lead}"
            raise RuntimeError(f"{name}: {fname} has shape {tuple(field.shape)}, {want}")
    ctx.shape, ctx.h, ctx.ds, ctx.n_fields, ctx.leads = rif.shape, h, ds, len(fields), ((),) + leads
    _ray_grad_wanted(ctx, name, 1 + len(fields), 2 + len(fields), x, v)
    (xt, vt, *integrals, steps), order, _ = march(rif.detach().flatten(), *(f.detach().flatten() for _, f in fields),
                                                  ctx.shape, x.detach(), v.detach(), h, ds)
    if any(ctx.needs_input_grad[:3 + len(fields)]):
        ctx.options = dataclasses.asdict(drrt._opt())
        ctx.order = drrt.keep_order(order)
        _keep_rays(ctx, x, v, xt.device)
        ctx.rays += (steps,)
        ctx.save_for_backward(rif, *(f for _, f in fields), xt, vt, *integrals[len(integrals) - keep:])
    return (xt, vt, *integrals)


def _integral_backward(ctx, back, grad_x, grad_v, *seeds):
    """-> (drif, *dfields, dx0, dv0) from ONE launch of `back` (``TracerC.backtrace_opl``, ...) under the forward's options,
    computing only what ``ctx.needs_input_grad`` asks for."""
    k = ctx.n_fields
    want_grids, want_rays = ctx.needs_input_grad[:1 + k], ctx.needs_input_grad[1 + k] or ctx.needs_input_grad[2 + k]
    if not (any(want_grids) or want_rays):
        return (None,) * (3 + k)
    grids, (outx, outv, *kept) = ctx.saved_tensors[:1 + k], ctx.saved_tensors[1 + k:]
    x0, v0, steps = ctx.rays
    with drrt.using(**ctx.options):
        *grads, dpos, dvel = back(*(g.detach().flatten() for g in grids), ctx.shape, x0, v0, outx, outv, steps, *kept, grad_x,
                                  grad_v, *seeds, ctx.h, ctx.ds, *want_grids, want_rays, order=ctx.order)
    dx0 = dpos.to(ctx.ray_devices[0]) if ctx.needs_input_grad[1 + k] else None
    dv0 = dvel.to(ctx.ray_devices[1]) if ctx.needs_input_grad[2 + k] else None
    return (*(g.reshape(*lead, *ctx.shape) if want else None for g, want, lead in zip(grads, want_grids, ctx.leads)),
            dx0, dv0)


class OPLTracerC(torch.autograd.Function):
    """``apply(rif, x, v, h, ds) -> (xt, vt, opl)``: ``trace`` with the optical path length ``opl = sum ds n_k^2`` of every
    ray (|v| = n along the march, so this is the integral of n along the path), all three outputs differentiable w.r.t.
    ``rif``, ``x`` and ``v``.  Not in the reference.

    The forward is ``TracerC.trace_opl``; backward is ONE ``TracerC.backtrace_opl`` launch (plus the zero-fill of the grid
    gradient when ``rif`` requires grad), which returns dL/drif and the ray gradients from the same reverse march and
    computes only what is asked for.  Unlike the Back* / AD* classes, whose dL/drif is the reference's ``backtrace`` from
    the exit ray, this adjoint replays the forward's iteration count: with ``drrt.options.corrected_h`` its dL/drif is the
    exact discrete derivative.  ``sort_rays`` and ``pair_grid`` are honoured as in ADTracerC; the options in effect at the
    forward (``drrt.options``, or the calling thread's ``drrt.using(...)`` block) are kept and applied to the backward launch,
    which autograd runs on a thread of its own.  Private copies of (x, v) and the iteration counts are kept whenever any
    input requires grad.  Rays that failed the forward get zero gradients.  fp32 rays only when ray gradients are asked
    for."""

    @staticmethod
    def forward(ctx, rif, x, v, h, ds):
        return _integral_forward(ctx, "OPLTracerC", drrt.TracerC()._trace_opl, rif, (), x, v, h, ds)

    @staticmethod
    def backward(ctx, grad_x, grad_v, grad_opl):
        return (*_integral_backward(ctx, drrt.TracerC().backtrace_opl, grad_x, grad_v, grad_opl), None, None)


class FieldIntegralTracerC(torch.autograd.Function):
    """``apply(rif, field, x, v, h, ds) -> (xt, vt, tau)``: ``trace`` with the line integral ``tau = sum ds n_k a_k`` of a
    second voxel field ``a`` (``field``: an absorption or emission coefficient, a group index; a grid of ``rif``'s shape)
    along every bent ray (|v| = n along the march, so this is the integral of the field along the path), all three outputs
    differentiable w.r.t. ``rif``, ``field``, ``x`` and ``v``.  Not in the reference.

    The forward is ``TracerC.trace_field``; backward is ONE ``TracerC.backtrace_field`` launch (plus one zero-fill per grid
    gradient asked for), which returns dL/drif, dL/dfield and the ray gradients from the same reverse march and computes
    only what is asked for.  Like OPLTracerC this adjoint replays the forward's iteration count: with
    ``drrt.options.corrected_h`` its dL/drif is the exact discrete derivative; dL/dfield and the ray gradients are that
    either way.  ``sort_rays`` and ``pair_grid`` are honoured as in ADTracerC; the options in effect at the forward
    (``drrt.options``, or the calling thread's ``drrt.using(...)`` block) are kept and applied to the backward launch, which
    autograd runs on a thread of its own.  Private copies of (x, v) and the iteration counts are kept whenever any input
    requires grad.  Rays that failed the forward get zero gradients.  fp32 rays only when ray gradients are asked for."""

    @staticmethod
    def forward(ctx, rif, field, x, v, h, ds):
        return _integral_forward(ctx, "FieldIntegralTracerC", drrt.TracerC()._trace_field, rif, (("field", field),), x, v, h,
                                 ds)

    @staticmethod
    def backward(ctx, grad_x, grad_v, grad_tau):
        return (*_integral_backward(ctx, drrt.TracerC().backtrace_field, grad_x, grad_v, grad_tau), None, None)


class EmissionTracerC(torch.autograd.Function):
    """``apply(rif, emission, absorption, x, v, h, ds) -> (xt, vt, rad, tau)``: ``trace`` with the radiative-transfer line
    integral ``rad = int e exp(-int a)`` of an emitting (``emission``) and self-absorbing (``absorption``) medium -- two
    grids of ``rif``'s shape -- along every bent ray, and the optical depth ``tau = int a dl``: what a camera sees through
    a flame, a hot jet or a fluorescing volume that also refracts.  Over the samples inside the box, with
    ``w_k = ds n_k``: ``rad = sum exp_neg(tau_k) w_k e_k`` (the transmittance in front of the sample), ``tau = sum w_k a_k``.
    All four outputs are differentiable w.r.t. ``rif``, ``emission``, ``absorption``, ``x`` and ``v``.  Not in the reference.

    The forward is ``TracerC.trace_emission``; backward is ONE ``TracerC.backtrace_emission`` launch (plus one zero-fill per
    grid gradient asked for), which returns all five gradients from the same reverse march and computes only what is asked
    for.  The reverse march recovers every transmittance from the forward's ``tau`` by subtraction, so dL/demission,
    dL/dabsorption and the ray gradients are the derivative of the discrete forward to fp32 rounding; dL/drif is the same
    derivative with ``drrt.options.corrected_h``.  ``sort_rays`` and ``pair_grid`` are honoured as in ADTracerC; the options
    in effect at the forward (``drrt.options``, or the calling thread's ``drrt.using(...)`` block) are kept and applied to
    the backward launch, which autograd runs on a thread of its own.  Private copies of (x, v) and the iteration counts are
    kept, and ``tau`` is saved with the exit rays, whenever any input requires grad.  Rays that failed the forward get zero gradients.  fp32 rays only
    when ray gradients are asked for."""

    @staticmethod
    def forward(ctx, rif, emission, absorption, x, v, h, ds):
        return _integral_forward(ctx, "EmissionTracerC", drrt.TracerC()._trace_emission, rif,
                                 (("emission", emission), ("absorption", absorption)), x, v, h, ds, keep=1)

    @staticmethod
    def backward(ctx, grad_x, grad_v, grad_rad, grad_tau):
        return (*_integral_backward(ctx, drrt.TracerC().backtrace_emission, grad_x, grad_v, grad_rad, grad_tau), None, None)


class VectorIntegralTracerC(torch.autograd.Function):
    """``apply(rif, vfield, x, v, h, ds) -> (xt, vt, circ)``: ``trace`` with the line integral ``circ = int u . dl`` of a
    vector field ``u`` projected on the ray's own direction (``vfield``: a flow velocity, n_e B; shape ``(3,) + rif.shape``,
    component planes of ``rif``'s shape, plane c pairing with component c of x / v) along every bent ray:
    ``circ = sum ds u_k . v_{k+1}`` over the samples inside the box, v_{k+1} the velocity that carries the ray from x_k to
    x_{k+1}.  All three outputs are differentiable w.r.t. ``rif``, ``vfield``, ``x`` and ``v``; ``vfield.grad`` has
    ``vfield``'s shape.  Not in the reference.

    The forward is ``TracerC.trace_vector``; backward is ONE ``TracerC.backtrace_vector`` launch (plus one zero-fill per
    gradient plane asked for: one for ``rif``, three for ``vfield``), which returns dL/drif, dL/dvfield and the ray gradients
    from the same reverse march and computes only what is asked for.  Like OPLTracerC this adjoint replays the forward's
    iteration count: with ``drrt.options.corrected_h`` its dL/drif is the exact discrete derivative; dL/dvfield and the ray
    gradients are that either way.  ``sort_rays`` and ``pair_grid`` are honoured as in ADTracerC; the options in effect at
    the forward (``drrt.options``, or the calling thread's ``drrt.using(...)`` block) are kept and applied to the backward
    launch, which autograd runs on a thread of its own.  Private copies of (x, v) and the iteration counts are kept whenever
    any input requires grad.  Rays that failed the forward get zero gradients.  fp32 rays only when ray gradients are asked
    for."""

    @staticmethod
    def forward(ctx, rif, vfield, x, v, h, ds):
        return _integral_forward(ctx, "VectorIntegralTracerC", drrt.TracerC()._trace_vector, rif,
                                 (("vfield", vfield, (3,)),), x, v, h, ds)

    @staticmethod
    def backward(ctx, grad_x, grad_v, grad_circ):
        return (*_integral_backward(ctx, drrt.TracerC().backtrace_vector, grad_x, grad_v, grad_circ), None, None)


def _path_forward(ctx, name, velocities, rif, x, v, h, ds, stride, samples):
    """Forward of PathTracerC and, with `velocities`, of PhasePathTracerC -> (xt, vt, path[, vpath], count); keeps the stride
    and the length of the series for the backward."""
    def march(*a):
        out, order, left = drrt.TracerC()._trace_path(*a, stride, samples, velocities=velocities)
        ctx.stride, ctx.samples = int(stride), int(out[2].shape[0])
        return out, order, left
    *out, count = _integral_forward(ctx, name, march, rif, (), x, v, h, ds)
    ctx.mark_non_differentiable(count)
    return (*out, count)


def _path_backward(ctx, backtrace, grad_x, grad_v, *seeds):
    """Backward of the same two: ONE launch of `backtrace` (``TracerC.backtrace_path`` / ``backtrace_phase``), with the kept
    stride and series length spliced into `_integral_backward`'s call."""
    def back(*a, **kw):                 # a: (rif, shape, x0, v0, xt, vt, steps, dx, dv, *seeds, h, ds, grid, rays)
        k = 11 + len(seeds)
        return backtrace(*a[:k], ctx.stride, *a[k:], samples=ctx.samples, **kw)
    return (*_integral_backward(ctx, back, grad_x, grad_v, *seeds), None, None, None, None)


class PathTracerC(torch.autograd.Function):
    """``apply(rif, x, v, h, ds, stride, samples) -> (xt, vt, path, count)``: ``trace`` with the path of every ray, ``path``
    of shape ``(samples, n, 3)`` (``path[j]``: every ray at sample j; ``path[:, i]``: ray i's polyline): the marching
    positions in front of iterations 0, stride, 2 stride, ..., ``count`` (int32[n], not differentiable) of them per ray, then
    xt repeated (``samples=None``: ``ceil(max_steps / stride) + 1``, which always ends on xt).  xt, vt and path are
    differentiable w.r.t. ``rif``, ``x`` and ``v``: a field given in torch (an analytic density, an MLP, a grid of another
    resolution sampled with ``grid_sample``), a loss on the curve itself or a quadrature of one's own is a few lines of torch
    on ``path``, and its gradient reaches ``rif`` through the sample positions.  Not in the reference.

    The forward is ``TracerC.trace_path``; backward is ONE ``TracerC.backtrace_path`` launch (plus the zero-fill of the grid
    gradient when ``rif`` requires grad), the derivative of the discrete forward with the iteration counts and ``count`` held
    fixed; ``path``'s gradient arrives dense or not at all.  Options, kept copies, failed rays and dtypes: as for
    OPLTracerC."""

    @staticmethod
    def forward(ctx, rif, x, v, h, ds, stride, samples=None):
        return _path_forward(ctx, "PathTracerC", False, rif, x, v, h, ds, stride, samples)

    @staticmethod
    def backward(ctx, grad_x, grad_v, grad_path, _grad_count=None):
        return _path_backward(ctx, drrt.TracerC().backtrace_path, grad_x, grad_v, grad_path)


class PhasePathTracerC(torch.autograd.Function):
    """``apply(rif, x, v, h, ds, stride, samples) -> (xt, vt, path, vpath, count)``: PathTracerC with the marching velocities
    beside the positions.  ``vpath`` has ``path``'s shape: ``vpath[j]`` is the velocity the march carries in front of
    iteration j stride (``vpath[0] = v``), ``count`` of them per ray, then vt repeated, so ``(path[j], vpath[j])`` is the
    march's state at sample j and ``|vpath[j]|`` the refractive index the ray saw there -- what a chord of ``path`` cannot
    give at a stride above 1.  xt, vt, path and vpath are differentiable w.r.t. ``rif``, ``x`` and ``v``: an integrand that
    depends on the ray's direction (a Doppler or Faraday term with an analytic or MLP flow, an anisotropic emitter) or a
    loss on the direction of a bundle at depth is a few lines of torch.  Not in the reference.

    The forward is ``TracerC.trace_phase``; backward is ONE ``TracerC.backtrace_phase`` launch (plus the zero-fill of the
    grid gradient when ``rif`` requires grad), the derivative of the discrete forward with the iteration counts and
    ``count`` held fixed.  Options, kept copies, failed rays and dtypes: as for PathTracerC."""

    @staticmethod
    def forward(ctx, rif, x, v, h, ds, stride, samples=None):
        return _path_forward(ctx, "PhasePathTracerC", True, rif, x, v, h, ds, stride, samples)

    @staticmethod
    def backward(ctx, grad_x, grad_v, grad_path, grad_vpath, _grad_count=None):
        return _path_backward(ctx, drrt.TracerC().backtrace_phase, grad_x, grad_v, grad_path, grad_vpath)


def _cable_integral_forward(ctx, name, march, profiles, radius, length, x, v, sp, ds):
    """Forward of a fibre march with an integral up to the record: ``march(flat profiles..., radius, length, x, v, sp, ds)
    -> (xt, vt, dist2, integral, rec_steps)`` (``TracerC.trace_cable_opl`` / ``trace_cable_field``) on detached inputs ->
    (xt, vt, dist2, integral), dist2 not differentiable.  apply() takes (*profiles, radius, length, x, v, sp, ds).  When
    any input requires grad ``ctx`` gets a private copy of x (the adjoint replays nothing: of the forward's ray inputs it
    takes x alone; a copy as _keep_rays makes) and the record iterations, and, saved, the profiles and the record."""
    ctx.set_materialize_grads(False)
    ctx.radius, ctx.length, ctx.ds = radius, length, ds
    ix = len(profiles) + 2
    _ray_grad_wanted(ctx, name, ix, ix + 1, x, v)
    xt, vt, dist2, integral, rec = march(*[p.detach().flatten() for p in profiles], radius, length, x.detach(), v.detach(),
                                         sp.detach(), ds)
    if any(ctx.needs_input_grad[i] for i in (*range(len(profiles)), ix, ix + 1)):
        ctx.ray_devices = (x.device, v.device)
        ctx.rays = (x.detach().to(device=xt.device, dtype=torch.float32).clone(), rec)
        ctx.save_for_backward(*profiles, xt, vt)
    ctx.mark_non_differentiable(dist2)
    return xt, vt, dist2, integral


def _cable_integral_backward(ctx, nprof, back, grad_x, grad_v, grad_integral):
    """Backward of the same: ONE ``back(flat profiles..., radius, length, x, xt, vt, rec_steps, grad_x, grad_v,
    grad_integral, ds, wanted per profile..., rays wanted) -> (gradient | None per profile, dpos | None, dvel | None)``
    (``TracerC.backtrace_cable_opl`` / ``backtrace_cable_field``) -> the gradients in apply()'s order."""
    ix = nprof + 2
    want = [ctx.needs_input_grad[i] for i in range(nprof)]
    want_rays = ctx.needs_input_grad[ix] or ctx.needs_input_grad[ix + 1]
    if not (any(want) or want_rays):
        return (None,) * (nprof + 6)
    *profiles, xt, vt = ctx.saved_tensors
    x0, rec = ctx.rays
    *grads, dpos, dvel = back(*[p.detach().flatten() for p in profiles], ctx.radius, ctx.length, x0, xt, vt, rec, grad_x,
                              grad_v, grad_integral, ctx.ds, *want, want_rays)
    dx0 = dpos.to(ctx.ray_devices[0]) if ctx.needs_input_grad[ix] else None
    dv0 = dvel.to(ctx.ray_devices[1]) if ctx.needs_input_grad[ix + 1] else None
    return (*[g.reshape(p.shape) if w else None for g, p, w in zip(grads, profiles, want)], None, None, dx0, dv0, None, None)


class CableOPLTracerC(torch.autograd.Function):
    """``apply(rif (Rr,), radius, length, x, v, sp, ds) -> (xt, vt, dist2, opl)``: the fibre march with the optical path
    length ``opl = sum ds n_k^2`` of every ray up to its closest-approach record; xt, vt and opl are differentiable w.r.t.
    ``rif``, ``x`` and ``v``.  opl is the integral of n along the path (the transit time) when the rays enter with
    |v| = n; rays scaled otherwise (examples/fiber_demo.py divides by the boundary index) get the same sum, which is not
    that integral.  Not in the reference.

    The forward is ``TracerC.trace_cable_opl``, which also returns the iteration of every record; backward is ONE
    ``TracerC.backtrace_cable_opl`` launch (plus the zero-fill of the profile gradient when ``rif`` requires grad) that
    replays nothing, returns dL/drif and the ray gradients from the same reverse march and computes only what is asked
    for.  Unlike BackCableTracerC / ADCableTracerC, whose dL/drif is the reference's ``backtrace_cable`` (the continuous
    adjoint with a backward-escape test and a step bound), this is the derivative of the discrete forward with the
    record's iteration held fixed.  ``dist2`` is not differentiable and ``sp`` gets no gradient.  A private copy of x and
    the record iterations are kept whenever any input requires grad.  fp32 rays only when ray gradients are asked for."""

    @staticmethod
    def forward(ctx, rif, radius, length, x, v, sp, ds):
        return _cable_integral_forward(ctx, "CableOPLTracerC", drrt.TracerC().trace_cable_opl, (rif,), radius, length, x, v,
                                       sp, ds)

    @staticmethod
    def backward(ctx, grad_x, grad_v, grad_dist2, grad_opl):
        return _cable_integral_backward(ctx, 1, drrt.TracerC().backtrace_cable_opl, grad_x, grad_v, grad_opl)


class CableFieldTracerC(torch.autograd.Function):
    """``apply(rif (Rr,), a (Rr,), radius, length, x, v, sp, ds) -> (xt, vt, dist2, tau)``: the fibre march with the line
    integral ``tau = sum ds n_k a_k`` of a second radial profile ``a`` (``rif``'s samples, same radius: a group index, an
    attenuation or a gain) along every ray up to its closest-approach record; xt, vt and tau are differentiable w.r.t.
    ``rif``, ``a``, ``x`` and ``v``.  tau is the integral of a along the path when the rays enter with |v| = n; rays scaled
    otherwise (examples/fiber_demo.py divides by the boundary index) get the same sum, which is not that integral.  With
    ``a = rif`` tau is CableOPLTracerC's opl bit for bit.  Not in the reference.

    The forward is ``TracerC.trace_cable_field``, which also returns the iteration of every record; backward is ONE
    ``TracerC.backtrace_cable_field`` launch (plus one zero-fill per profile gradient asked for) that replays nothing,
    returns dL/drif, dL/da and the ray gradients from the same reverse march and computes only what is asked for.  It is
    the derivative of the discrete forward with the record's iteration held fixed.  ``dist2`` is not differentiable and
    ``sp`` gets no gradient.  A private copy of x and the record iterations are kept whenever any input requires grad.
    fp32 rays only when ray gradients are asked for."""

    @staticmethod
    def forward(ctx, rif, a, radius, length, x, v, sp, ds):
        if a.numel() != rif.numel():
            raise RuntimeError(f"CableFieldTracerC: the second profile must have the {rif.numel()} samples of rif, got "
                               f"{a.numel()}")
        return _cable_integral_forward(ctx, "CableFieldTracerC", drrt.TracerC().trace_cable_field, (rif, a), radius, length,
                                       x, v, sp, ds)

    @staticmethod
    def backward(ctx, grad_x, grad_v, grad_dist2, grad_tau):
        return _cable_integral_backward(ctx, 2, drrt.TracerC().backtrace_cable_field, grad_x, grad_v, grad_tau)


# The reference's enoki-autodiff names for the plane and SDF marches (core/tracer.py:122-234; its ADPlaneTracerC is broken
# upstream) resolve to the adjoint classes so that `autodiff=True` (core/luneburg_opt.py:80-83) keeps working,
# with the documented difference that no gradient flows to x, v through THESE names.  The classes with ray gradients are
# ADTracerC, ADCableTracerC, ADRayPlaneTracerC, ADRaySDFTracerC and ADRayTargetTracerC: the ray-state adjoint of trace is
# exact because its rays end at the sample where they leave the box; the other four replay their forward to find the
# iteration of the recorded sample (and, for the plane, SDF and target marches, which iterations were refracted).
# trace_target has no AD class in the reference; ADRayTargetTracerC also takes the gradient arriving on dist2 and returns
# one for the target.  The fibre march's dist2 still has none (ADCableTracerC ignores it, as the reference does).
ADPlaneTracerC = BackPlaneTracerC
ADSDFTracerC = BackSDFTracerC
