"""Counterpart of the part of the reference's ``core/sensor.py`` that directly follows the march:
``trace_rays_to_plane`` (``:195-202``), ``get_tan_vecs`` (``:219-231``), ``generate_sensor``
(``:5-28``), the differentiable 2-D image splat used by the image / Luneburg experiments
(``core/image_opt.py:99-101``, ``core/luneburg_opt.py:121-123``), and ``generate_inf_sensor`` (``:31-53``),
the far-field (direction histogram) sensor of the image experiments (``core/image_opt.py:116``).

``get_sdf_vals_near`` / ``get_sdf_vals_far`` (``:102-138``) sample a texture at the same sensor coordinates (fused kernels).

``generate_sensor`` keeps the reference's signature; on ``cuda`` (ROCm) tensors it runs the fused
HIP kernels (``csrc/drrt_sensor.hip``: ray -> plane -> sensor frame -> 16 tent taps -> atomics, and
the analytic backward that yields ``(grad_x, grad_v)`` directly) instead of ~20 (N,16)-sized torch
temporaries + ``index_put_``.  There is no CPU compute path: CPU tensors raise.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from ._lib import _p, _stream
from .drrt import _f32


def _ray_grads(x_: torch.Tensor):
    """The (grad_x, grad_v) outputs of a backward kernel."""
    return torch.empty_like(x_), torch.empty_like(x_)


class _RaysToPlane(torch.autograd.Function):

    @staticmethod
    def forward(ctx, x, v, p, n):
        dev = x.device
        with torch.cuda.device(dev):
            x_, v_, p_, n_ = (_f32(t, dev) for t in (x, v, p, n))
            stride = 3 if p_.shape[0] > 1 else 0
            xo = torch.empty_like(x_)
            _lib.check(_lib.load().drrt_rays_to_plane_f32(x_.shape[0], _p(x_), _p(v_), _p(p_), _p(n_), stride, _p(xo),
                                                          _stream(dev)))
        ctx.save_for_backward(x_, v_, p_, n_)
        ctx.stride = stride
        return xo

    @staticmethod
    def backward(ctx, g):
        x_, v_, p_, n_ = ctx.saved_tensors
        dev = x_.device
        with torch.cuda.device(dev):
            g_ = _f32(g, dev)
            gx, gv = _ray_grads(x_)
            _lib.check(_lib.load().drrt_rays_to_plane_bwd_f32(x_.shape[0], _p(x_), _p(v_), _p(p_), _p(n_), ctx.stride,
                                                              _p(g_), _p(gx), _p(gv), _stream(dev)))
        return gx, gv, None, None


def trace_rays_to_plane(rays, plane):
    """core/sensor.py:195-202: intersect the rays with their planes, ``(x + t v, v)`` with ``t = n.(p - x) / n.v``.

    The reference writes the two dot products as ``torch.matmul`` on (N,1,3) x (N,3,1) operands -- a batched matmul of
    N one-by-three products, ~25 ms forward + ~55 ms backward for 1M rays on this GPU, 15x the march.  For fp32 (N,3)
    rays on the cuda (ROCm) device with (N,3) or (1,3) planes that are constants (they are in every experiment of the
    reference) this runs one fused HIP kernel each way; any other input takes the reference's torch expressions."""
    x, v = rays
    p, n = plane
    fused = (x.is_cuda and x.dtype == torch.float32 and v.dtype == torch.float32 and x.dim() == 2 and x.shape[1] == 3
             and v.shape == x.shape and p.dim() == 2 and n.dim() == 2 and p.shape == n.shape and p.shape[1] == 3
             and p.shape[0] in (1, x.shape[0]) and not p.requires_grad and not n.requires_grad)
    if fused:
        return _RaysToPlane.apply(x, v, p, n), v
    t = torch.matmul(n[:, None, :], (p - x)[:, :, None]).squeeze(2)
    t = t / torch.matmul(n[:, None, :], v[:, :, None]).squeeze(2)
    return (x + t * v), v


def get_tan_vecs(n, t=None):
    """core/sensor.py:219-231."""
    if t is None:
        t2 = torch.zeros_like(n)
        if torch.abs(n)[0, -1] > 0.001:
            t2[0, 0] = 1
        else:
            t2[0, -1] = 1
    else:
        t2 = t
    t1 = torch.cross(n, t2, dim=1)
    return t1, t2


def _vec3(t: torch.Tensor):
    v = t.detach().reshape(-1)[:3].to(torch.float32).cpu().tolist()
    return (C.c_float * 3)(*v)


def _single_plane(*vecs) -> None:
    """The fused sensor operators take ONE plane / frame per call (the reference calls them once per view with (1, 3)
    tensors, core/image_opt.py:99-119).  A (N, 3) tensor whose rows differ -- per-ray planes -- would silently use row 0:
    refuse it (``trace_rays_to_plane`` is the operator that takes per-ray planes)."""
    from .drrt import _capturing
    if _capturing():               # the row comparison reads a device value on the host: not capturable; a captured call
        return                     # has been checked when it ran eagerly before the capture
    for t in vecs:
        if isinstance(t, torch.Tensor) and t.dim() == 2 and t.shape[0] > 1 and not bool((t == t[:1]).all()):
            raise RuntimeError("this sensor operator takes one plane / frame per call (rows differ); split the rays by "
                               "view as the reference does (core/image_opt.py:99-119)")


def _frame(dev, p, n, t1, t2):
    """The sensor frame of a call -> (frame12, host): when every given vector is a tensor on `dev` (the reference keeps
    its planes there, core/image_opt.py:88-119) they are packed into ONE 12-float device tensor (p, n, t1, t2; zeros for
    p / n of the far field) for the *_dframe entries -- no copy back to the host, hence no device sync per call;
    otherwise host float[3] arrays for the plain entries."""
    given = [t for t in (p, n, t1, t2) if t is not None]
    if all(isinstance(t, torch.Tensor) and t.is_cuda and t.device == dev for t in given):
        zero = None
        parts = []
        for t in (p, n, t1, t2):
            if t is None:
                zero = torch.zeros(3, dtype=torch.float32, device=dev) if zero is None else zero
                parts.append(zero)
            else:
                parts.append(t.detach().reshape(-1)[:3].to(torch.float32))
        return torch.cat(parts).contiguous(), None
    return None, tuple(_vec3(t) for t in given)


def _energy(e, nr: int, dev):
    """The `e` of a splat -> (per-ray tensor or None, scalar): one entry per ray, or one value for all of them."""
    if isinstance(e, torch.Tensor) and e.numel() > 1:
        e_ = _f32(e, dev).reshape(-1).contiguous()
        if e_.numel() != nr:
            raise RuntimeError("e must be a scalar or have one entry per ray")
        return e_, 0.0
    return None, float(e)


def _call(entry: str, head, fdev, frame, *tail) -> None:
    """One sensor entry, ``entry(*head, <frame>, *tail, stream)``: `entry` names it with ``{}`` where ``_dframe`` goes, and
    that twin is the one called when _frame() packed the frame on the device (``fdev``).  Tensors go in as their device
    pointers (None as NULL); `head` is (n, rays ...), and the stream is the current one of the rays' device."""
    fn = getattr(_lib.load(), entry.format("" if fdev is None else "_dframe"))
    args = (*head, *(frame if fdev is None else (fdev,)), *tail)
    _lib.check(fn(*(_p(a) if isinstance(a, torch.Tensor) else a for a in args), _stream(head[1].device)))


class _SensorSplat(torch.autograd.Function):

    @staticmethod
    def forward(ctx, x, v, e, p, n, t1, t2, res, span):
        if not x.is_cuda:
            raise RuntimeError("generate_sensor expects tensors on the cuda (ROCm) device (no CPU path)")
        dev = x.device
        with torch.cuda.device(dev):
            x_, v_ = _f32(x, dev), _f32(v, dev)
            e_, e_s = _energy(e, x_.shape[0], dev)
            img = torch.empty(int(res), int(res), dtype=torch.float32, device=dev)
            fdev, frame = _frame(dev, p, n, t1, t2)
            _call("drrt_sensor_splat{}_f32", (x_.shape[0], x_, v_, e_, e_s), fdev, frame, int(res), float(span), img, 0)
        ctx.saved = (x_, v_, e_, e_s, fdev, frame, int(res), float(span))
        return img

    @staticmethod
    def backward(ctx, grad_img):
        x_, v_, e_, e_s, fdev, frame, res, span = ctx.saved
        with torch.cuda.device(x_.device):
            g = _f32(grad_img, x_.device)
            gx, gv = _ray_grads(x_)
            _call("drrt_sensor_splat{}_bwd_f32", (x_.shape[0], x_, v_, e_, e_s), fdev, frame, res, span, g, gx, gv)
        return gx, gv, None, None, None, None, None, None, None


def _refuse_grad(op, **inputs):
    """The fused splats return gradients of the rays only.  In the reference generate_sensor / generate_inf_sensor are
    plain torch, so a per-ray `e` or a plane that requires grad gets a gradient there: refuse such an input instead of
    dropping its gradient silently (as _TexGet does for the texture)."""
    if not torch.is_grad_enabled():
        return
    for name, t in inputs.items():
        if isinstance(t, torch.Tensor) and t.requires_grad:
            raise RuntimeError(f"{op}: the fused operator is not differentiable w.r.t. `{name}`; pass {name}.detach() "
                               f"(the reference experiments compute it under torch.no_grad())")


def generate_sensor(rays, e, plane, res, span, tangent=None):
    """core/sensor.py:5-28: image (res, res) of the rays splatted onto the sensor plane
    (p, n given as (1,3) tensors, one plane per call as in the reference); differentiable w.r.t.
    the rays only (an `e`, plane or tangent that requires grad raises)."""
    x, v = rays
    p, n = plane
    _refuse_grad("generate_sensor", e=e, p=p, n=n, tangent=tangent)
    t1, t2 = get_tan_vecs(n, tangent)
    return _SensorSplat.apply(x, v, e, p, n, t1, t2, res, span)


class _FarSensorSplat(torch.autograd.Function):

    @staticmethod
    def forward(ctx, v, e, t1, t2, res, ang_cut):
        if not v.is_cuda:
            raise RuntimeError("generate_inf_sensor expects tensors on the cuda (ROCm) device (no CPU path)")
        dev = v.device
        with torch.cuda.device(dev):
            v_ = _f32(v, dev)
            e_, e_s = _energy(e, v_.shape[0], dev)
            img = torch.empty(int(res), int(res), dtype=torch.float32, device=dev)
            fdev, frame = _frame(dev, None, None, t1, t2)
            _call("drrt_sensor_far_splat{}_f32", (v_.shape[0], v_, e_, e_s), fdev, frame, int(res), float(ang_cut), img, 0)
        ctx.saved = (v_, e_, e_s, fdev, frame, int(res), float(ang_cut))
        return img

    @staticmethod
    def backward(ctx, grad_img):
        v_, e_, e_s, fdev, frame, res, ang_cut = ctx.saved
        with torch.cuda.device(v_.device):
            g = _f32(grad_img, v_.device)
            gx, gv = _ray_grads(v_)
            _call("drrt_sensor_far_splat{}_bwd_f32", (v_.shape[0], v_, e_, e_s), fdev, frame, res, ang_cut, g, gx, gv)
        return gv, None, None, None, None, None


def generate_inf_sensor(rays, e, plane, res, angle_span=120, tangent=None):
    """core/sensor.py:31-53: far-field image (res, res) -- the normalised ray directions splatted in the sensor
    frame over [-ang_cut, ang_cut]^2, ang_cut = sin(angle_span / 2); differentiable w.r.t. the directions (the
    positions and the plane point do not enter, as in the reference; an `e`, normal or tangent that requires grad
    raises)."""
    x, v = rays
    p, n = plane
    _refuse_grad("generate_inf_sensor", e=e, n=n, tangent=tangent)
    ang_cut = float(torch.sin(0.5 * torch.deg2rad(torch.tensor(float(angle_span), dtype=torch.float32))))   # :38
    t1, t2 = get_tan_vecs(n, tangent)
    return _FarSensorSplat.apply(v, e, t1, t2, res, ang_cut)


MAX_CHANNELS = 32          # kMaxChannels of csrc/drrt_sensor.hip


def _radiance(op, rad, nr: int):
    """The `rad` of a radiance splat -> ((N, C) view, whether it came as (N,)): one value per ray, or one per ray and
    channel (colour or spectral bands, absorption lines, time gates built from an optical path length, ...)."""
    if not isinstance(rad, torch.Tensor) or rad.dim() == 0:
        raise RuntimeError(f"{op}: `rad` is a tensor with one value per ray, (N,), or per ray and channel, (N, C); for "
                           f"one energy shared by all rays use generate_sensor / generate_inf_sensor")
    if rad.dim() > 2 or rad.shape[0] != nr:
        raise RuntimeError(f"{op}: `rad` must have shape (N,) or (N, C) for the N = {nr} rays, got {tuple(rad.shape)}")
    if rad.dim() == 2 and not 1 <= rad.shape[1] <= MAX_CHANNELS:
        raise RuntimeError(f"{op}: `rad` must have 1 to {MAX_CHANNELS} channels, got {rad.shape[1]}")
    return (rad[:, None] if rad.dim() == 1 else rad), rad.dim() == 1


class _RadianceSplat(torch.autograd.Function):
    """splat_radiance / splat_radiance_far (`far`): k_sensor_radiance forward, and ONE launch of k_sensor_radiance_bwd
    that computes the gradients ctx.needs_input_grad asks for (the others go in as NULL and are not computed)."""

    @staticmethod
    def forward(ctx, x, v, rad, p, n, t1, t2, res, span, far):
        op = "splat_radiance_far" if far else "splat_radiance"
        if not v.is_cuda:
            raise RuntimeError(f"{op} expects tensors on the cuda (ROCm) device (no CPU path)")
        _single_plane(p, n)
        dev = v.device
        with torch.cuda.device(dev):
            x_, v_, rad_ = (_f32(t, dev) for t in (x, v, rad))
            nr, nc = rad_.shape
            img = torch.empty(nc, int(res), int(res), dtype=torch.float32, device=dev)
            fdev, frame = _frame(dev, None if far else p, None if far else n, t1, t2)
            head = (nr, v_, rad_, nc) if far else (nr, x_, v_, rad_, nc)
            entry = "drrt_sensor_radiance_far{}" if far else "drrt_sensor_radiance{}"
            _call(entry + "_f32", head, fdev, frame, int(res), float(span), img, 0)
        ctx.saved = (entry, head, fdev, frame, int(res), float(span))
        return img

    @staticmethod
    def backward(ctx, grad_img):
        entry, head, fdev, frame, res, span = ctx.saved
        v_, rad_ = head[-3], head[-2]
        want_x, want_v, want_rad = ctx.needs_input_grad[:3]
        with torch.cuda.device(v_.device):
            g = _f32(grad_img, v_.device)
            gx = torch.empty_like(v_) if want_x and len(head) == 5 else None      # the far field does not read x
            gv = torch.empty_like(v_) if want_v else None
            grad = torch.empty_like(rad_) if want_rad else None
            _call(entry + "_bwd_f32", head, fdev, frame, res, span, g, grad, gx, gv)
        return gx, gv, grad, None, None, None, None, None, None, None


def _splat_radiance(op, far, rays, rad, plane, res, span, tangent):
    x, v = rays
    p, n = plane
    _refuse_grad(op, **({"n": n} if far else {"p": p, "n": n}), tangent=tangent)
    rad2, flat = _radiance(op, rad, v.shape[0])
    t1, t2 = get_tan_vecs(n, tangent)
    img = _RadianceSplat.apply(x, v, rad2, p, n, t1, t2, res, span, far)
    return img[0] if flat else img


def splat_radiance(rays, rad, plane, res, span, tangent=None):
    """generate_sensor for a per-ray, per-channel energy, differentiable w.r.t. the rays AND `rad`: `rad` (N,) gives the
    image (res, res), `rad` (N, C) with 1 <= C <= 32 gives (C, res, res), whose channel c is
    ``generate_sensor(rays, rad[:, c], plane, res, span, tangent)`` -- same plane intersection, frame, 4 x 4 tent taps,
    normalisation and foreshortening |v.n|.  The channels of a ray share its landing point and its 16 weights, which one
    fused HIP kernel forms once (csrc/drrt_sensor.hip k_sensor_radiance); the backward is one launch that computes the
    gradients asked for.  E.g. a shadowgraph through an absorbing, refracting volume: ``rad = exp(-tau)`` with ``tau``
    from FieldIntegralTracerC -- the image then depends on the volume through the landing point and through the weight.
    A plane or tangent that requires grad raises, as in generate_sensor."""
    return _splat_radiance("splat_radiance", False, rays, rad, plane, res, float(span), tangent)


def splat_radiance_far(rays, rad, plane, res, angle_span=120, tangent=None):
    """generate_inf_sensor for a per-ray, per-channel energy (see splat_radiance): the far-field image(s) of the
    normalised directions, differentiable w.r.t. the directions and `rad`; the positions do not enter."""
    ang_cut = float(torch.sin(0.5 * torch.deg2rad(torch.tensor(float(angle_span), dtype=torch.float32))))
    return _splat_radiance("splat_radiance_far", True, rays, rad, plane, res, ang_cut, tangent)


class _TexGet(torch.autograd.Function):

    @staticmethod
    def forward(ctx, x, v, tex, p, n, t1, t2, span, mode):
        if not x.is_cuda:
            raise RuntimeError("get_sdf_vals_* expect tensors on the cuda (ROCm) device (no CPU path)")
        if isinstance(tex, torch.Tensor) and tex.requires_grad:
            # the reference's Grid.Get path is differentiable w.r.t. the texture; this fused operator only returns the
            # gradients of the rays -- say so instead of handing back a silent zero
            raise RuntimeError("get_sdf_vals_*: the fused operator is not differentiable w.r.t. the texture; pass "
                               "d_tex.detach() (the experiments optimise the volume, not the measured texture)")
        _single_plane(p, n)            # (t1, t2 of get_tan_vecs are set in row 0 only, as in the reference)
        dev = x.device
        with torch.cuda.device(dev):
            x_, v_, tex_ = (_f32(t, dev) for t in (x, v, tex))
            if tex_.dim() != 2 or tex_.shape[0] != tex_.shape[1]:
                raise RuntimeError("the texture must be square (the reference clips both axes with res[0])")
            fdev, frame = _frame(dev, p, n, t1, t2)
            f = torch.empty(x_.shape[0], dtype=torch.float32, device=dev)
            _call("drrt_sensor_tex_get{}_f32", (x_.shape[0], x_, v_), fdev, frame, tex_, int(tex_.shape[0]), float(span),
                  int(mode), f)
        ctx.saved = (x_, v_, tex_, fdev, frame, float(span), int(mode))
        return f

    @staticmethod
    def backward(ctx, grad_f):
        x_, v_, tex_, fdev, frame, span, mode = ctx.saved
        with torch.cuda.device(x_.device):
            g = _f32(grad_f, x_.device)
            gx, gv = _ray_grads(x_)
            _call("drrt_sensor_tex_get{}_bwd_f32", (x_.shape[0], x_, v_), fdev, frame, tex_, int(tex_.shape[0]), span, mode,
                  g, gx, gv)
        return gx, gv, None, None, None, None, None, None, None


def get_sdf_vals_near(rays, d_tex, plane, span, tangent=None):
    """core/sensor.py:102-119: the (res, res) texture ``d_tex`` (e.g. the signed distance to a measured caustic)
    sampled at the points where the rays meet the sensor plane (Grid.Get's radial-tent interpolant); differentiable
    w.r.t. the rays.  One fused HIP kernel each way (plane intersection, sensor frame, 16 taps)."""
    x, v = rays
    p, n = plane
    t1, t2 = get_tan_vecs(n, tangent)
    return _TexGet.apply(x, v, d_tex, p, n, t1, t2, span, 0)


def get_sdf_vals_far(rays, d_tex, plane, ang_span, tangent=None):
    """core/sensor.py:122-138: the texture sampled at the rays' directions projected on the sensor frame,
    ``v . T + ang_cut`` with ``ang_cut = sin(ang_span / 2)`` (the direction as it is, not normalised -- as written)."""
    x, v = rays
    p, n = plane
    ang_cut = float(torch.sin(0.5 * torch.deg2rad(torch.tensor(float(ang_span), dtype=torch.float32))))
    t1, t2 = get_tan_vecs(n, tangent)
    return _TexGet.apply(x, v, d_tex, p, n, t1, t2, 2.0 * ang_cut, 1)

