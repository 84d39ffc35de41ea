"""Differentiable float64 torch restatements of trace with each integral operator's output -- TEST INFRASTRUCTURE ONLY.

One loop (`_march`): oracle/torch_ad.trace's (its eval_grad / inbounds / escaped), array at a time.  The march of the library
ends a ray at the iteration that flags it; the loop here goes on while any ray marches, so every operator masks a flagged
ray's later samples with `esc` (they are masked to 0 outside the box anyway, but a ray flagged inside it is not).  `steps` is
the per-ray iteration count at which each ray was flagged (max_steps where it never was).

An operator hands the loop up to three closures, called in this order within an iteration, and keeps its own sums:
  front(it, x, n, inside, esc)   the sample x_k in front of the update, n its index under the mask `inside`
  kicked(v)                      v_{k+1}, the velocity that carries the ray from x_k to x_{k+1}
  moved(x)                       x_{k+1}
The order in which an operator creates its torch operations is part of the yardstick (autograd accumulates in it)."""
import torch

from oracle.torch_ad import escaped, eval_grad, inbounds


def _march(rif, pos, vel, h, ds, front=None, kicked=None, moved=None):
    """-> (xt, vt, steps)."""
    shape = rif.shape
    max_steps = int(4 * h * max(shape) / ds)
    x, v = pos.clone(), vel.clone()
    xt, vt = pos.clone(), vel.clone()
    steps = torch.full((pos.shape[0],), max_steps, dtype=torch.int64, device=pos.device)
    inside = inbounds(shape, h, x)
    esc = torch.zeros_like(inside)
    for it in range(max_steps):
        n, g = eval_grad(rif, x, h, inside)
        if front:
            front(it, x, n, inside, esc)
        v = v + (ds * n)[:, None] * g
        if kicked:
            kicked(v)
        x = x + ds * v
        if moved:
            moved(x)
        cur_inside = inbounds(shape, h, x)
        cross = inside & ~cur_inside
        now = (cross | escaped(shape, h, x, v)) & ~esc
        steps = torch.where(now, torch.full_like(steps, it + 1), steps)
        esc = esc | now
        xt = torch.where(cross[:, None], x, xt)
        vt = torch.where(cross[:, None], v, vt)
        if bool(esc.all()):
            break
        inside = cur_inside
    if not bool(esc.all()):
        xt = torch.where(esc[:, None], xt, x)
    return xt, vt, steps


def _zeros(pos):
    return torch.zeros(pos.shape[0], dtype=pos.dtype, device=pos.device)


def trace_opl(rif, pos, vel, h, ds):
    """``opl += ds n^2``.  Differentiable w.r.t. rif, pos, vel.  -> (xt, vt, opl, steps)."""
    opl = _zeros(pos)

    def front(it, x, n, inside, esc):
        nonlocal opl
        opl = opl + torch.where(esc, torch.zeros_like(n), ds * n * n)

    xt, vt, steps = _march(rif, pos, vel, h, ds, front)
    return xt, vt, opl, steps


def trace_field(rif, field, pos, vel, h, ds):
    """``tau += ds n a``, `a` the sample of `field` under the same `inside` mask as `n`.  Differentiable w.r.t. rif, field,
    pos, vel.  -> (xt, vt, tau, steps)."""
    assert field.shape == rif.shape
    tau = _zeros(pos)

    def front(it, x, n, inside, esc):
        nonlocal tau
        a, _ = eval_grad(field, x, h, inside)
        tau = tau + torch.where(esc, torch.zeros_like(n), ds * n * a)

    xt, vt, steps = _march(rif, pos, vel, h, ds, front)
    return xt, vt, tau, steps


def trace_emission(rif, emission, absorption, pos, vel, h, ds):
    """``rad += exp(-tau) ds n e`` and then ``tau += ds n a``, `e` and `a` sampled as trace_field's `a`, the exponential
    torch.exp.  Differentiable w.r.t. rif, emission, absorption, pos, vel.  -> (xt, vt, rad, tau, steps)."""
    assert emission.shape == rif.shape and absorption.shape == rif.shape
    tau = _zeros(pos)
    rad = torch.zeros_like(tau)

    def front(it, x, n, inside, esc):
        nonlocal rad, tau
        e, _ = eval_grad(emission, x, h, inside)
        a, _ = eval_grad(absorption, x, h, inside)
        rad = rad + torch.where(esc, torch.zeros_like(n), torch.exp(-tau) * ds * n * e)
        tau = tau + torch.where(esc, torch.zeros_like(n), ds * n * a)

    xt, vt, steps = _march(rif, pos, vel, h, ds, front)
    return xt, vt, rad, tau, steps


def trace_vector(rif, vfield, pos, vel, h, ds, extent=False):
    """``circ += ds u(x_k) . v_{k+1}``: `u` the samples of the three component planes ``vfield[c]`` (shape
    ``(3,) + rif.shape``; plane c pairs with component c of pos / vel) under the same `inside` mask as `n`.  Differentiable
    w.r.t. rif, vfield, pos, vel.  -> (xt, vt, circ, steps, S), ``S = sum ds (|ux vx| + |uy vy| + |uz vz|)`` the per-ray scale
    of the same summands: circ cancels, S does not, so an error of circ is measured against S.  With `extent` a sixth
    result: per ray and axis, the largest |x_c| among the positions x_k, x_{k+1} of the iterations that sampled inside the
    box (0 for a ray that never did)."""
    assert tuple(vfield.shape) == (3,) + tuple(rif.shape)
    circ = _zeros(pos)
    scale = torch.zeros_like(circ)
    reach = torch.zeros_like(pos)
    u = zero = flagged = live = None

    def front(it, x, n, inside, esc):
        nonlocal u, zero, flagged, live, reach
        u = torch.stack([eval_grad(vfield[c], x, h, inside)[0] for c in range(3)], 1)
        zero, flagged, live = torch.zeros_like(n), esc, (inside & ~esc)[:, None]
        reach = torch.where(live, torch.maximum(reach, x.detach().abs()), reach)      # no graph: its place is free

    def kicked(v):
        nonlocal circ, scale
        term = u * v
        circ = circ + torch.where(flagged, zero, ds * term.sum(1))
        scale = scale + torch.where(flagged, zero, ds * term.abs().sum(1))

    def moved(x):
        nonlocal reach
        reach = torch.where(live, torch.maximum(reach, x.detach().abs()), reach)

    xt, vt, steps = _march(rif, pos, vel, h, ds, front, kicked, moved)
    if extent:
        return xt, vt, circ, steps, scale.detach(), reach
    return xt, vt, circ, steps, scale.detach()


def trace_path(rif, pos, vel, h, ds, stride, samples, velocities=False):
    """Records the marching position x in front of every iteration that is a multiple of `stride`, `samples` = M entries at
    most, and with `velocities` the velocity v in front of it beside x: vel for iteration 0 and the `kicked` value of
    iteration k - 1 behind it.  The per-ray count ``min(M, ceil(steps / stride))`` is known behind the loop; the entries at
    and behind it are replaced by xt (vt) with ``torch.where``, so autograd sees xt (vt) there and x_{j stride}
    (v_{j stride}) in front of it.  The loop ends when every ray is flagged; the entries it has not reached then belong to no
    ray's samples (j stride >= steps for every ray) and are padding.  Differentiable w.r.t. rif, pos, vel.
    -> (xt, vt, path (samples, n, 3)[, vpath (samples, n, 3)], count, steps)."""
    rec, vrec = [], []
    carried = vel

    def front(it, x, n, inside, esc):
        if it % stride == 0 and len(rec) < samples:
            rec.append(x)
            vrec.append(carried)

    def kicked(v):
        nonlocal carried
        carried = v

    xt, vt, steps = _march(rif, pos, vel, h, ds, front, kicked if velocities else None)
    count = torch.clamp((steps + stride - 1) // stride, max=samples)
    series = []
    for recorded, pad in ((rec, xt), (vrec, vt))[:2 if velocities else 1]:
        rows = []
        for j in range(samples):
            rows.append(torch.where((j < count)[:, None], recorded[j], pad) if j < len(rec) else pad)
        series.append(torch.stack(rows))
    return (xt, vt, *series, count, steps)


def trace_phase(rif, pos, vel, h, ds, stride, samples):
    """trace_path with both series -> (xt, vt, path, vpath, count, steps)."""
    return trace_path(rif, pos, vel, h, ds, stride, samples, velocities=True)
