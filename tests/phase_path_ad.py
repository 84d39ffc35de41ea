"""Differentiable float64 torch restatement of trace with both series of trace_phase -- TEST INFRASTRUCTURE ONLY.

integral_ad._march with its `front` and `kicked` closures: the velocity in front of iteration k is vel for k = 0 and the
`kicked` value of iteration k - 1 behind it, so `front` records (x_k, v_k) where integral_ad.trace_path records x_k.  The
entries at and behind the per-ray count are replaced by (xt, vt) with ``torch.where``, as there."""
import torch

from integral_ad import _march


def trace_phase(rif, pos, vel, h, ds, stride, samples):
    """-> (xt, vt, path (samples, n, 3), vpath (samples, n, 3), count, steps).  Differentiable w.r.t. rif, pos, vel."""
    rec, vrec = [], []
    carried = vel

    def front(it, x, n, inside, esc):
        if it % stride == 0 and len(rec) < samples:
            rec.append(x)
            vrec.append(carried)

    def kicked(v):
        nonlocal carried
        carried = v

    xt, vt, steps = _march(rif, pos, vel, h, ds, front, kicked)
    count = torch.clamp((steps + stride - 1) // stride, max=samples)
    rows, vrows = [], []
    for j in range(samples):
        live = (j < count)[:, None]
        rows.append(torch.where(live, rec[j], xt) if j < len(rec) else xt)
        vrows.append(torch.where(live, vrec[j], vt) if j < len(rec) else vt)
    return xt, vt, torch.stack(rows), torch.stack(vrows), count, steps
