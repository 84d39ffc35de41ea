"""What test_vector_integral.py and test_vector_fuzz.py share: the vector field of a case, the host build's calls, the float64
referee and float32 yardstick of trace_vector (once per key, handed out unchanged), the rows they are compared by, and the
GPU calls.  A plain module: no fixtures, no tests."""
import numpy as np
import torch

import cases
import integral_ad
import integral_common as IC
import integral_fuzz_common as IF
import integral_host as OH
from raygrad_common import TIE_TOL, _t, rel_err

ATOMIC_TOL = 2e-5       # grid gradients, kernel vs host build: only the order of the atomic sums differs
PLANES = ("dL/dux", "dL/duy", "dL/duz")
MODES = ("all", "noray")          # every seed set; no seeds on (xt, vt)


def make_vfield(shape, seed):
    """Seeded, fp32, smooth, sign-changing, shape (3,) + shape: component c is 0.4 (mean of sines along the three axes, with
    periods and phases of its own, less its average over the grid, so that it changes sign on a 2 x 3 x 3 grid too) + 0.05
    (uniform noise - 1/2).  The three components differ and none is symmetric under a permutation of the axes."""
    D, H, W = shape
    z, y, x = np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing="ij")
    rng = np.random.default_rng(seed + 41)
    out = []
    for c, (a, b, g) in enumerate(((0.9, 0.5, 1.3), (0.4, 1.1, 0.7), (1.2, 0.8, 0.35))):
        s = (np.sin(a * x + 0.3 + c) + np.sin(b * y + 1.1 - 0.5 * c) + np.sin(g * z + 2.0 + 0.7 * c)) / 3.0
        out.append(0.4 * (s - s.mean()) + 0.05 * (rng.random(shape) - 0.5))
    u = np.stack(out).astype(np.float32)
    assert (u.min((1, 2, 3)) < -0.02).all() and (u.max((1, 2, 3)) > 0.02).all()
    return u


def host_forward(s):
    return OH.trace_vector(s["rif"], s["vfield"], s["res"], s["pos"], s["vel"], s["h"], s["ds"])


def host_back(s, k, dx, dv, dcirc, sel=slice(None), **kw):
    pick = lambda a: None if a is None else a[sel]      # noqa: E731
    return OH.backtrace_vector(s["rif"], s["vfield"], s["res"], s["pos"][sel], s["vel"][sel], k["xt"][sel], k["vt"][sel],
                               k["steps"][sel], pick(dx), pick(dv), pick(dcirc), s["h"], s["ds"], **kw)


def _T(a, dtype):
    return torch.tensor(np.asarray(a), dtype=dtype)


_yards = {}


def yard(oracle, s, key):
    """-> dict(k, ms, compared, scaled, failed, circ64, circ32, S): the host fp32 forward, and the rays that are tie-free for
    the product (tests/integral_common.py::reference under `key`: the fp32 host build and the fp64 oracle leave on the same
    iteration with exit samples within TIE_TOL) and for the yardstick (the same between the float32 and the float64 runs of
    tests/integral_ad).  `scaled`: compared rays with S > 0.  `ad`: filled by `autograd`."""
    if key in _yards:
        return _yards[key]
    k = host_forward(s)
    _, tie_prod, _, ms = IC.reference(oracle, s, key)
    with torch.no_grad():
        lo, hi = (integral_ad.trace_vector(*(_T(s[name], dt) for name in ("rif", "vfield", "pos", "vel")), s["h"], s["ds"])
                  for dt in (torch.float32, torch.float64))
    ms_ad = int(4 * s["h"] * max(s["rif"].shape) / s["ds"])
    close = lambda a, b: (a.double() - b).abs().max(1).values <= TIE_TOL      # noqa: E731
    tie_ref = ((lo[3] < ms_ad) & (lo[3] == hi[3]) & close(lo[0], hi[0]) & close(lo[1], hi[1])).numpy()
    compared = tie_prod & tie_ref
    assert np.array_equal(hi[3].numpy()[compared], k["steps"][compared].astype(np.int64))
    S = hi[4].numpy()
    _yards[key] = dict(k=k, ms=ms, compared=compared, scaled=compared & (S > 0), failed=k["steps"] >= ms,
                       circ64=hi[2].numpy(), circ32=lo[2].numpy().astype(np.float64), S=S, ad={})
    return _yards[key]


def seeds_of(s, mode, compared):
    """(dx, dv, dcirc): the seeds of a mode, those of the rays that are not compared zeroed, (dx, dv) zero for "noray"."""
    z = compared[:, None] if mode == "all" else np.zeros((len(compared), 1), bool)
    return (s["dx"] * z).astype(np.float32), (s["dv"] * z).astype(np.float32), (s["dcirc"] * compared).astype(np.float32)


def autograd(oracle, s, key):
    """{dtype: {mode: (dL/drif, dL/du as (3, nvox), dpos, dvel)}} for torch.float64 and torch.float32: torch.autograd of
    L = <dx, xt> + <dv, vt> + <dcirc, circ> through tests/integral_ad, one forward and one backward per mode.  Only the compared
    rays are marched: the seeds of the others are zero; their rows of the per-ray results are zero."""
    y = yard(oracle, s, key)
    if y["ad"]:
        return y["ad"]
    idx = np.nonzero(y["compared"])[0]
    n = len(s["pos"])

    def full(a):
        out = np.zeros((n, 3), a.dtype)
        out[idx] = a
        return out
    for dt in (torch.float64, torch.float32):
        leaves = [_T(s[name], dt).requires_grad_(True) for name in ("rif", "vfield")] + \
                 [_T(s[name][idx], dt).requires_grad_(True) for name in ("pos", "vel")]
        outs = integral_ad.trace_vector(*leaves, s["h"], s["ds"])[:3]
        r = {}
        for mode in MODES:
            L = sum((o * _T(w[idx], dt)).sum() for o, w in zip(outs, seeds_of(s, mode, y["compared"])))
            gr, gu, gp, gv = torch.autograd.grad(L, leaves, retain_graph=True)
            r[mode] = (gr.numpy().reshape(-1), gu.numpy().reshape(3, -1), full(gp.numpy()), full(gv.numpy()))
        y["ad"][dt] = r
    return y["ad"]


def circ_rows(y, circ):
    """[(quantity, e_prod, e_ref, cap)]: the largest |circ - circ64| / S over the compared rays with S > 0."""
    m = y["scaled"]
    err = lambda x: float((np.abs(np.asarray(x, np.float64) - y["circ64"])[m] / y["S"][m]).max())      # noqa: E731
    return [("circ", err(circ), err(y["circ32"]), IF.CAPS["out"])]


def adjoint_rows(oracle, s, key, mode, dpos, dvel, grad, grad_vfield):
    """[(quantity, e_prod, e_ref, cap, |gradient|)] against float64 autograd: the largest rel_err of (dpos, dvel) over the
    compared rays, the rel-L2 of dL/drif and of each plane of dL/du."""
    y, ad = yard(oracle, s, key), autograd(oracle, s, key)
    hi, lo = ad[torch.float64][mode], ad[torch.float32][mode]
    cmp_ = y["compared"]
    rows = [("rays", float(rel_err(dpos, dvel, hi[2], hi[3])[cmp_].max()),
             float(rel_err(lo[2], lo[3], hi[2], hi[3])[cmp_].max()), IF.CAPS["rays"],
             float(np.abs(np.concatenate([hi[2], hi[3]], 1)[cmp_]).max())),
            ("dL/drif", cases.rel_l2(grad, hi[0]), cases.rel_l2(lo[0], hi[0]), IF.CAPS["grid"], float(np.linalg.norm(hi[0])))]
    gv = np.asarray(grad_vfield).reshape(3, -1)
    for c, label in enumerate(PLANES):
        rows.append((label, cases.rel_l2(gv[c], hi[1][c]), cases.rel_l2(lo[1][c], hi[1][c]), IF.CAPS["grid"],
                     float(np.linalg.norm(hi[1][c]))))
    return rows


def check_adjoint(oracle, s, key, mode, label):
    """The host build's adjoint with the seeds of `mode`, flag on, under the bound; the signal is real."""
    y = yard(oracle, s, key)
    dx, dv, dcirc = seeds_of(s, mode, y["compared"])
    seeded = mode == "all"
    r = host_back(s, y["k"], dx if seeded else None, dv if seeded else None, dcirc, corrected_h=True)
    rows = adjoint_rows(oracle, s, key, mode, r["dpos"], r["dvel"], r["grad"], r["grad_vfield"])
    bad = IF.report(f"{label} seeds={mode}", rows)
    assert rows[0][4] > 1e-3 and all(row[4] > 0.1 for row in rows[1:]), rows
    assert bad == []
    return r


def gpu_forward(T, s, dev):
    from adjointnonlinearraytracing_amd import drrt
    xt, vt, circ, steps = T.trace_vector(_t(s["rif"], dev), _t(s["vfield"], dev), s["res"], _t(s["pos"], dev),
                                         _t(s["vel"], dev), s["h"], s["ds"])
    return xt, vt, circ, steps, drrt.read_stats(), drrt.keep_order(drrt.last_order)


def gpu_back(T, s, dev, fw, order=None, dx="dx", dv="dv", dcirc="dcirc", **kw):
    from adjointnonlinearraytracing_amd import drrt
    xt, vt, _, steps = fw[:4]
    seed = lambda k: None if k is None else _t(s[k], dev)      # noqa: E731
    out = T.backtrace_vector(_t(s["rif"], dev), _t(s["vfield"], dev), s["res"], _t(s["pos"], dev), _t(s["vel"], dev), xt, vt,
                             steps, seed(dx), seed(dv), seed(dcirc), s["h"], s["ds"], order=order, **kw)
    return out, drrt.read_stats()


def grids_close(grad, gvf, r, tol=ATOMIC_TOL):
    """dL/drif and each plane of dL/du within `tol` rel-L2 of the host build's."""
    errs = [cases.rel_l2(grad.cpu().numpy(), r["grad"])]
    errs += [cases.rel_l2(a, b) for a, b in zip(gvf.cpu().numpy().reshape(3, -1), r["grad_vfield"].reshape(3, -1))]
    return max(errs) <= tol


def ad_grads(s, dev, seeds, rif_grad=True, vfield_grad=True, x_grad=True, v_grad=True, dtype=torch.float32, vfield=None,
             shaped=False):
    """VectorIntegralTracerC.apply -> L = <dx, xt> + <dv, vt> + <dcirc, circ> -> backward
    -> (rif.grad, vfield.grad, x.grad, v.grad, outputs).  `shaped`: the grids go in with the shape of the resolution
    (W, H, D), which the class takes from rif.shape (a non-cubic configuration); the flat order is the library's either way."""
    from adjointnonlinearraytracing_amd import tracer
    rif, vf = _t(s["rif"], dev), _t(s["vfield"] if vfield is None else vfield, dev)
    if shaped:
        rif, vf = rif.reshape(*s["res"]), vf.reshape(3, *s["res"])
    rif, vf = rif.requires_grad_(rif_grad), vf.requires_grad_(vfield_grad)
    x = _t(s["pos"], dev).to(dtype).requires_grad_(x_grad)
    v = _t(s["vel"], dev).requires_grad_(v_grad)
    out = tracer.VectorIntegralTracerC.apply(rif, vf, x, v, s["h"], s["ds"])
    loss = sum((o * _t(np.asarray(w, np.float32), dev)).sum() for o, w in zip(out, seeds) if w is not None)
    if loss.requires_grad:
        loss.backward()
    torch.cuda.synchronize()
    return rif.grad, vf.grad, x.grad, v.grad, [o.detach() for o in out]
