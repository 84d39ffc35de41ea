"""What test_path.py, test_path_fuzz.py, test_phase_path.py and test_phase_path_fuzz.py share: the sample counts, the host
build's calls, the referee of trace_path and trace_phase (float64 autograd, float32 as the yardstick) and the GPU calls.
Every helper serves both: path is phase without the velocity series (`velocities=False`, one series where phase hands two);
the *_phase names fix `velocities=True`.  A plain module: no fixtures, no tests."""
import functools

import numpy as np
import torch

import cases
import integral_ad
import integral_host as OH
from integral_common import _same
from integral_fuzz_common import CAPS, FLOOR, bound
from raygrad_common import _t, max_steps_fwd, rel_err

# mode -> (ray seeds, which entries of dpath, which entries of dvpath): None = no seed of that kind.  The path modes are the
# modes with no velocity seed.
PATH_MODES = {"all": (True, "every", None), "noray": (False, "every", None), "prefix": (False, "prefix", None),
              "inbox": (False, "inbox", None), "padded": (False, "padded", None)}
PHASE_MODES = {"all": (True, "every", "every"), "noray": (False, "every", "every"), "vprefix": (False, None, "prefix"),
               "vinbox": (False, None, "inbox"), "vpadded": (False, None, "padded"), "inbox": (False, "inbox", "inbox")}
STRIDES = (1, 5)
_bits = lambda a: np.ascontiguousarray(a).view(np.uint32)      # noqa: E731


def pad_m(ms, stride):
    """The smallest M that always ends on xt (the Python surface's default)."""
    return -(-ms // stride) + 1


def trunc_m(ms, stride):
    """An M that cuts every ray that crosses the box: a crossing takes about max_steps / 4 iterations."""
    return ms // (8 * stride) + 2


def count_of(steps, stride, M):
    return np.minimum(M, -(-steps.astype(np.int64) // stride)).astype(np.int64)


def dpath_of(shape, seed):
    return np.random.default_rng(seed + 4200).normal(size=shape).astype(np.float32)


def classes(k, r, stride, M):
    """(prefix, inbox, padded) masks of shape (M, n) from the host forward `k` and a host adjoint `r` of it (whose reverse
    iteration counts give the free-flight prefix e = K - steps of every ray that did not fail)."""
    K = k["steps"].astype(np.int64)
    e = K - r["steps"].astype(np.int64)
    idx = (np.arange(M, dtype=np.int64) * stride)[:, None]
    sample = np.arange(M)[:, None] < k["count"][None, :]
    return sample & (idx <= e[None, :]), sample & (idx > e[None, :]), ~sample


def dvpath_of(shape, seed):
    return np.random.default_rng(seed + 9100).normal(size=shape).astype(np.float32)


def fwd(s, stride, M, velocities=False):
    entry = OH.trace_phase if velocities else OH.trace_path
    return entry(s["rif"], s["res"], s["pos"], s["vel"], s["h"], s["ds"], stride, M)


def _back(entry, s, k, dx, dv, series, stride, M, sel=slice(None), **kw):
    cut = lambda a: None if a is None else a[sel]      # noqa: E731
    return entry(s["rif"], s["res"], s["pos"][sel], s["vel"][sel], k["xt"][sel], k["vt"][sel], k["steps"][sel], cut(dx), cut(dv),
                 *(None if a is None else a[:, sel] for a in series), s["h"], s["ds"], stride, M, **kw)


def back(s, k, dx, dv, dpath, stride, M, **kw):
    return _back(OH.backtrace_path, s, k, dx, dv, (dpath,), stride, M, **kw)


def back_phase(s, k, dx, dv, dpath, dvpath, stride, M, **kw):
    return _back(OH.backtrace_phase, s, k, dx, dv, (dpath, dvpath), stride, M, **kw)


def referee(c, compared, stride, M, tag, modes=None, velocities=False):
    """The host build against float64 autograd of L = <dx, xt> + <dv, vt> + <dpath, path> (+ <dvpath, vpath> with
    `velocities`) under the bound float32 autograd sets, on the configuration `c`, for every mode (PHASE_MODES with
    `velocities`, else PATH_MODES) -> (the largest e_prod / max(e_ref, FLOOR): per quantity with `velocities`, else the one
    figure over the gradients, the rows that miss their bound, {mode: |series seeds|_1}).  One forward per dtype; the host forward's count and steps must be the float64 run's on the
    compared rays.  A sample's error is the largest absolute difference over the compared rays and j < M, over the box's
    longest edge for path and over the largest |v| of the float64 run for vpath."""
    table = PHASE_MODES if velocities else PATH_MODES
    names = ("path", "vpath") if velocities else ("path",)
    k = fwd(c, stride, M, velocities)
    ms = max_steps_fwd(c["res"], c["h"], c["ds"])
    idx = np.nonzero(compared)[0]
    n = len(c["pos"])
    bases = (dpath_of((M, n, 3), stride * 1000 + M), dvpath_of((M, n, 3), stride * 1000 + M))[:len(names)]
    host_back = (lambda *a, **kw: back_phase(c, k, *a, stride, M, **kw)) if velocities else \
        (lambda *a, **kw: back(c, k, *a, stride, M, **kw))
    pre, box, pad = classes(k, host_back(None, None, *(None,) * len(names)), stride, M)
    keep = {"every": np.ones((M, n), bool), "prefix": pre, "inbox": box, "padded": pad}
    edge = max((r - 1) * c["h"] for r in c["res"])
    runs = {}
    for dt in (torch.float64, torch.float32):
        T = lambda a, dt=dt: torch.tensor(np.asarray(a), dtype=dt)      # noqa: E731
        leaves = [T(c["rif"]).requires_grad_(True), T(c["pos"][idx]).requires_grad_(True), T(c["vel"][idx]).requires_grad_(True)]
        runs[dt] = (leaves, integral_ad.trace_path(*leaves, c["h"], c["ds"], stride, M, velocities), T)
    hi, lo = runs[torch.float64][1], runs[torch.float32][1]
    assert np.array_equal(hi[-1].numpy(), k["steps"][idx].astype(np.int64)) and np.array_equal(lo[-1].numpy(), hi[-1].numpy())
    assert np.array_equal(hi[-2].numpy(), k["count"][idx]) and np.array_equal(k["count"], count_of(k["steps"], stride, M))
    worst, bad = {}, []
    scales = (edge, float(np.linalg.norm(hi[3].detach().numpy(), axis=2).max()) if velocities else None)
    for col, (name, scale) in enumerate(zip(names, scales), 2):
        x64 = hi[col].detach().numpy()
        e_prod = float(np.abs(k[name][:, idx].astype(np.float64) - x64).max() / scale)
        e_ref = float(np.abs(lo[col].detach().numpy().astype(np.float64) - x64).max() / scale)
        worst[name] = e_prod / max(e_ref, FLOOR)
        print(f"{tag} {name}: e_prod {e_prod:.3e} e_ref {e_ref:.3e} ratio {worst[name]:.2f} cap {CAPS['out']:.1e}")
        if not e_prod <= CAPS["out"]:
            bad.append((name, e_prod, e_ref, CAPS["out"]))
    weight = {}
    for mode in modes or tuple(table):
        rays, *which = table[mode]
        z = compared[:, None] if rays else np.zeros((n, 1), bool)
        dx, dv = (c["dx"] * z).astype(np.float32), (c["dv"] * z).astype(np.float32)
        cut = lambda b, w: (b * ((keep[w] if w else np.zeros((M, n), bool)) & compared[None, :])[:, :, None]).astype(np.float32)   # noqa: E731
        series = [cut(b, w) for b, w in zip(bases, which)]
        weight[mode] = float(np.sum([np.abs(a).sum() for a in series], dtype=np.float32))
        # a path seed of no entries is no seed at all; the velocity seed is always handed over
        r = host_back(dx if rays else None, dv if rays else None, series[0] if which[0] else None, *series[1:],
                      corrected_h=True)
        g = {}
        for dt, (leaves, out, T) in runs.items():
            L = (out[0] * T(dx[idx])).sum() + (out[1] * T(dv[idx])).sum()
            for o, a in zip(out[2:], series):
                L = L + (o * T(a[:, idx])).sum()
            gr, gp, gv = torch.autograd.grad(L, leaves, retain_graph=True, allow_unused=True)
            rows_ = []
            for a in (gp, gv):                                             # only the compared rays are marched
                rows_.append(np.zeros((n, 3)))
                if a is not None:
                    rows_[-1][idx] = a.numpy()
            g[dt] = (np.zeros(c["rif"].size) if gr is None else gr.numpy().reshape(-1), *rows_)
        (gr64, gp64, gv64), (gr32, gp32, gv32) = g[torch.float64], g[torch.float32]
        rows = [("rays", float(rel_err(r["dpos"], r["dvel"], gp64, gv64)[compared].max()),
                 float(rel_err(gp32, gv32, gp64, gv64)[compared].max()), CAPS["rays"])]
        if np.linalg.norm(gr64) > 0:
            rows.append(("dL/drif", cases.rel_l2(r["grad"], gr64), cases.rel_l2(gr32, gr64), CAPS["grid"]))
        else:
            assert not r["grad"].any()
        for name, e_prod, e_ref, cap in rows:
            b = bound(e_ref, cap)
            ratio = e_prod / max(e_ref, FLOOR)
            worst[name] = max(worst.get(name, 0.0), ratio)
            print(f"{tag} seeds={mode} {name}: e_prod {e_prod:.3e} e_ref {e_ref:.3e} ratio {ratio:.2f} bound {b:.3e}")
            if not e_prod <= b:
                bad.append((mode, name, e_prod, e_ref, b))
        assert r["n_failed"] == int((k["steps"] >= ms).sum()) == k["n_failed"]
    if velocities:
        print(f"{tag}: largest ratios to the yardstick " + ", ".join(f"{q} {v:.2f}" for q, v in worst.items()))
        return worst, bad, weight
    worst = max((v for q, v in worst.items() if q not in names), default=0.0)
    print(f"{tag}: largest ratio to the yardstick {worst:.2f}")
    return worst, bad, weight


def _gpu_forward(T, s, dev, stride, M, velocities=False):
    from adjointnonlinearraytracing_amd import drrt
    march = T.trace_phase if velocities else T.trace_path
    out = march(_t(s["rif"], dev), s["res"], _t(s["pos"], dev), _t(s["vel"], dev), s["h"], s["ds"], stride, M)
    return out, drrt.read_stats(), drrt.keep_order(drrt.last_order)


def _back_gpu(march, s, dev, out, stride, series, order=None, dx="dx", dv="dv", **kw):
    from adjointnonlinearraytracing_amd import drrt
    xt, vt, *_, steps = out
    seed = lambda k: None if k is None else _t(s[k], dev)      # noqa: E731
    res = march(_t(s["rif"], dev), s["res"], _t(s["pos"], dev), _t(s["vel"], dev), xt, vt, steps, seed(dx), seed(dv),
                *(None if a is None else _t(a, dev) for a in series), s["h"], s["ds"], stride, order=order, **kw)
    return res, drrt.read_stats()


def _gpu_back(T, s, dev, out, stride, dpath, **kw):
    return _back_gpu(T.backtrace_path, s, dev, out, stride, (dpath,), **kw)


def _gpu_back_phase(T, s, dev, out, stride, dpath, dvpath, **kw):
    return _back_gpu(T.backtrace_phase, s, dev, out, stride, (dpath, dvpath), **kw)


def _forward_matches(out, st, k):
    xt, vt, *series, count, steps = out
    assert _same(xt, k["xt"]) and _same(vt, k["vt"])
    assert len(series) == (2 if "vpath" in k else 1) and all(_same(a, k[name]) for a, name in zip(series, ("path", "vpath")))
    assert count.dtype == torch.int32 and np.array_equal(count.cpu().numpy(), k["count"])
    assert np.array_equal(steps.cpu().numpy().astype(np.int64), k["steps"].astype(np.int64))
    assert st["n_failed"] == k["n_failed"] and st["ray_steps"] == int(k["steps"].astype(np.int64).sum())


fwd_phase = functools.partial(fwd, velocities=True)
referee_phase = functools.partial(referee, velocities=True)
_gpu_forward_phase = functools.partial(_gpu_forward, velocities=True)
