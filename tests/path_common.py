"""What test_path.py and test_path_fuzz.py share: the sample counts, the host build's calls, the referee of trace_path
(float64 autograd, float32 as the yardstick) and the GPU calls.  A plain module: no fixtures, no tests."""
import numpy as np
import torch

import cases
import integral_ad
import integral_host as OH
from integral_common import _same
from integral_fuzz_common import CAPS, FLOOR, bound
from raygrad_common import _t, max_steps_fwd, rel_err

MODES = ("all", "noray", "prefix", "inbox", "padded")
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


def fwd(s, stride, M):
    return OH.trace_path(s["rif"], s["res"], s["pos"], s["vel"], s["h"], s["ds"], stride, M)


def back(s, k, dx, dv, dpath, stride, M, sel=slice(None), **kw):
    cut = lambda a: None if a is None else a[sel]      # noqa: E731
    return OH.backtrace_path(s["rif"], s["res"], s["pos"][sel], s["vel"][sel], k["xt"][sel], k["vt"][sel], k["steps"][sel],
                             cut(dx), cut(dv), None if dpath is None else dpath[:, sel], s["h"], s["ds"], stride, M, **kw)


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


def referee(c, compared, stride, M, tag, modes=MODES):
    """The host build against float64 autograd under the bound float32 autograd sets, on the configuration `c`, for every
    mode -> (largest e_prod / max(e_ref, FLOOR) over the gradients, the rows that miss their bound, {mode: |seeds|_1}).
    One forward per dtype; the host forward's count and steps must be the float64 run's on the compared rays."""
    k = fwd(c, stride, M)
    ms = max_steps_fwd(c["res"], c["h"], c["ds"])
    idx = np.nonzero(compared)[0]
    n = len(c["pos"])
    base = dpath_of((M, n, 3), stride * 1000 + M)
    pre, box, pad = classes(k, back(c, k, None, None, None, stride, M), stride, M)
    keep = {"all": np.ones((M, n), bool), "noray": np.ones((M, n), bool), "prefix": pre, "inbox": box, "padded": pad}
    edge = max((r - 1) * c["h"] for r in c["res"])
    runs = {}
    for dt in (torch.float64, torch.float32):
        T = lambda a: torch.tensor(np.asarray(a), dtype=dt)      # noqa: E731
        leaves = [T(c["rif"]).requires_grad_(True), T(c["pos"][idx]).requires_grad_(True), T(c["vel"][idx]).requires_grad_(True)]
        runs[dt] = (leaves, integral_ad.trace_path(*leaves, c["h"], c["ds"], stride, M), T)
    hi, lo = runs[torch.float64][1], runs[torch.float32][1]
    assert np.array_equal(hi[4].numpy(), k["steps"][idx].astype(np.int64)) and np.array_equal(lo[4].numpy(), hi[4].numpy())
    assert np.array_equal(hi[3].numpy(), k["count"][idx]) and np.array_equal(k["count"], count_of(k["steps"], stride, M))
    p64 = hi[2].detach().numpy()
    e_path = float(np.abs(k["path"][:, idx].astype(np.float64) - p64).max() / edge)
    e_path_ref = float(np.abs(lo[2].detach().numpy().astype(np.float64) - p64).max() / edge)
    print(f"{tag} path: e_prod {e_path:.3e} e_ref {e_path_ref:.3e} ratio {e_path / max(e_path_ref, FLOOR):.2f} cap {CAPS['out']:.1e}")
    bad = [] if e_path <= CAPS["out"] else [("path", e_path, e_path_ref, CAPS["out"])]
    worst, weight = 0.0, {}
    for mode in modes:
        z = compared[:, None] if mode == "all" else np.zeros((n, 1), bool)
        dx, dv = (c["dx"] * z).astype(np.float32), (c["dv"] * z).astype(np.float32)
        dpath = (base * (keep[mode] & compared[None, :])[:, :, None]).astype(np.float32)
        weight[mode] = float(np.abs(dpath).sum())
        r = back(c, k, dx if mode == "all" else None, dv if mode == "all" else None, dpath, stride, M, corrected_h=True)
        g = {}
        for dt, (leaves, out, T) in runs.items():
            L = (out[0] * T(dx[idx])).sum() + (out[1] * T(dv[idx])).sum() + (out[2] * T(dpath[:, idx])).sum()
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
            worst = max(worst, ratio)
            print(f"{tag} seeds={mode} {name}: e_prod {e_prod:.3e} e_ref {e_ref:.3e} ratio {ratio:.2f} bound {b:.3e}")
            if not e_prod <= b:
                bad.append((mode, name, e_prod, e_ref, b))
        assert r["n_failed"] == int((k["steps"] >= ms).sum()) == k["n_failed"]
    print(f"{tag}: largest ratio to the yardstick {worst:.2f}")
    return worst, bad, weight


def _gpu_forward(T, s, dev, stride, M):
    from adjointnonlinearraytracing_amd import drrt
    out = T.trace_path(_t(s["rif"], dev), s["res"], _t(s["pos"], dev), _t(s["vel"], dev), s["h"], s["ds"], stride, M)
    return out, drrt.read_stats(), drrt.keep_order(drrt.last_order)


def _gpu_back(T, s, dev, out, stride, dpath, order=None, dx="dx", dv="dv", **kw):
    from adjointnonlinearraytracing_amd import drrt
    xt, vt, _, _, steps = out
    seed = lambda k: None if k is None else _t(s[k], dev)      # noqa: E731
    res = T.backtrace_path(_t(s["rif"], dev), s["res"], _t(s["pos"], dev), _t(s["vel"], dev), xt, vt, steps, seed(dx), seed(dv),
                           None if dpath is None else _t(dpath, dev), s["h"], s["ds"], stride, order=order, **kw)
    return res, drrt.read_stats()


def _forward_matches(out, st, k):
    xt, vt, path, count, steps = out
    assert _same(xt, k["xt"]) and _same(vt, k["vt"]) and _same(path, k["path"])
    assert count.dtype == torch.int32 and np.array_equal(count.cpu().numpy(), k["count"])
    assert np.array_equal(steps.cpu().numpy().astype(np.int64), k["steps"].astype(np.int64))
    assert st["n_failed"] == k["n_failed"] and st["ray_steps"] == int(k["steps"].astype(np.int64).sum())
