"""What test_phase_path.py and test_phase_path_fuzz.py share: the host build's calls, the referee of trace_phase (float64
autograd, float32 as the yardstick) and the GPU calls.  The sample counts, strides and seed classes are path_common's.  A
plain module: no fixtures, no tests."""
import numpy as np
import torch

import cases
from integral_common import _same
from integral_fuzz_common import CAPS, FLOOR, bound
from path_common import classes, count_of, dpath_of
import phase_path_ad
import phase_path_host as PH
from raygrad_common import _t, max_steps_fwd, rel_err

# mode -> (ray seeds, which entries of dpath, which entries of dvpath): None = no seed of that kind
MODES = {"all": (True, "every", "every"), "noray": (False, "every", "every"), "vprefix": (False, None, "prefix"),
         "vinbox": (False, None, "inbox"), "vpadded": (False, None, "padded"), "inbox": (False, "inbox", "inbox")}


def fwd(s, stride, M):
    return PH.trace_phase(s["rif"], s["res"], s["pos"], s["vel"], s["h"], s["ds"], stride, M)


def back(s, k, dx, dv, dpath, dvpath, stride, M, **kw):
    return PH.backtrace_phase(s["rif"], s["res"], s["pos"], s["vel"], k["xt"], k["vt"], k["steps"], dx, dv, dpath, dvpath,
                              s["h"], s["ds"], stride, M, **kw)


def dvpath_of(shape, seed):
    return np.random.default_rng(seed + 9100).normal(size=shape).astype(np.float32)


def referee(c, compared, stride, M, tag, modes=tuple(MODES)):
    """The host build against float64 autograd of L = <dx, xt> + <dv, vt> + <dpath, path> + <dvpath, vpath> under the bound
    float32 autograd sets, on the configuration `c`, for every mode -> ({quantity: largest e_prod / max(e_ref, FLOOR)}, the
    rows that miss their bound, {mode: |series seeds|_1}).  One forward per dtype; the host forward's count and steps must be
    the float64 run's on the compared rays.  A sample's error is the largest absolute difference over the compared rays and
    j < M, over the box's longest edge for path and over the largest |v| of the float64 run for vpath."""
    k = fwd(c, stride, M)
    ms = max_steps_fwd(c["res"], c["h"], c["ds"])
    idx = np.nonzero(compared)[0]
    n = len(c["pos"])
    base, vbase = dpath_of((M, n, 3), stride * 1000 + M), dvpath_of((M, n, 3), stride * 1000 + M)
    pre, box, pad = classes(k, back(c, k, None, None, None, None, stride, M), stride, M)
    keep = {"every": np.ones((M, n), bool), "prefix": pre, "inbox": box, "padded": pad}
    edge = max((r - 1) * c["h"] for r in c["res"])
    runs = {}
    for dt in (torch.float64, torch.float32):
        T = lambda a, dt=dt: torch.tensor(np.asarray(a), dtype=dt)      # noqa: E731
        leaves = [T(c["rif"]).requires_grad_(True), T(c["pos"][idx]).requires_grad_(True), T(c["vel"][idx]).requires_grad_(True)]
        runs[dt] = (leaves, phase_path_ad.trace_phase(*leaves, c["h"], c["ds"], stride, M), T)
    hi, lo = runs[torch.float64][1], runs[torch.float32][1]
    assert np.array_equal(hi[5].numpy(), k["steps"][idx].astype(np.int64)) and np.array_equal(lo[5].numpy(), hi[5].numpy())
    assert np.array_equal(hi[4].numpy(), k["count"][idx]) and np.array_equal(k["count"], count_of(k["steps"], stride, M))
    worst, bad = {}, []
    vmax = float(np.linalg.norm(hi[3].detach().numpy(), axis=2).max())
    for name, col, scale in (("path", 2, edge), ("vpath", 3, vmax)):
        x64 = hi[col].detach().numpy()
        e_prod = float(np.abs(k[name][:, idx].astype(np.float64) - x64).max() / scale)
        e_ref = float(np.abs(lo[col].detach().numpy().astype(np.float64) - x64).max() / scale)
        worst[name] = e_prod / max(e_ref, FLOOR)
        print(f"{tag} {name}: e_prod {e_prod:.3e} e_ref {e_ref:.3e} ratio {worst[name]:.2f} cap {CAPS['out']:.1e}")
        if not e_prod <= CAPS["out"]:
            bad.append((name, e_prod, e_ref, CAPS["out"]))
    weight = {}
    for mode in modes:
        rays, which, vwhich = MODES[mode]
        z = compared[:, None] if rays else np.zeros((n, 1), bool)
        dx, dv = (c["dx"] * z).astype(np.float32), (c["dv"] * z).astype(np.float32)
        cut = lambda b, w: (b * ((keep[w] if w else np.zeros((M, n), bool)) & compared[None, :])[:, :, None]).astype(np.float32)   # noqa: E731
        dpath, dvpath = cut(base, which), cut(vbase, vwhich)
        weight[mode] = float(np.abs(dpath).sum() + np.abs(dvpath).sum())
        r = back(c, k, dx if rays else None, dv if rays else None, dpath if which else None, dvpath, stride, M,
                 corrected_h=True)
        g = {}
        for dt, (leaves, out, T) in runs.items():
            L = (out[0] * T(dx[idx])).sum() + (out[1] * T(dv[idx])).sum() + (out[2] * T(dpath[:, idx])).sum() + \
                (out[3] * T(dvpath[:, idx])).sum()
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
    print(f"{tag}: largest ratios to the yardstick " + ", ".join(f"{q} {v:.2f}" for q, v in worst.items()))
    return worst, bad, weight


def _gpu_forward(T, s, dev, stride, M):
    from adjointnonlinearraytracing_amd import drrt
    out = T.trace_phase(_t(s["rif"], dev), s["res"], _t(s["pos"], dev), _t(s["vel"], dev), s["h"], s["ds"], stride, M)
    return out, drrt.read_stats(), drrt.keep_order(drrt.last_order)


def _gpu_back(T, s, dev, out, stride, dpath, dvpath, order=None, dx="dx", dv="dv", **kw):
    from adjointnonlinearraytracing_amd import drrt
    xt, vt, _, _, _, steps = out
    seed = lambda k: None if k is None else _t(s[k], dev)      # noqa: E731
    series = lambda a: None if a is None else _t(a, dev)      # noqa: E731
    res = T.backtrace_phase(_t(s["rif"], dev), s["res"], _t(s["pos"], dev), _t(s["vel"], dev), xt, vt, steps, seed(dx), seed(dv),
                            series(dpath), series(dvpath), s["h"], s["ds"], stride, order=order, **kw)
    return res, drrt.read_stats()


def _forward_matches(out, st, k):
    xt, vt, path, vpath, count, steps = out
    assert _same(xt, k["xt"]) and _same(vt, k["vt"]) and _same(path, k["path"]) and _same(vpath, k["vpath"])
    assert count.dtype == torch.int32 and np.array_equal(count.cpu().numpy(), k["count"])
    assert np.array_equal(steps.cpu().numpy().astype(np.int64), k["steps"].astype(np.int64))
    assert st["n_failed"] == k["n_failed"] and st["ray_steps"] == int(k["steps"].astype(np.int64).sum())
