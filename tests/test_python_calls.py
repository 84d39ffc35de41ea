"""Call transcript of the Python tracer layer (drrt.TracerC / TracerS, the tracer.* autograd classes, dist.ShardedBackTracerC).

The layer marshals arguments for the C ABI; what it computes is the kernels' business and is tested elsewhere.  What is
pinned here is what the layer ASKS of the library: for every case a recorder stands in for ``_lib.load()`` and writes down
every ``drrt_*`` call -- entry name, integers and floats, the flags word, and for every pointer what it addresses (a named
input of the Python call, output k of it, the stats block, the workspace and the offset into it, null) --, the order / step
hints in sequence, and after every Python call which of ``last_order`` / ``last_steps`` / ``last_bundle_counters`` are set,
whether ``keep_order`` accepts the order, and the kernels launched (``drrt_profile_begin`` / ``_lib.profile_collect``).
The expected transcript is ``tests/golden/python_calls.json``, recorded with this very file (``DRRT_RECORD_CALLS=<path>``
writes one instead of comparing) from the commit BEFORE the layer was folded onto one grid-call path and one autograd
skeleton, so the table is that commit's, not this one's.  The file uses the public surface and the ``_lib.load`` hook only.

What makes a transcript independent of what ran before it: every case starts with one unrecorded ``backtrace`` and one
unrecorded ``trace`` (the module's ``last_*`` attributes, the library's per-thread last order / steps and this stream's
workspace are then those calls'); the workspace is written down as "ws" with its size compared with what
``drrt_workspace_bytes_grid`` just answered, not as a number of bytes (it only ever grows).

Shapes: a 9 x 10 x 11 grid (so a transposed ``res`` shows), h = 1/8, ds = h/2; 65 rays = one full wave plus one lane,
so two adjoint blocks, six of them never entering the box; 1 ray; 0 rays; an 8-sample fibre profile.  Where gradients are
compared bit for bit (the autograd classes against the direct calls) the seeds of the one ray that sits alone in the
second block -- the last of the forward's visit order, and the last of the caller's order for the unsorted fibre march
-- are zero: it then adds zeros, and the sum over the first block's rays does not depend on when it does."""
import json
import os

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "python_calls.json")
RECORD = os.environ.get("DRRT_RECORD_CALLS")
W, H, D = 9, 10, 11
HH, DS = 0.125, 0.0625
RADIUS, LENGTH, CDS = 0.5, 2.0, 0.03125
NS = (65, 1, 0)

# the march entries: (name suffix, where their tail (stats, workspace, workspace_bytes, flags, stream) starts)
_TAIL_AT = {"drrt_backtrace_chunk_f32": -10}
_PTR_RETURNS = ("drrt_last_order", "drrt_last_steps", "drrt_last_bundle_counters")
_recorded = {}


def _is_march(name):
    return name.endswith(("_f32", "_f16io", "_q16io")) and name.startswith(("drrt_trace", "drrt_backtrace"))


class Recorder:
    """Stands in for the ctypes library: forwards every call, writes the ``drrt_*`` ones down."""

    def __init__(self, lib, drrt):
        self._lib, self._drrt = lib, drrt
        self.lines, self.named, self.ws, self.need, self.pending, self.quiet = [], {}, None, 0, [], False

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("drrt_") or name.startswith("drrt_profile") or name in ("drrt_last_error", "drrt_version"):
            return fn

        def call(*args):
            rc = fn(*args)
            if not self.quiet:
                self._note(name, args, rc)
            elif _is_march(name):
                self._tail(name, args)
            return rc
        return call

    def name(self, **tensors):
        for k, t in tensors.items():
            if t is not None:
                self.named[k] = (t.data_ptr(), t.numel() * t.element_size(), t)      # holding t keeps the address its own

    def _where(self, addr):
        if not addr:
            return "null"
        for k, (ptr, nbytes, _) in self.named.items():
            if ptr and ptr <= addr < ptr + max(nbytes, 1):
                return k if addr == ptr else f"{k}+{addr - ptr}"
        if self.ws and self.ws[0] <= addr < self.ws[0] + self.ws[1]:
            return f"ws+{addr - self.ws[0]}"
        return None

    def _tail(self, name, args):
        t = _TAIL_AT.get(name, -5)
        self.ws = (args[t + 1].value or 0, int(args[t + 2]))
        return t % len(args)

    def _note(self, name, args, rc):
        import ctypes as C
        t = self._tail(name, args) if _is_march(name) else None
        out = []
        for i, a in enumerate(args):
            if t is not None and i == t:
                st = self._drrt.last_stats
                out.append("stats" if st is not None and a.value == st.data_ptr() else "NOT-last_stats")
            elif t is not None and i == t + 1:
                out.append("ws")
            elif t is not None and i == t + 2:
                out.append("ws_bytes>=need" if int(a) >= self.need else f"ws_bytes={int(a)}<need={self.need}")
            elif t is not None and i == t + 3:
                out.append(hex(int(a)))
            elif t is not None and i == t + 4:
                out.append("stream" if (a.value or 0) == torch.cuda.current_stream().cuda_stream else "NOT-current-stream")
            elif a is None:
                out.append("null")
            elif isinstance(a, C.c_void_p):
                w = self._where(a.value)
                if w is None:                        # an output, or a temporary: known when the Python call has returned
                    self.pending.append((len(self.lines), len(out), a.value))
                    w = "?"
                out.append(w)
            elif isinstance(a, C.Array):
                out.append(str(list(a)))
            elif i == 0 and name in ("drrt_set_order_hint", "drrt_set_step_hint"):
                out.append(self._where(a) or "other")          # an address as an integer: what drrt_last_order() returned
            elif isinstance(a, (int, float)):
                out.append(repr(a))
            else:
                out.append("&count")                 # C.byref(count)
        if name in _PTR_RETURNS:
            ret = self._where(rc) or "other"
            if args and hasattr(args[0], "_obj"):
                ret += f" count={args[0]._obj.value}"
        else:
            ret = repr(rc)
            if name == "drrt_workspace_bytes_grid":
                self.need = int(rc)
        self.lines.append([name] + out + ["-> " + ret])

    def resolve(self, outputs):
        """After a Python call: the pointers not placed yet are its outputs, or tensors nobody outside the call saw."""
        self.name(**{f"out{k}": t for k, t in enumerate(outputs) if isinstance(t, torch.Tensor)})
        for line, col, addr in self.pending:
            self.lines[line][1 + col] = self._where(addr) or "other"
        self.pending = []
        for k in [k for k in self.named if k.startswith("out")]:
            del self.named[k]
        self.lines = [ln if isinstance(ln, str) else f"{ln[0]}({', '.join(ln[1:-1])}) {ln[-1]}" for ln in self.lines]


class Case:
    """One transcript: ``do(label, fn, *args)`` makes a Python call under the recorder and returns what it returned."""

    def __init__(self, monkeypatch, scene):
        from adjointnonlinearraytracing_amd import _lib, drrt
        self.drrt, self._lib, self.s = drrt, _lib, scene
        self.T = drrt.TracerC()
        self.rec = Recorder(_lib.load(), drrt)
        monkeypatch.setattr(_lib, "load", lambda: self.rec)
        self.rec.quiet = True
        s = scene[65]
        # the fixed starting state (module docstring): an adjoint, then a forward
        self.T.backtrace(s["rif"], (W, H, D), s["pos"], s["vel"], s["dx"], s["dv"], HH, DS)
        self.T.trace(s["rif"], (W, H, D), s["pos"], s["vel"], HH, DS)
        torch.cuda.synchronize()
        self.rec.quiet = False
        self.rec._lib.drrt_profile_begin(256)

    def close(self):
        self.rec._lib.drrt_profile_end()

    def do(self, label, fn, *args, **kw):
        rec, drrt = self.rec, self.drrt
        rec.lines.append(f"== {label}")
        err = None
        try:
            out = fn(*args, **kw)
        except RuntimeError as e:
            out, err = None, str(e)
        rec.resolve(out if isinstance(out, (tuple, list)) else (out,))
        if err is not None:
            rec.lines.append("raised: " + err)
        order = drrt.last_order
        rec.quiet = True
        kept = drrt.keep_order(order)
        names = [n for n, _ in self._lib.profile_collect()]
        rec.quiet = False
        rec.lines.append(f"last_order={order is not None} keep_order={kept is not None} steps_on_order="
                         f"{getattr(order, 'drrt_steps', None) is not None} last_steps={drrt.last_steps is not None} "
                         f"last_bundle_counters={drrt.last_bundle_counters is not None} launches={','.join(names)}")
        return out

    def quietly(self, fn, *args, **kw):
        self.rec.quiet = True
        try:
            return fn(*args, **kw)
        finally:
            self.rec.quiet = False


def _check(case_id, case):
    case.close()
    lines = case.rec.lines
    assert not [ln for ln in lines if "NOT-" in ln or "<need" in ln], lines
    if RECORD:
        _recorded[case_id] = lines
        return
    with open(GOLDEN) as f:
        table = json.load(f)                     # {"lines": the distinct lines, "cases": {case: indices into them}}
    want = [table["lines"][k] for k in table["cases"][case_id]]
    assert lines == want, "\n".join(f"{'  ' if a == b else '!!'} {a}\n{'  ' if a == b else '!!'} {b}" for a, b in
                                    zip(lines + [""] * len(want), want + [""] * len(lines)) if a != b or not a)


@pytest.fixture(scope="module", autouse=True)
def _write_recording():
    yield
    if RECORD and _recorded:
        lines = sorted({ln for case in _recorded.values() for ln in case})
        at = {ln: k for k, ln in enumerate(lines)}
        with open(RECORD, "w") as f:
            json.dump(dict(lines=lines, cases={k: [at[ln] for ln in v] for k, v in sorted(_recorded.items())}), f, indent=0)


# ---- the scene ------------------------------------------------------------------------------------------------------
def _field(seed=3, amp=0.2):
    """cases.smooth_field on the 9 x 10 x 11 grid: band-limited, asymmetric in x, y, z."""
    rng = np.random.default_rng(seed)
    Z, Y, X = np.meshgrid(np.linspace(0, 1, D), np.linspace(0, 1, H), np.linspace(0, 1, W), indexing="ij")
    f = np.zeros((D, H, W))
    for _ in range(6):
        k = rng.uniform(0.5, 3.0, 3) * np.pi
        ph = rng.uniform(0, 2 * np.pi, 3)
        f += rng.uniform(0.3, 1.0) * np.sin(k[0] * X + ph[0]) * np.sin(k[1] * Y + ph[1]) * np.sin(k[2] * Z + ph[2])
    f = (f - f.min()) / (f.max() - f.min())
    sdf = np.sqrt((X - 0.5) ** 2 + (Y - 0.5) ** 2 + (Z - 0.5) ** 2) - 0.3
    return (1.0 + amp * f).astype(np.float32), sdf.astype(np.float32)


def _rays(n_all=65, seed=11):
    rng = np.random.default_rng(seed)
    ext = np.array([(W - 1) * HH, (H - 1) * HH, (D - 1) * HH])
    pos = rng.uniform(0.1, 0.9, (n_all, 3)) * ext
    pos[:, 1] = -0.3 * DS
    vel = rng.normal(0, 0.08, (n_all, 3))
    vel[:, 1] = 1.0
    pos[7], vel[7] = [-0.2, 0.3, 0.4], [-1.0, 0.0, 0.0]            # outside, heading away
    pos[19], vel[19] = [0.5, -0.4, 0.5], [0.0, -1.0, 0.1]
    pos[33], vel[33] = [0.4, 0.5, 1.6], [0.1, 0.0, 1.0]
    pos[41], vel[41] = [-0.1, -0.2, 0.3], [0.0, 0.0, 1.0]          # outside, parallel to a face
    pos[52], vel[52] = [0.3, 1.4, -0.05], [1.0, 0.0, 0.0]
    pos[60], vel[60] = [1.2, 0.2, 0.2], [0.0, 1.0, 0.0]
    vel /= np.linalg.norm(vel, axis=1, keepdims=True)
    po = np.tile(np.array([[0.5, 0.8, 0.5]]) * ext, (n_all, 1))
    pd = np.tile(np.array([[0.1, 0.95, 0.05]]) / np.linalg.norm([0.1, 0.95, 0.05]), (n_all, 1))
    tg = rng.uniform(0.2, 0.8, (n_all, 3)) * ext
    tg[:, 1] = 0.9 * ext[1]
    ang, rad = rng.uniform(0, 2 * np.pi, n_all), RADIUS * rng.uniform(0, 0.8, n_all)
    cpos = np.stack([RADIUS + rad * np.cos(ang), np.zeros(n_all), RADIUS + rad * np.sin(ang)], -1)
    cvel = rng.normal(0, 0.1, (n_all, 3))
    cvel[:, 1] = 1.0
    cvel /= np.linalg.norm(cvel, axis=1, keepdims=True)
    ctg = np.stack([RADIUS + rng.normal(0, 0.1, n_all), np.full(n_all, LENGTH), RADIUS + rng.normal(0, 0.1, n_all)], -1)
    return dict(pos=pos, vel=vel, po=po, pd=pd, tg=tg, dx=rng.normal(size=(n_all, 3)), dv=rng.normal(size=(n_all, 3)),
                cpos=cpos, cvel=cvel, ctg=ctg)


@pytest.fixture(scope="module")
def scene(gpu):
    """{n: tensors of the n-ray case} on the GPU, made once and never written to."""
    from adjointnonlinearraytracing_amd import drrt
    rif, sdf = _field()
    r = {k: torch.tensor(v, dtype=torch.float32, device=gpu) for k, v in _rays().items()}
    grid = dict(rif=torch.tensor(rif, device=gpu), sdf=torch.tensor(sdf, device=gpu),
                prof=torch.tensor(np.sqrt(2.0 - np.linspace(0, 1, 8) ** 2), dtype=torch.float32, device=gpu))
    # the ray alone in the second adjoint block adds zeros (module docstring)
    drrt.TracerC().trace(grid["rif"], grid["rif"].shape, r["pos"], r["vel"], HH, DS)
    lone = int(drrt.last_order[64])
    for k in ("dx", "dv"):
        r[k][lone] = 0
        r[k][64] = 0
    out = {}
    for n in NS:
        s = dict(grid, **{k: v[:n].contiguous() for k, v in r.items()})
        if n:
            s["pos16"], s["vel16"] = drrt.encode_rays16((W, H, D), HH, s["pos"], s["vel"])
        else:
            s["pos16"] = s["vel16"] = torch.empty(0, 3, dtype=torch.int16, device=gpu)
        out[n] = s
    torch.cuda.synchronize()
    return out


RES = (W, H, D)
ADJOINTS = ("backtrace", "backtrace_rays", "backtrace_chunked", "backtrace_sdf", "backtrace_pln_rays", "backtrace_sdf_rays")


def _paired(c, s, method, order, n):
    """The forward that `method` is the adjoint of, then `method` with `order` ("none" / "live" / "copy" / "stale")."""
    T, drrt = c.T, c.drrt
    c.rec.name(**s)
    if method in ("backtrace", "backtrace_rays", "backtrace_chunked"):
        xt, vt = c.do("trace", T.trace, s["rif"], RES, s["pos"], s["vel"], HH, DS)
    elif method == "backtrace_pln_rays":
        xt, vt, _ = c.do("trace_pln", T.trace_pln, s["rif"], RES, s["pos"], s["vel"], s["po"], s["pd"], HH, DS)
    else:
        xt, vt = c.do("trace_sdf", T.trace_sdf, s["rif"], s["sdf"], RES, s["pos"], s["vel"], HH, DS)
    steps = c.quietly(drrt.keep_steps, drrt.last_steps)
    live = drrt.last_order
    o = dict(none=None, live=live, stale=live, copy=c.quietly(drrt.keep_order, live))[order]
    if order == "stale":
        c.quietly(T.trace, s["rif"], RES, s["pos"], s["vel"], HH, DS)
    c.rec.name(xt=xt, vt=vt, steps=steps, order_copy=o if order == "copy" else None)
    label = f"{method}(order={order})"
    if method == "backtrace":
        c.do(label, T.backtrace, s["rif"], RES, xt, vt, s["dx"], s["dv"], HH, DS, order=o)
    elif method == "backtrace_rays":
        if steps is None:                                   # no iteration counts were left (no rays): an empty tensor
            steps = torch.empty(0, dtype=torch.int32, device=xt.device)
        c.do(label, T.backtrace_rays, s["rif"], RES, s["pos"], s["vel"], xt, vt, steps, s["dx"], s["dv"], HH, DS, order=o)
    elif method == "backtrace_chunked":
        seen = []

        def on_chunk(k, grad, progress):
            c.rec.name(**{f"progress{k}": progress})
            seen.append((k, grad, progress))
        grad = c.do(label, T.backtrace_chunked, s["rif"], RES, xt, vt, s["dx"], s["dv"], HH, DS, order=o, chunks=3,
                    on_chunk=on_chunk)
        for k, g, progress in seen:
            p = c.quietly(drrt.decode_chunk_progress, progress)
            c.rec.lines.append(f"on_chunk({k}, grad is the result: {g.data_ptr() == grad.data_ptr()}, active={p['active']}, "
                               f"rays boxed={p['pos_min'] is not None}, samples boxed={p['sample_min'] is not None})")
    elif method == "backtrace_sdf":
        c.do(label, T.backtrace_sdf, s["rif"], s["sdf"], RES, xt, vt, s["dx"], s["dv"], HH, DS, order=o)
    elif method == "backtrace_pln_rays":
        c.do(label, T.backtrace_pln_rays, s["rif"], RES, s["pos"], s["vel"], s["po"], s["pd"], s["dx"], s["dv"], HH, DS, order=o)
    else:
        c.do(label, T.backtrace_sdf_rays, s["rif"], s["sdf"], RES, s["pos"], s["vel"], s["dx"], s["dv"], HH, DS, order=o)


# ---- drrt.TracerC / TracerS ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("order", ["none", "live", "copy", "stale"])
@pytest.mark.parametrize("method", ADJOINTS)
def test_adjoint_and_its_order(gpu, scene, monkeypatch, method, order, n):
    """Every adjoint that takes `order` (chunks=3 for the chunked one, with what on_chunk receives), behind its forward."""
    c = Case(monkeypatch, scene)
    _paired(c, scene[n], method, order, n)
    _check(f"{method}-{order}-n{n}", c)


@pytest.mark.gpu
@pytest.mark.parametrize("n", NS)
def test_remaining_methods(gpu, scene, monkeypatch, n):
    """trace_target and the fibre methods (the other public TracerC methods are in test_adjoint_and_its_order)."""
    c, s = Case(monkeypatch, scene), scene[n]
    c.rec.name(**s)
    T = c.T
    c.do("trace_target", T.trace_target, s["rif"], RES, s["pos"], s["vel"], s["tg"], HH, DS)
    xt, vt, _ = c.do("trace_cable", T.trace_cable, s["prof"], RADIUS, LENGTH, s["cpos"], s["cvel"], s["ctg"], CDS)
    c.rec.name(xt=xt, vt=vt)
    c.do("backtrace_cable", T.backtrace_cable, s["prof"], RADIUS, LENGTH, xt, vt, s["dx"], s["dv"], CDS)
    c.do("backtrace_cable_rays", T.backtrace_cable_rays, s["prof"], RADIUS, LENGTH, s["cpos"], s["cvel"], s["ctg"],
         s["dx"], s["dv"], CDS)
    _check(f"remaining-n{n}", c)


@pytest.mark.gpu
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("fmt", ["fp32", "f16", "q16", "qpos"])
def test_ray_formats(gpu, scene, monkeypatch, fmt, n):
    """trace and backtrace in the four ray-state formats."""
    c, s = Case(monkeypatch, scene), scene[n]
    pos = s["pos16"] if fmt in ("q16", "qpos") else s["pos"].half() if fmt == "f16" else s["pos"]
    vel = s["vel16"] if fmt == "q16" else s["vel"].half() if fmt == "f16" else s["vel"]
    dx, dv = (s["dx"].half(), s["dv"].half()) if fmt in ("f16", "q16") else (s["dx"], s["dv"])
    c.rec.name(rif=s["rif"], pos=pos, vel=vel, dx=dx, dv=dv)
    xt, vt = c.do("trace", c.T.trace, s["rif"], RES, pos, vel, HH, DS)
    assert xt.dtype == pos.dtype and vt.dtype == vel.dtype
    c.rec.name(xt=xt, vt=vt)
    c.do("backtrace", c.T.backtrace, s["rif"], RES, xt, vt, dx, dv, HH, DS, order=c.drrt.last_order)
    c.do("backtrace, own sort", c.T.backtrace, s["rif"], RES, xt, vt, dx, dv, HH, DS)
    _check(f"format-{fmt}-n{n}", c)


OPTIONS = [dict(sort_rays=False), dict(pair_grid=True), dict(pair_grid=False), dict(pair_grid="auto"), dict(corrected_h=True)] + \
    [dict(adjoint_window=w) for w in ("auto", "box", "ring", "ring_sparse", "ring_direct", "ring_general")]


@pytest.mark.gpu
@pytest.mark.parametrize("opts", OPTIONS, ids=lambda o: "-".join(f"{k}={v}" for k, v in o.items()))
def test_options(gpu, scene, monkeypatch, opts):
    """Per-call options: trace, the paired and the self-sorting backtrace, and the ray-state adjoint under each."""
    c, s = Case(monkeypatch, scene), scene[65]
    c.rec.name(**s)
    with c.drrt.using(**opts):
        xt, vt = c.do("trace", c.T.trace, s["rif"], RES, s["pos"], s["vel"], HH, DS)
        steps, order = c.quietly(c.drrt.keep_steps, c.drrt.last_steps), c.drrt.last_order
        c.rec.name(xt=xt, vt=vt, steps=steps)
        c.do("backtrace(order=live)", c.T.backtrace, s["rif"], RES, xt, vt, s["dx"], s["dv"], HH, DS, order=order)
        c.do("backtrace_rays(order=live)", c.T.backtrace_rays, s["rif"], RES, s["pos"], s["vel"], xt, vt, steps, s["dx"],
             s["dv"], HH, DS, order=order)
        c.do("backtrace(order=None)", c.T.backtrace, s["rif"], RES, xt, vt, s["dx"], s["dv"], HH, DS)
    _check("options-" + "-".join(f"{k}={v}" for k, v in opts.items()), c)


@pytest.mark.gpu
def test_tracer_s(gpu, scene, monkeypatch):
    """The four TracerS methods on host tensors: staged, the TracerC calls, results back on the host."""
    c = Case(monkeypatch, scene)
    s = {k: v.cpu() for k, v in scene[65].items()}
    S = c.drrt.TracerS()
    xt, vt = c.do("trace", S.trace, s["rif"], RES, s["pos"], s["vel"], HH, DS)
    assert not xt.is_cuda and not vt.is_cuda
    out = c.do("trace_sdf", S.trace_sdf, s["rif"], s["sdf"], RES, s["pos"], s["vel"], HH, DS)
    out += c.do("trace_target", S.trace_target, s["rif"], RES, s["pos"], s["vel"], s["tg"], HH, DS)
    grad = c.do("backtrace", S.backtrace, s["rif"], RES, xt, vt, s["dx"], s["dv"], HH, DS)
    assert isinstance(out, tuple) and len(out) == 5 and not any(t.is_cuda for t in out + (grad,))
    _check("tracer_s", c)


def _refusals(c, s):
    T, i16 = c.T, s["pos16"]
    rays = (s["rif"], RES, s["pos"], s["vel"])
    adj = (s["rif"], RES, s["pos"], s["vel"], s["dx"], s["dv"])
    return {
        "cpu tensor": (T.trace, (s["rif"].cpu(),) + rays[1:] + (HH, DS), "TracerC expects tensors on the cuda (ROCm) device"),
        "ray shape": (T.trace, (s["rif"], RES, s["pos"].reshape(3, -1), s["vel"], HH, DS), "expected a (N,3) ray tensor"),
        "mismatched n": (T.trace, (s["rif"], RES, s["pos"], s["vel"][:7], HH, DS), "expected a (65,3) ray tensor, got (7, 3)"),
        "mismatched n, adjoint": (T.backtrace, adj[:5] + (s["dv"][:7], HH, DS), "expected a (65,3) ray tensor, got (7, 3)"),
        "codes to trace_pln": (T.trace_pln, (s["rif"], RES, i16, s["vel"], s["po"], s["pd"], HH, DS),
                               "torch.int16 ray tensor where this call takes floating-point values"),
        "codes as directions only": (T.trace, (s["rif"], RES, s["pos"], s["vel16"], HH, DS),
                                     "torch.int16 ray tensor where this call takes floating-point values"),
        "int32 rays": (T.trace, (s["rif"], RES, s["pos"].to(torch.int32), s["vel"], HH, DS),
                       "torch.int32 ray tensor where this call takes floating-point values"),
        "codes as seeds": (T.backtrace, adj[:4] + (i16, s["dv"], HH, DS),
                           "torch.int16 ray tensor where this call takes floating-point values"),
        "int32 next to codes": (T.trace, (s["rif"], RES, i16, s["vel"].to(torch.int32), HH, DS),
                                "torch.int32 ray tensor where this call takes floating-point values"),
        "q16 rays, fp32 seeds": (T.backtrace, (s["rif"], RES, i16, s["vel16"], s["dx"], s["dv"], HH, DS),
                                 "q16 exit rays (int16) go with float16 seeds dx, dv"),
        "sdf size": (T.trace_sdf, (s["rif"], s["sdf"].reshape(-1)[:-1]) + rays[1:] + (HH, DS), "Resolution doesn't match data"),
        "sdf size, adjoint": (T.backtrace_sdf, (s["rif"], s["sdf"].reshape(-1)[:-1]) + adj[1:] + (HH, DS),
                              "Resolution doesn't match data"),
        "sdf size, ray adjoint": (T.backtrace_sdf_rays, (s["rif"], s["sdf"].reshape(-1)[:-1]) + adj[1:] + (HH, DS),
                                  "Resolution doesn't match data"),
        "steps dtype": (T.backtrace_rays, adj[:4] + adj[2:4] + (torch.zeros(65, dtype=torch.int64, device=s["rif"].device),)
                        + adj[4:] + (HH, DS), "steps must be 65 int32 iteration counts"),
        "steps length": (T.backtrace_rays, adj[:4] + adj[2:4] + (torch.zeros(64, dtype=torch.int32, device=s["rif"].device),)
                         + adj[4:] + (HH, DS), "steps must be 65 int32 iteration counts"),
        "res of length 2": (T.trace, (s["rif"], RES[:2], s["pos"], s["vel"], HH, DS), "res must have 3 entries"),
        "res of length 2, adjoint": (T.backtrace, (s["rif"], RES[:2]) + adj[2:] + (HH, DS), "res must have 3 entries"),
    }


@pytest.mark.gpu
def test_python_side_refusals(gpu, scene, monkeypatch):
    """What the layer refuses itself: the message, and no march entry of the library called.  (The size query and the
    clearing of the hints, which the transcript shows where they happen, launch nothing.)"""
    c, s = Case(monkeypatch, scene), scene[65]
    c.rec.name(**{k: v for k, v in s.items() if k in ("rif", "sdf", "pos", "vel", "dx", "dv", "po", "pd")})
    for label, (fn, args, message) in _refusals(c, s).items():
        before = len(c.rec.lines)
        assert c.do(label, fn, *args) is None
        said = [ln for ln in c.rec.lines[before:] if ln.startswith("raised: ")]
        assert len(said) == 1 and message in said[0], (label, said)
        assert not [ln for ln in c.rec.lines[before:] if _is_march(ln.split("(")[0])], (label, c.rec.lines[before:])
        assert c.rec.lines[-1].endswith("launches="), (label, c.rec.lines[-1])
    _check("refusals", c)


# ---- the autograd classes ----------------------------------------------------------------------------------------------
def _classes():
    from adjointnonlinearraytracing_amd import dist, tracer
    return {"BackTracerC": (tracer.BackTracerC, "trace"), "ADTracerC": (tracer.ADTracerC, "trace"),
            "ShardedBackTracerC": (dist.ShardedBackTracerC, "trace"),
            "BackPlaneTracerC": (tracer.BackPlaneTracerC, "pln"), "ADPlaneTracerC": (tracer.ADPlaneTracerC, "pln"),
            "ADRayPlaneTracerC": (tracer.ADRayPlaneTracerC, "pln"),
            "BackTargetTracerC": (tracer.BackTargetTracerC, "target"),
            "BackSDFTracerC": (tracer.BackSDFTracerC, "sdf"), "ADSDFTracerC": (tracer.ADSDFTracerC, "sdf"),
            "ADRaySDFTracerC": (tracer.ADRaySDFTracerC, "sdf"),
            "BackCableTracerC": (tracer.BackCableTracerC, "cable"), "ADCableTracerC": (tracer.ADCableTracerC, "cable")}


CLASS_NAMES = ["BackTracerC", "ADTracerC", "ShardedBackTracerC", "BackPlaneTracerC", "ADPlaneTracerC", "ADRayPlaneTracerC",
               "BackTargetTracerC", "BackSDFTracerC", "ADSDFTracerC", "ADRaySDFTracerC", "BackCableTracerC", "ADCableTracerC"]


@pytest.fixture(scope="module")
def direct(scene):
    """{family: (dL/drif, dL/dx, dL/dv)} from the direct TracerC calls, in the forward's visit order: made once."""
    from adjointnonlinearraytracing_amd import drrt
    T, s = drrt.TracerC(), scene[65]
    res = tuple(s["rif"].shape)                      # what the autograd classes pass
    out = {}
    xt, vt = T.trace(s["rif"], res, s["pos"], s["vel"], HH, DS)
    steps, order = drrt.keep_steps(drrt.last_steps), drrt.keep_order(drrt.last_order)
    out["trace"] = (T.backtrace(s["rif"], res, xt, vt, s["dx"], s["dv"], HH, DS, order=order).reshape(res),) + \
        T.backtrace_rays(s["rif"], res, s["pos"], s["vel"], xt, vt, steps, s["dx"], s["dv"], HH, DS, order=order)
    xt, vt, fm = T.trace_pln(s["rif"], res, s["pos"], s["vel"], s["po"], s["pd"], HH, DS)
    order = drrt.keep_order(drrt.last_order)
    out["pln"] = (T.backtrace(s["rif"], res, xt, vt, s["dx"], s["dv"], HH, DS, order=order).reshape(res),) + \
        T.backtrace_pln_rays(s["rif"], res, s["pos"], s["vel"], s["po"], s["pd"], s["dx"], s["dv"], HH, DS, order=order)
    xt, vt, _ = T.trace_target(s["rif"], res, s["pos"], s["vel"], s["tg"], HH, DS)
    order = drrt.keep_order(drrt.last_order)
    out["target"] = (T.backtrace(s["rif"], res, xt, vt, s["dx"], s["dv"], HH, DS, order=order).reshape(res), None, None)
    xt, vt = T.trace_sdf(s["rif"], s["sdf"], res, s["pos"], s["vel"], HH, DS)
    order = drrt.keep_order(drrt.last_order)
    out["sdf"] = (T.backtrace_sdf(s["rif"], s["sdf"], res, xt, vt, s["dx"], s["dv"], HH, DS, order=order).reshape(res),) + \
        T.backtrace_sdf_rays(s["rif"], s["sdf"], res, s["pos"], s["vel"], s["dx"], s["dv"], HH, DS, order=order)
    xt, vt, _ = T.trace_cable(s["prof"], RADIUS, LENGTH, s["cpos"], s["cvel"], s["ctg"], CDS)
    out["cable"] = (T.backtrace_cable(s["prof"], RADIUS, LENGTH, xt, vt, s["dx"], s["dv"], CDS),) + \
        T.backtrace_cable_rays(s["prof"], RADIUS, LENGTH, s["cpos"], s["cvel"], s["ctg"], s["dx"], s["dv"], CDS)
    torch.cuda.synchronize()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("v_grad", [True, False])
@pytest.mark.parametrize("x_grad", [True, False])
@pytest.mark.parametrize("rif_grad", [True, False])
@pytest.mark.parametrize("name", CLASS_NAMES)
def test_autograd_classes(gpu, scene, direct, monkeypatch, name, rif_grad, x_grad, v_grad):
    """The nine classes, the two aliases and ShardedBackTracerC on one rank: forward and backward transcripts, which
    gradients come back, and every gradient bit for bit the direct TracerC call's."""
    cls, family = _classes()[name]
    with_ray_grads = name in ("ADTracerC", "ADRayPlaneTracerC", "ADRaySDFTracerC", "ADCableTracerC")
    c, s = Case(monkeypatch, scene), scene[65]
    cable = family == "cable"
    rif = (s["prof"] if cable else s["rif"]).clone().requires_grad_(rif_grad)
    x = (s["cpos"] if cable else s["pos"]).clone().requires_grad_(x_grad)
    v = (s["cvel"] if cable else s["vel"]).clone().requires_grad_(v_grad)
    c.rec.name(rif=rif, x=x, v=v, **{k: s[k] for k in ("sdf", "po", "pd", "tg", "ctg")})
    args = dict(trace=(rif, x, v, HH, DS), pln=(rif, x, v, s["po"], s["pd"], HH, DS), target=(rif, x, v, s["tg"], HH, DS),
                sdf=(rif, s["sdf"], x, v, HH, DS), cable=(rif, RADIUS, LENGTH, x, v, s["ctg"], CDS))[family]
    out = c.do("forward", cls.apply, *args)
    assert len(out) == dict(trace=2, pln=3, target=3, sdf=2, cable=3)[family]
    if family == "pln":
        assert out[2].dtype == torch.bool and not out[2].requires_grad
    c.rec.name(xt=out[0], vt=out[1])
    if rif_grad or x_grad or v_grad:
        loss = (out[0] * s["dx"]).sum() + (out[1] * s["dv"]).sum()
        c.do("backward", loss.backward)
        g_rif, g_x, g_v = direct[family]
        assert (rif.grad is not None) == rif_grad
        assert (x.grad is not None) == (x_grad and with_ray_grads) and (v.grad is not None) == (v_grad and with_ray_grads)
        for got, want in ((rif.grad, g_rif), (x.grad, g_x), (v.grad, g_v)):
            assert got is None or torch.equal(got, want.reshape(got.shape))
    else:
        assert not out[0].requires_grad
    _check(f"{name}-rif{int(rif_grad)}-x{int(x_grad)}-v{int(v_grad)}", c)
