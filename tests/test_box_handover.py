"""The cell hand-over of the box-window adjoint (k_backtrace_flat, csrc/drrt_adjoint_box.hip): every way a ray can leave a
cell -- across one face in each of the six directions (to the LDS window, pair / quad pre-reduced, or to the grid when the
cell lies outside the window), across several faces or into / out of a clamped cell (all eight corners), at the end of the
ray or of a depth chunk -- on a NON-CUBIC 20 x 24 x 28 grid (a swapped stride shows), larger than the 9^3 window in every axis
(the window re-anchors and flushes), in a smooth asymmetric medium, with per-ray seeds of very different magnitudes (a corner
sent to the wrong slot changes the result).

Every case forces the box kernel (DRRT_FLAG_STATIC_WINDOW), with and without DRRT_FLAG_SORT_RAYS and DRRT_FLAG_PAIR_GRID, and
compares its gradient with the one-atomic-per-tap kernel's (DRRT_FLAG_DIRECT_ATOMICS) on the same exit rays and with the
oracle's backtrace: rel-L2 <= 2e-5 (the project's bound), step totals equal and non-zero.  The instantiation with the event
counters (DRRT_FLAG_DEBUG_COUNTERS) runs beside the product one, is held to the same bound, and its counters, summed
over the cases, must show that every path of the hand-over ran."""
import ctypes as C

import numpy as np
import pytest
import torch

import cases

pytestmark = pytest.mark.gpu

W, H, D = 20, 24, 28
HV = 0.05                                         # voxel size
EXT = np.array([(W - 1) * HV, (H - 1) * HV, (D - 1) * HV])
N = 1000                                          # rays per case: not a multiple of 64, 16 bundles
BOUND = 2e-5
COUNTERS = {"flushes": 0, "face_window": 0, "face_adds": 0, "face_global": 0, "all_eight": 0, "wave_steps": 0,
            "multi_axis": 0, "clamped": 0}
_DBG_SLOT = {"flushes": 0, "face_window": 4, "face_adds": 5, "face_global": 6, "all_eight": 7, "wave_steps": 8,
             "multi_axis": 9, "clamped": 15}


def _medium():
    z, y, x = np.meshgrid(np.linspace(0, 1, D), np.linspace(0, 1, H), np.linspace(0, 1, W), indexing="ij")
    rif = 1.0 + 0.08 * np.exp(-((x - 0.4) ** 2 / 0.09 + (y - 0.65) ** 2 / 0.16 + (z - 0.8) ** 2 / 0.2)) \
        + 0.02 * np.sin(3 * x + 1) * np.cos(2 * y) + 0.015 * z * z
    sdf = 0.45 - y * EXT[1] + 0.1 * x * EXT[0]      # negative beyond a tilted plane in the middle of the volume
    return rif.astype(np.float32), sdf.astype(np.float32)


def _seeds(n, rng):
    """adjoint seeds whose magnitude varies over two decades from ray to ray"""
    mag = 10.0 ** rng.uniform(-1.0, 1.0, (n, 1))
    return (rng.normal(size=(n, 3)) * mag).astype(np.float32), (rng.normal(size=(n, 3)) * mag).astype(np.float32)


def _beam(axis, sign, rng, n=N, centre=(0.42, 0.58, 0.47), half_cells=2.5, tilt=0.02, beyond=0.3, ds=HV / 2, copies=1, jitter=None):
    """Exit rays of a collimated beam that travelled along sign * axis: they stand `beyond` steps past the face the beam left
    through, on a patch of 2 * half_cells cells around `centre` (fractions of the extents), and the adjoint marches them back
    through the whole volume.  copies = 4: every ray four times in a row (a quad of lanes shares its cells); with `jitter`
    (cells) the third and fourth copy are moved by that much across the beam, so pairs share cells and quads do not."""
    m = n // copies
    pos = np.asarray(centre) * EXT + rng.uniform(-half_cells, half_cells, (m, 3)) * HV
    pos[:, axis] = EXT[axis] + beyond * ds if sign > 0 else -beyond * ds
    vel = rng.normal(0.0, tilt, (m, 3))
    vel[:, axis] = sign
    pos, vel = np.repeat(pos, copies, axis=0), np.repeat(vel, copies, axis=0)
    if jitter is not None:
        t = (axis + 1) % 3
        pos[2::4, t] += jitter * HV; pos[3::4, t] += jitter * HV
        pos += rng.uniform(-1e-3, 1e-3, pos.shape) * HV * (np.arange(3) != axis)
    return pos.astype(np.float32), vel.astype(np.float32), ds


def _oblique(direction, ds, rng):
    """a beam oblique to all three axes that ended inside the volume: two- and three-face jumps on the way back"""
    d = np.asarray(direction, np.float64); d /= np.linalg.norm(d)
    start = np.where(d > 0, 0.8, 0.2) * EXT
    pos = start + rng.uniform(-2.0, 2.0, (N, 3)) * HV
    vel = d + rng.normal(0.0, 0.02, (N, 3))
    return pos.astype(np.float32), vel.astype(np.float32), ds


def _grazing(face, rng):
    """a beam along another axis whose rays straddle the box face `face` (0..5 = x0 x1 y0 y1 z0 z1): some run in the clamped
    cells outside it, some in the regular cells inside, and the tilt across the face moves rays from one kind to the other"""
    a, far = face // 2, face % 2
    along = (a + 1) % 3
    pos, vel, ds = _beam(along, 1, rng, tilt=0.02)
    edge = EXT[a] if far else 0.0
    pos[:, a] = edge + rng.uniform(-1.0, 1.6, N) * HV * (-1.0 if far else 1.0)
    vel[:, a] = rng.normal(0.0, 0.08, N)
    return pos, vel, ds


def _spread(rng):
    """exit rays all over the far y face, in random order and with a wide fan: the bundles are incoherent, cells miss the
    window, the window stays put for its cool-down and one-face leaves go to the grid"""
    pos = rng.uniform(0.04, 0.96, (N, 3)) * EXT
    pos[:, 1] = EXT[1] + 0.3 * HV / 2
    vel = rng.normal(0.0, 0.15, (N, 3))
    vel[:, 1] = 1.0
    return pos.astype(np.float32), vel.astype(np.float32), HV / 2


def _case_table():
    t = {}
    for k, (axis, sign) in enumerate(((0, 1), (0, -1), (1, 1), (1, -1), (2, 1), (2, -1))):
        name = "xyz"[axis] + ("+" if sign > 0 else "-")
        t["beam" + name] = lambda rng, a=axis, s=sign: _beam(a, s, rng)
        t["quads" + name] = lambda rng, a=axis, s=sign: _beam(a, s, rng, copies=4)
        t["pairs" + name] = lambda rng, a=axis, s=sign: _beam(a, s, rng, copies=4, jitter=1.5)
        t["graze" + "xyz"[k // 2] + "01"[k % 2]] = lambda rng, f=k: _grazing(f, rng)
    t["oblique_half"] = lambda rng: _oblique((1.0, 0.8, 0.6), HV / 2, rng)
    t["oblique_half_mixed"] = lambda rng: _oblique((-0.7, 1.0, -0.9), HV / 2, rng)
    t["oblique_full"] = lambda rng: _oblique((1.0, 0.8, 0.6), HV, rng)
    t["oblique_full_mixed"] = lambda rng: _oblique((-0.7, 1.0, -0.9), HV, rng)
    t["outside"] = lambda rng: _beam(2, 1, rng, beyond=6.5)          # three cells beyond the far z face
    t["spread"] = _spread
    return t


CASES = _case_table()
FLAG_SETS = (("plain", 0), ("sort", 1), ("pair", 64), ("sort_pair", 65))
_results = {}


class _Gpu:
    """the grid on the device and the C-ABI calls of this file"""
    _inst = None

    def __init__(self, dev):
        from adjointnonlinearraytracing_amd import _lib
        self.L, self.lib, self.dev = _lib, _lib.load(), dev
        self.rif_np, self.sdf_np = _medium()
        self.rif = torch.from_numpy(self.rif_np).reshape(-1).to(dev)
        self.sdf = torch.from_numpy(self.sdf_np).reshape(-1).to(dev)
        self.nvox = self.rif.numel()
        self.res = (C.c_int * 3)(W, H, D)
        self.stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    @classmethod
    def get(cls, dev):
        if cls._inst is None:
            cls._inst = cls(dev)
        return cls._inst

    def backtrace(self, rays, ds, flags, sdf=False):
        """-> (grad float64[nvox], ray_steps, counters or None)"""
        p = lambda t: C.c_void_p(t.data_ptr())
        xt, vt, dx, dv = rays
        n = xt.shape[0]
        ws = torch.empty(int(self.lib.drrt_workspace_bytes_grid(n, self.nvox, flags)) + 1024, dtype=torch.uint8, device=self.dev)
        grad = torch.empty(self.nvox, dtype=torch.float32, device=self.dev)
        st = torch.zeros(3, dtype=torch.int64, device=self.dev)
        if sdf:
            rc = self.lib.drrt_backtrace_sdf_f32(p(self.rif), p(self.sdf), self.nvox, self.res, n, p(xt), p(vt), p(dx), p(dv), HV, ds,
                                                 p(grad), p(st), p(ws), ws.numel(), flags, self.stream)
        else:
            rc = self.lib.drrt_backtrace_f32(p(self.rif), self.nvox, self.res, n, p(xt), p(vt), p(dx), p(dv), HV, ds, p(grad), p(st),
                                             p(ws), ws.numel(), flags, self.stream)
        self.L.check(rc)
        torch.cuda.synchronize()
        ctr = None
        if flags & self.L.FLAG_DEBUG_COUNTERS:
            o = (ws.numel() - 512) & ~7
            ctr = ws[o:o + 512].view(torch.int64).cpu().tolist()
        return grad.cpu().numpy().astype(np.float64), int(st[0].item()), ctr

    def chunked(self, rays, ds, flags, K):
        """the march in K depth chunks (drrt_backtrace_chunk_f32) -> (grad, ray_steps)"""
        p = lambda t: C.c_void_p(t.data_ptr())
        xt, vt, dx, dv = rays
        n = xt.shape[0]
        ws = torch.empty(int(self.lib.drrt_workspace_bytes_grid(n, self.nvox, flags)) + 1024, dtype=torch.uint8, device=self.dev)
        state = torch.empty(int(self.lib.drrt_backtrace_chunk_state_bytes(n)), dtype=torch.uint8, device=self.dev)
        grad = torch.empty(self.nvox, dtype=torch.float32, device=self.dev)
        st = torch.zeros(3, dtype=torch.int64, device=self.dev)
        total = int(self.lib.drrt_backtrace_max_steps(self.res, HV, ds))
        per = (total + K - 1) // K
        for k in range(K):
            if k > 0 and flags & self.L.FLAG_SORT_RAYS:
                self.lib.drrt_set_order_hint(self.lib.drrt_last_order(None), n)
            self.L.check(self.lib.drrt_backtrace_chunk_f32(p(self.rif), self.nvox, self.res, n, p(xt), p(vt), p(dx), p(dv), HV, ds,
                                                           p(grad), p(st), p(ws), ws.numel(), flags, self.stream, p(state),
                                                           state.numel(), k * per, per if k < K - 1 else -1, None))
        torch.cuda.synchronize()
        return grad.cpu().numpy().astype(np.float64), int(st[0].item())


def _rays(name, dev):
    import zlib
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    pos, vel, ds = CASES[name](rng)
    dx, dv = _seeds(pos.shape[0], rng)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return (pos, vel, dx, dv), tuple(to(a) for a in (pos, vel, dx, dv)), ds


def _run(name, dev, oracle):
    """One ray set through the oracle, the one-atomic-per-tap kernel and the box kernel under every flag set (product and
    counter instantiation); the figures of every comparison, computed once per session."""
    if name in _results:
        return _results[name]
    G = _Gpu.get(dev)
    host, rays, ds = _rays(name, dev)
    with oracle.arith("factored"):
        ob = oracle.backtrace(G.rif_np, (W, H, D), *host, HV, ds, dtype=np.float32)
    g_direct, st_direct, _ = G.backtrace(rays, ds, G.L.FLAG_DIRECT_ATOMICS)
    out = {"steps_oracle": int(ob["steps_total"]), "steps_direct": st_direct, "runs": {}}
    for fname, fl in FLAG_SETS:
        for inst, extra in (("product", 0), ("counters", G.L.FLAG_DEBUG_COUNTERS)):
            g, st, ctr = G.backtrace(rays, ds, fl | G.L.FLAG_STATIC_WINDOW | extra)
            out["runs"][fname, inst] = dict(steps=st, vs_direct=cases.rel_l2(g, g_direct), vs_oracle=cases.rel_l2(g, ob["grad"]))
            if ctr is not None:
                for k, slot in _DBG_SLOT.items():
                    COUNTERS[k] += ctr[slot]
    _results[name] = out
    return out


@pytest.mark.parametrize("name", sorted(CASES))
def test_box_handover_equals_direct_atomics_and_oracle(gpu, oracle, name):
    r = _run(name, gpu, oracle)
    print(name, r)
    assert r["steps_oracle"] > 0 and r["steps_direct"] == r["steps_oracle"], (name, r)
    for key, run in r["runs"].items():
        assert run["steps"] == r["steps_oracle"], (name, key, run)
        assert run["vs_direct"] <= BOUND, (name, key, run)
        assert run["vs_oracle"] <= BOUND, (name, key, run)


@pytest.mark.parametrize("fname,fl", FLAG_SETS)
def test_box_handover_backtrace_sdf(gpu, oracle, fname, fl):
    """MODE 1 of the same source: the ray also ends where its sdf sample turns non-negative -- in the middle of the volume,
    with a cell's accumulators to hand over."""
    G = _Gpu.get(gpu)
    host, rays, ds = _rays("beamy+", gpu)
    with oracle.arith("factored"):
        ob = oracle.backtrace(G.rif_np, (W, H, D), *host, HV, ds, dtype=np.float32, sdf=G.sdf_np)
        full = oracle.backtrace(G.rif_np, (W, H, D), *host, HV, ds, dtype=np.float32)
    g_direct, st_direct, _ = G.backtrace(rays, ds, G.L.FLAG_DIRECT_ATOMICS, sdf=True)
    g, st, _ = G.backtrace(rays, ds, fl | G.L.FLAG_STATIC_WINDOW, sdf=True)
    print(fname, st, ob["steps_total"], full["steps_total"], cases.rel_l2(g, g_direct), cases.rel_l2(g, ob["grad"]))
    assert 0 < ob["steps_total"] < full["steps_total"]          # the sdf did end the rays early
    assert st == st_direct == ob["steps_total"]
    assert cases.rel_l2(g, g_direct) <= BOUND
    assert cases.rel_l2(g, ob["grad"]) <= BOUND


@pytest.mark.parametrize("fname,fl", FLAG_SETS)
def test_box_handover_chunked(gpu, oracle, fname, fl):
    """CHUNK instantiation: drrt_backtrace_chunk_f32 with K = 3 against one launch, the one-atomic-per-tap kernel and the oracle"""
    G = _Gpu.get(gpu)
    host, rays, ds = _rays("beamz-", gpu)
    with oracle.arith("factored"):
        ob = oracle.backtrace(G.rif_np, (W, H, D), *host, HV, ds, dtype=np.float32)
    g_direct, st_direct, _ = G.backtrace(rays, ds, G.L.FLAG_DIRECT_ATOMICS)
    g_one, st_one, _ = G.backtrace(rays, ds, fl | G.L.FLAG_STATIC_WINDOW)
    g, st = G.chunked(rays, ds, fl | G.L.FLAG_STATIC_WINDOW, 3)
    print(fname, st, cases.rel_l2(g, g_one), cases.rel_l2(g, g_direct), cases.rel_l2(g, ob["grad"]))
    assert ob["steps_total"] > 0 and st == st_one == st_direct == ob["steps_total"]
    assert cases.rel_l2(g, g_one) <= BOUND
    assert cases.rel_l2(g, g_direct) <= BOUND
    assert cases.rel_l2(g, ob["grad"]) <= BOUND


def test_box_handover_cases_exercise_every_path(gpu, oracle):
    """The event counters of the counter instantiation, summed over all the ray sets above: window flushes, one-face leaves
    handed to the window (some of them pre-reduced away: fewer lanes add than leave) and to the grid, all-eight leaves,
    wave-steps whose lanes leave across two or more axes, ray-steps in clamped cells."""
    for name in sorted(CASES):
        _run(name, gpu, oracle)
    print(COUNTERS)
    assert COUNTERS["flushes"] > 0
    assert COUNTERS["face_window"] > 0
    assert 0 < COUNTERS["face_adds"] < COUNTERS["face_window"]
    assert COUNTERS["face_global"] > 0
    assert COUNTERS["all_eight"] > 0
    assert COUNTERS["wave_steps"] > 0
    assert COUNTERS["multi_axis"] > 0
    assert COUNTERS["clamped"] > 0
