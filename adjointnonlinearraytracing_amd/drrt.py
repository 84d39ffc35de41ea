"""`drrt` module mirror: ``TracerC`` / ``TracerS`` objects with the reference's method names and
argument order (``/root/reference/src/drrt.cpp:21-59``, ``include/tracer.h:15-89``), operating on
torch tensors instead of enoki arrays and backed by the hand-written HIP kernels in
``csrc/`` through the C ABI (``include/drrt_hip.h``).

* ``TracerC`` -- tensors on the ``cuda`` (ROCm) device; asynchronous on torch's current stream.
* ``TracerS`` -- the reference's CPU class (``Tracer<false,false>``, binds trace / trace_sdf /
  trace_target / backtrace only, ``src/drrt.cpp:38-45``).  Here it accepts CPU tensors, stages
  them to the GPU, runs the SAME HIP kernels and copies the results back: there is deliberately
  no CPU compute path in this package.
* ``TracerD`` (enoki autodiff, ``src/drrt.cpp:28-36``) is out of scope; constructing it raises.

All methods ``detach()`` / ``contiguous()`` / cast to fp32 exactly where the reference narrows
(``core/tracer.py:299-301``, ``include/tracer.h:20-21``); ``res`` may be any 3-sequence
(``torch.Size`` is what the scripts pass, ``core/tracer.py:298,307``).  Ray tensors of any floating-point dtype are
converted to fp32 by value; integer ray tensors are codes of the 16-bit ray state and are refused wherever the call does not
select it (``_rays``).
"""
from __future__ import annotations

import contextlib
import ctypes as C
import dataclasses
import threading
from dataclasses import dataclass
from typing import Dict, Optional, Sequence, Tuple

import torch

from . import _lib
from ._lib import _p, _stream


@dataclass
class Options:
    sort_rays: bool = True        # locality-sort rays by entry voxel (DRRT_FLAG_SORT_RAYS)
    corrected_h: bool = False     # adjoint: divide gradient splat by h; default = as written
    check_failed: bool = True     # print "failed to exit all rays" like src/tracer.cpp:89-90 (asynchronously: no host
                                  # sync per call; the message may appear one call late -- see flush_warnings())
    direct_atomics: bool = False  # adjoint: one global atomic per tap (debug / A-B)
    adjoint_window: str = "auto"  # adjoint: "auto" = the bundles of the call are classified on the device and the box-window kernel
                                  # (k_backtrace_flat) or the ring-window kernel (k_backtrace_ring; its general or its
                                  # sparse-only instantiations) runs; "box" / "ring" / "ring_sparse" / "ring_direct" force one, "ring_general"
                                  # keeps the choice but never takes the sparse-only instantiation (A-B)
    chord_key: bool = False       # locality sort with the rounds-1/2 key (DRRT_FLAG_CHORD_KEY, A-B)
    pair_grid: object = "auto"    # the "pair copy" of the grid in the workspace (DRRT_FLAG_PAIR_GRID; 8 bytes per voxel, two
                                  # 16-byte gathers per cell instead of four 8-byte ones).  True, False, or "auto" = a
                                  # forward march builds it when the call keeps the whole GPU busy and does enough
                                  # ray-steps per voxel to pay for the copy, and the adjoint paired with that forward
                                  # reuses it.  Bit-identical; 256^3 / 1M rays: forward 1.31 -> 1.06 ms (+0.05 ms for the
                                  # copy), adjoint -2 %

    @property
    def quad_grid(self):          # round-1 name
        return self.pair_grid

    @quad_grid.setter
    def quad_grid(self, v):
        self.pair_grid = v


options = Options()          # the process-wide defaults

# Per-thread overrides: `with drrt.using(sort_rays=False): ...` changes the options of the calls made by THIS thread inside
# the block and nothing else (two threads with different settings do not race on the module global; the visit-order hint
# of the C ABI is per thread in the same way).  Calls outside any block read the module-level `options`.
_tls = threading.local()


def _opt() -> Options:
    return getattr(_tls, "options", None) or options


@contextlib.contextmanager
def using(**overrides):
    """Context manager: the tracer calls of the current thread run with `overrides` applied on top of the options in
    effect (``with drrt.using(corrected_h=True, pair_grid=False): ...``); restored on exit, nestable."""
    prev = getattr(_tls, "options", None)
    _tls.options = dataclasses.replace(prev or options, **overrides)
    try:
        yield _tls.options
    finally:
        _tls.options = prev

# last call's statistics (ray_steps, n_failed, iters) as a device tensor of 3 int64 words
last_stats: Optional[torch.Tensor] = None

# Visit order (int32 ray indices) used by the last SORTED forward call: a VIEW into that call's workspace, valid until
# the next call on the same (device, stream) that sorts rays or stores state there -- any trace*, or a backtrace* that is
# not given an order.  A stale view is recognised (generation stamp `drrt_gen`) and ignored by the calls it is handed
# to, which then sort for themselves: slower, never wrong.  Holders that outlive the next call -- tracer.Back*TracerC's
# ctx, dist.ShardedBackTracerC -- take a private copy with keep_order().  Handed to the paired backtrace
# (drrt_set_order_hint) the adjoint visits rays in the forward's bundle order (include/drrt_hip.h, "visit order hand-over").
last_order: Optional[torch.Tensor] = None
# Per-ray iteration counts (int32, caller ray order) of the last trace / trace_pln call, whether or not it sorted: a
# workspace VIEW with the same lifetime rules as `last_order` (keep_steps() takes the private copy).  The ray-state
# adjoint (TracerC.backtrace_rays) needs them.
last_steps: Optional[torch.Tensor] = None
_order_gen: Dict[tuple, int] = {}            # per workspace key: how often its order / state region has been rewritten

# one scratch buffer per (device, stream): calls queued on different streams must not share scratch
_workspaces: Dict[tuple, torch.Tensor] = {}


def _wkey(device: torch.device) -> tuple:
    return (device, torch.cuda.current_stream(device).cuda_stream)


def _flags(adjoint: bool = False) -> int:
    f = 0
    if _opt().sort_rays:
        f |= _lib.FLAG_SORT_RAYS
    if adjoint and _opt().corrected_h:
        f |= _lib.FLAG_CORRECTED_H
    if adjoint and _opt().direct_atomics:
        f |= _lib.FLAG_DIRECT_ATOMICS
    if adjoint and _opt().adjoint_window == "box":
        f |= _lib.FLAG_STATIC_WINDOW
    if adjoint and _opt().adjoint_window == "ring":
        f |= _lib.FLAG_RING_WINDOW
    if adjoint and _opt().adjoint_window == "ring_sparse":       # A-B: the ring kernel's sparse-only instantiation, forced
        f |= _lib.FLAG_RING_WINDOW | _lib.FLAG_RING_SPARSE
    if adjoint and _opt().adjoint_window == "ring_direct":       # A-B: ... its direct sparse-only instantiation, forced
        f |= _lib.FLAG_RING_WINDOW | _lib.FLAG_RING_SPARSE | _lib.FLAG_RING_DIRECT
    if adjoint and _opt().adjoint_window == "ring_general":      # A-B: device-side choice between box and the GENERAL ring kernel
        f |= _lib.FLAG_RING_GENERAL
    if _opt().chord_key:
        f |= _lib.FLAG_CHORD_KEY
    return f


def _workspace(n: int, flags: int, device: torch.device, nvox: int = 0) -> torch.Tensor:
    need = int(_lib.load().drrt_workspace_bytes_grid(n, nvox, flags))
    key = _wkey(device)
    ws = _workspaces.get(key)
    if ws is None or ws.numel() < need:
        ws = torch.empty(max(need, 1 << 20), dtype=torch.uint8, device=device)
        _workspaces[key] = ws
        _pair_tokens.pop(key, None)
    if not (flags & _lib.FLAG_PAIR_GRID):
        _pair_tokens.pop(key, None)             # this call may overwrite the region a pair copy lived in
    return ws


# What the pair copy in a device's workspace was built from: (rif tensor, key).  Holding the tensor keeps its
# storage alive, so equal (data_ptr, version counter) means "same contents"; n and the sort bit fix where in
# the workspace the copy lives.
_pair_tokens: Dict[tuple, tuple] = {}


def _march_workspace(rif_: torch.Tensor, res, n: int, h: float, ds: float, flags: int, device: torch.device,
                     paired: bool = False, adjoint: bool = False):
    """Workspace + final flags of a grid march call: decides on DRRT_FLAG_PAIR_GRID (options.pair_grid).
    Forward calls always rebuild the copy.  An adjoint the caller explicitly pairs with its forward
    (`paired`: it passed the forward's visit order) adds DRRT_FLAG_PAIR_REUSE when the workspace still holds the
    copy built from this very tensor (same storage, same version counter, same layout) and no other call has
    used the workspace since.  With "auto" an adjoint never builds the copy itself (it gains ~2 %, less than the
    copy costs): it uses it only when it can reuse the forward's."""
    q = _opt().pair_grid
    auto = q == "auto"
    if auto:
        # the copy moves 12 B per voxel; the gathers it halves only bound the march when the GPU is full of waves
        ok = float(ds) > 0.0 and float(h) > 0.0               # invalid steps are the library's to report
        q = ok and n >= _PAIR_AUTO_MIN_RAYS and \
            n * max(int(r) for r in res) * (float(h) / float(ds)) >= 8.0 * rif_.numel()
    if not q or n == 0:
        return flags, _workspace(n, flags, device)
    pflags = flags | _lib.FLAG_PAIR_GRID
    key = (rif_.data_ptr(), rif_._version, rif_.numel(), n, flags & _lib.FLAG_SORT_RAYS)
    if auto and adjoint:
        tok = _pair_tokens.get(_wkey(device))
        need = int(_lib.load().drrt_workspace_bytes_grid(n, rif_.numel(), pflags))
        ws = _workspaces.get(_wkey(device))
        if not (paired and tok is not None and tok[1] == key and ws is not None and ws.numel() >= need):
            return flags, _workspace(n, flags, device)
    ws = _workspace(n, pflags, device, rif_.numel())         # may reallocate -> drops the token
    tok = _pair_tokens.get(_wkey(device))
    if paired and tok is not None and tok[1] == key:
        pflags |= _lib.FLAG_PAIR_REUSE
    _pair_tokens[_wkey(device)] = (rif_, key)
    return pflags, ws


_PAIR_AUTO_MIN_RAYS = 384 * 1024     # about 6 resident waves per SIMD on 256 CUs


def _dev(t: torch.Tensor) -> torch.device:
    if not t.is_cuda:
        raise RuntimeError("TracerC expects tensors on the cuda (ROCm) device; use TracerS for host tensors")
    return t.device


def _f32(t: torch.Tensor, device: torch.device) -> torch.Tensor:
    return t.detach().to(device=device, dtype=torch.float32).contiguous()


def _is_half(*ts: torch.Tensor) -> bool:
    """fp16 ray-state mode (BASELINE config 5): every ray tensor of the call is float16."""
    return all(t.dtype == torch.float16 for t in ts)


def _is_q16(*ts: torch.Tensor) -> bool:
    """16-bit ray state "q16" (include/drrt_hip.h): every position / direction tensor of the call is int16 codes."""
    return all(t.dtype == torch.int16 for t in ts)


def encode_rays16(res: Sequence[int], h: float, pos: Optional[torch.Tensor] = None, vel: Optional[torch.Tensor] = None):
    """fp32 (n,3) positions / directions -> q16 codes (int16 tensors; position codes are unsigned 16-bit values stored
    in int16 storage).  Rounded on the device exactly as the kernels round their outputs (drrt_q16_encode)."""
    ref = pos if pos is not None else vel
    dev = _dev(ref)
    with torch.cuda.device(dev):
        p_ = None if pos is None else _rays(pos, dev)
        v_ = None if vel is None else _rays(vel, dev)
        n = (p_ if p_ is not None else v_).shape[0]
        pq = None if p_ is None else torch.empty(n, 3, dtype=torch.int16, device=dev)
        vq = None if v_ is None else torch.empty(n, 3, dtype=torch.int16, device=dev)
        _lib.check(_lib.load().drrt_q16_encode(_res3(res), float(h), n, _p(p_), _p(v_), _p(pq), _p(vq), _stream(dev)))
    return tuple(t for t in (pq, vq) if t is not None) if (pos is not None and vel is not None) else (pq if pq is not None else vq)


def decode_rays16(res: Sequence[int], h: float, pos_q: Optional[torch.Tensor] = None, vel_q: Optional[torch.Tensor] = None):
    """q16 codes -> fp32 (exact widening, drrt_q16_decode)."""
    ref = pos_q if pos_q is not None else vel_q
    dev = _dev(ref)
    with torch.cuda.device(dev):
        n = ref.shape[0]
        pq = None if pos_q is None else pos_q.detach().contiguous()
        vq = None if vel_q is None else vel_q.detach().contiguous()
        p_ = None if pq is None else torch.empty(n, 3, dtype=torch.float32, device=dev)
        v_ = None if vq is None else torch.empty(n, 3, dtype=torch.float32, device=dev)
        _lib.check(_lib.load().drrt_q16_decode(_res3(res), float(h), n, _p(pq), _p(vq), _p(p_), _p(v_), _stream(dev)))
    return tuple(t for t in (p_, v_) if t is not None) if (pos_q is not None and vel_q is not None) else (p_ if p_ is not None else v_)


def _rays(t: torch.Tensor, device: torch.device, n: Optional[int] = None, half: bool = False, q16: bool = False) -> torch.Tensor:
    if q16 != (t.dtype == torch.int16) or not (q16 or t.dtype.is_floating_point):
        # integer tensors are codes, not numbers: converting them to fp32 would march code 16384 as 16384.0
        raise RuntimeError(
            f"{t.dtype} ray tensor where this call takes {'int16 codes' if q16 else 'floating-point values'}: codes of the "
            "16-bit ray state (encode_rays16) go to trace / backtrace only, as int16 positions with int16 or floating-point "
            "directions; decode_rays16 turns them into fp32 for every other call")
    if q16:
        t = t.detach().to(device=device).contiguous()
    else:
        t = t.detach().to(device=device, dtype=torch.float16).contiguous() if half else _f32(t, device)
    if t.dim() != 2 or t.shape[1] != 3 or (n is not None and t.shape[0] != n):
        raise RuntimeError(f"expected a ({'N' if n is None else n},3) ray tensor, got {tuple(t.shape)}")
    return t


def _res3(res: Sequence[int]):
    r = [int(v) for v in res]
    if len(r) != 3:
        raise RuntimeError("res must have 3 entries")
    return (C.c_int * 3)(*r)


def _publish(**last) -> None:
    """The one place that sets the module attributes last_stats / last_order / last_steps / last_bundle_counters: what the
    call just made left behind, for callers that use the public methods.  The internal path (`_grid_call`) hands order and
    steps to its own caller as well, which is what tracer.py and dist.py use: a module attribute is shared by all threads."""
    globals().update(last)


def _new_stats(device: torch.device) -> torch.Tensor:
    st = torch.empty(3, dtype=torch.int64, device=device)
    _publish(last_stats=st)
    return st


def read_stats(stats: Optional[torch.Tensor] = None) -> Dict[str, int]:
    """Synchronising read of a stats block -> dict(ray_steps, n_failed, iters)."""
    s = (last_stats if stats is None else stats).cpu()
    return dict(ray_steps=int(s[0]), n_failed=int(s[1]), iters=int(s[2]) & 0xFFFFFFFF)


def _bump_order_gen(device: torch.device) -> None:
    """The call about to be made rewrites the order / state region of this (device, stream)'s workspace."""
    k = _wkey(device)
    _order_gen[k] = _order_gen.get(k, 0) + 1


def _ws_view(ptr, nbytes: int, ws: torch.Tensor) -> Optional[torch.Tensor]:
    """The `nbytes` at device address `ptr` as a uint8 view of the workspace `ws`; None when they do not lie inside it."""
    off = int(ptr) - ws.data_ptr() if ptr else -1
    return ws[off:off + nbytes] if 0 <= off and off + nbytes <= ws.numel() else None


def _last_view(fn, n: int, device: torch.device) -> Optional[torch.Tensor]:
    """What drrt_last_order / drrt_last_steps (`fn`) points at, if it is n words of this (device, stream)'s workspace: an
    int32 view stamped with the workspace's generation (`drrt_gen`, _valid_order)."""
    cnt = C.c_size_t(0)
    ptr = fn(C.byref(cnt))
    key = _wkey(device)
    v = _ws_view(ptr, 4 * n, _workspaces[key]) if cnt.value == n else None
    if v is None:
        return None
    v = v.view(torch.int32)
    v.drrt_gen = (key, _order_gen.get(key, 0))
    return v


def _capture_order(n: int, device: torch.device) -> Optional[torch.Tensor]:
    """The permutation (and, riding on it, the per-ray iteration counts) the library just left in the workspace: views, no
    copies -- see `last_order`."""
    order = _last_view(_lib.load().drrt_last_order, n, device) if _opt().sort_rays and n >= 2 else None
    if order is not None:
        # the forward march's per-ray iteration counts ride along ON the order tensor (attribute `drrt_steps`), so every
        # holder of the order hands both to the paired adjoint: its rays then start on the forward march's clock (step
        # hint, include/drrt_hip.h)
        steps = _last_view(_lib.load().drrt_last_steps, n, device)
        if steps is not None:
            order.drrt_steps = steps
    return order


def keep_steps(steps: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    """A private copy of `last_steps` that stays valid whatever is called next; None for a stale or missing view."""
    steps = _valid_order(steps)
    return None if steps is None else steps.clone()


def keep_order(order: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    """A private copy of a visit order (with its iteration counts) that stays valid whatever is called next; None for a
    stale or missing order.  For holders that keep the order across other tracer calls (autograd ctx)."""
    order = _valid_order(order)
    if order is None or getattr(order, "drrt_gen", None) is None:
        return order
    kept = order.clone()
    steps = getattr(order, "drrt_steps", None)
    if steps is not None:
        kept.drrt_steps = steps.clone()
    return kept


def _valid_order(order: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    """`order` unless it is a workspace view whose region has been rewritten since it was handed out."""
    if order is None:
        return None
    gen = getattr(order, "drrt_gen", None)
    if gen is not None and _order_gen.get(gen[0], 0) != gen[1]:
        return None
    return order


last_bundle_counters: Optional[torch.Tensor] = None


def _capture_counters(ws: torch.Tensor) -> None:
    """The bundle classification of the adjoint call just made (drrt_last_bundle_counters, include/drrt_hip.h): four int32
    copied out of its workspace (device-to-device, async) -> `last_bundle_counters`, or None when the call did not classify."""
    v = _ws_view(_lib.load().drrt_last_bundle_counters(), 32, ws)
    _publish(last_bundle_counters=None if v is None else v.view(torch.int32).clone())


def read_bundle_counters() -> Optional[Dict[str, int]]:
    """Synchronising read of `last_bundle_counters` -> which adjoint kernel the last backtrace* call chose, and why.
    The rule is the library's own (`drrt_ring_threshold_pct()`, `drrt_ring_long_threshold_permille()`: its compile-time
    thresholds, so variant builds report what they ran): the ring-window kernel when a fifth of the bundles' START cells do
    not fit the box window or when 7.5 % of the bundles left the forward march 12 or more cells of travel apart (24 iterations at ds = h / 2); its sparse-only
    instantiation unless the call pinned the general one (counter [5])."""
    if last_bundle_counters is None:
        return None
    c = [int(v) for v in last_bundle_counters.cpu()]
    share = c[0] / c[1] if c[1] else 0.0
    pct = int(_lib.load().drrt_ring_threshold_pct())
    ext = int(_lib.load().drrt_ring_long_threshold_permille())
    long_ = bool(c[6] and c[6] * 1000 >= c[1] * ext)
    ring = bool(c[0] and c[0] * 100 >= c[1] * pct) or long_
    sparse = ring and c[5] == 0
    dpct = int(_lib.load().drrt_ring_direct_threshold_pct())
    direct = sparse and c[3] != 0 and c[4] * 100 < c[3] * dpct
    return dict(bundles_not_fitting=c[0], bundles=c[1], lanes_outside=c[2], lanes=c[3], not_fitting_share=share,
                start_pair_share=(c[4] / c[3] if c[3] else 0.0),
                bundles_long=c[6], long_bundle_share=(c[6] / c[1] if c[1] else 0.0), long_threshold_permille=ext,
                ring_threshold_pct=pct,
                direct_threshold_pct=dpct,
                kernel=("ring_direct" if direct else "ring_sparse" if sparse else "ring") if ring else "box")


# A progress block nothing has been reduced into (k_chunk_progress_init): mins at the largest key, maxs at the smallest
_EMPTY_PROGRESS = ([0x7FFFFFFF] * 3 + [-0x80000000] * 3) * 2 + [0] + [0x7FFFFFFF] * 3 + [-0x80000000] * 3 + [0]


def decode_chunk_progress(progress: torch.Tensor) -> Dict[str, object]:
    """Synchronising read of a chunk's progress block (drrt_backtrace_chunk_f32) -> dict(active, pos_min, pos_max, vel_min,
    vel_max, sample_min, sample_max): the bounding boxes of where the still-marching rays stand and head, and of the
    samples the chunk contributed at (lists of 3 floats; None when there is no such ray / sample)."""
    k = progress.cpu().to(torch.int64)
    n_active = int(k[12]) & 0xFFFFFFFF
    bits = torch.where(k >= 0, k, k ^ 0x7FFFFFFF).to(torch.int32)
    f = bits.view(torch.float32).tolist()
    out = dict(active=n_active, pos_min=None, pos_max=None, vel_min=None, vel_max=None, sample_min=None, sample_max=None)
    if n_active:
        out.update(pos_min=f[0:3], pos_max=f[3:6], vel_min=f[6:9], vel_max=f[9:12])
    if int(k[13]) != 0x7FFFFFFF:
        out.update(sample_min=f[13:16], sample_max=f[16:19])
    return out


def _hint(order: Optional[torch.Tensor], n: int) -> bool:
    """Arm the library's order (and step) hint for the next march call; -> whether an order was handed over."""
    if order is not None and order.numel() == n and order.dtype == torch.int32 and order.is_cuda:
        _lib.load().drrt_set_order_hint(C.c_void_p(order.data_ptr()), n)
        steps = getattr(order, "drrt_steps", None)
        if steps is not None and steps.numel() == n and steps.dtype == torch.int32 and steps.device == order.device:
            _lib.load().drrt_set_step_hint(C.c_void_p(steps.data_ptr()), n)
        return True
    return False


def _clear_hint() -> None:
    """The library consumes a hint at the entry of the next march call; this covers the paths on which that call
    is never reached (an exception while marshalling arguments)."""
    _lib.load().drrt_set_order_hint(None, 0)
    _lib.load().drrt_set_step_hint(None, 0)


@contextlib.contextmanager
def _paired_adjoint(rif_, res, n: int, h, ds, device, order, replay: bool = False, flags: int = 0):
    """The call sequence of an adjoint that may be paired with its forward march through `order` (the forward's visit
    order): validate the order, workspace + final flags, a fresh stats block, order / step hint armed -> yields
    (flags, workspace, stats, order) for the library call -> hint cleared.  The order region of the workspace counts as
    rewritten when the call sorts for itself (no hint taken), and always for the adjoints that `replay` their forward:
    their second-pass flags go where the forward left its iteration counts, and they march with the forward's flags."""
    order = _valid_order(order)
    fl = _flags(adjoint=not replay) | flags
    (fl, ws), st = _march_workspace(rif_, res, n, h, ds, fl, device, paired=order is not None, adjoint=True), _new_stats(device)
    try:
        if not _hint(order, n) or replay:
            _bump_order_gen(device)
        yield fl, ws, st, order
    finally:
        _clear_hint()


@contextlib.contextmanager
def _forward_march(rif_, res, n: int, h, ds, device, flags: int = 0):
    """The call sequence of a forward grid march, the twin of `_paired_adjoint`: workspace + final flags, a fresh stats
    block, the order / state region of the workspace counted as rewritten -> yields (flags, workspace, stats, None) for
    the library call.  What the call leaves behind is `_grid_call`'s to collect."""
    (fl, ws), st = _march_workspace(rif_, res, n, h, ds, _flags() | flags, device), _new_stats(device)
    _bump_order_gen(device)
    yield fl, ws, st, None


# "failed to exit all rays" (src/tracer.cpp:90) without a host sync per call: the stats block is copied to pinned
# host memory asynchronously behind the kernels, and looked at when the copy has landed -- at the next tracer call,
# at flush_warnings(), or at interpreter exit.  The message can therefore appear one call late; it is never lost.
_pending_warn: list = []      # (event, pinned host tensor)
_pinned_pool: list = []


def _capturing() -> bool:
    """True while the current stream is being captured into a HIP graph: event queries, pinned allocations and host
    copies are not capturable, so the failed-ray bookkeeping stands still during a capture."""
    try:
        return torch.cuda.is_current_stream_capturing()
    except Exception:
        return False


def _drain_warnings(block: bool = False) -> None:
    if _capturing():
        return
    while _pending_warn and (block or _pending_warn[0][0].query()):
        ev, host = _pending_warn.pop(0)
        if block:
            ev.synchronize()
        if int(host[1]) > 0:
            print("failed to exit all rays")            # src/tracer.cpp:90
        _pinned_pool.append(host)


def flush_warnings() -> None:
    """Wait for the outstanding marches and print any pending "failed to exit all rays" message."""
    _drain_warnings(block=True)


def _at_exit() -> None:
    try:
        if _pending_warn:
            _drain_warnings(block=True)
    except Exception:              # the HIP runtime may already be gone at interpreter teardown
        pass


import atexit as _atexit   # noqa: E402
_atexit.register(_at_exit)


def _warn_failed(stats: torch.Tensor) -> None:
    _drain_warnings()
    if not _opt().check_failed or _capturing():      # a captured march reports through its stats block only
        return
    host = _pinned_pool.pop() if _pinned_pool else torch.empty(3, dtype=torch.int64, pin_memory=True)
    host.copy_(stats, non_blocking=True)
    ev = torch.cuda.Event()
    ev.record(torch.cuda.current_stream(stats.device))
    _pending_warn.append((ev, host))
    if len(_pending_warn) > 64:                          # bounded backlog
        _drain_warnings(block=True)


def _cable_profiles(rif, field, dev: torch.device) -> list:
    """The flat fp32 profile(s) of a cable entry on `dev`: [rif], or [rif, field] for the entries that integrate a second
    radial profile, which must have rif's number of samples."""
    profs = [_f32(rif, dev).reshape(-1)]
    if field is not None:
        profs.append(_f32(field, dev).reshape(-1))
        if profs[1].numel() != profs[0].numel():
            raise RuntimeError(f"the second profile must have the {profs[0].numel()} samples of rif, got {profs[1].numel()}")
    return profs


def _cable_call(name: str, rif, radius, length, ds, rays, make_outputs, warn: bool = False, field=None) -> tuple:
    """One call of a cable entry point (they share their shape: profile, radius, length, n, the (n,3) ray tensors `rays`, ds,
    the outputs, the usual tail) -> the outputs, made by ``make_outputs(profile, first ray tensor)``.  `field`: the second
    radial profile of the entries that take one, right after the first."""
    dev = _dev(rif)
    with torch.cuda.device(dev):
        profs, first = _cable_profiles(rif, field, dev), _rays(rays[0], dev)
        rif_ = profs[0]
        n = first.shape[0]
        rays_ = [first] + [_rays(t, dev, n) for t in rays[1:]]
        out = make_outputs(rif_, first)
        ws, st = _workspace(n, 0, dev), _new_stats(dev)
        _lib.check(getattr(_lib.load(), name)(
            *map(_p, profs), rif_.numel(), float(radius), float(length), n, *map(_p, rays_), float(ds), *map(_p, out),
            _p(st), _p(ws), ws.numel(), 0, _stream(dev)))
        if warn:
            _warn_failed(st)
    return out


def _backtrace_cable_integral(op: str, rif, field, radius, length, pos, xt, vt, rec_steps, dx, dv, dint, ds, grads, rays):
    """One call of drrt_backtrace_cable_<op>_f32, the adjoint of a cable march with an integral (they share their shape: the
    profile(s), radius, length, n, pos, xt, vt, rec_steps, the three optional seeds, ds, one gradient per profile, dpos,
    dvel, the usual tail) -> ([grad | None per profile], dpos | None, dvel | None).  `grads`: per profile gradient (wanted,
    the tensor it is added to or None, that argument's name); with any such tensor the call runs under DRRT_FLAG_NO_ZERO,
    which covers every gradient, so a wanted one without a tensor is added to fresh zeros."""
    who = f"backtrace_cable_{op}"
    dev = _dev(rif)
    with torch.cuda.device(dev):
        profs, pos_ = _cable_profiles(rif, field, dev), _rays(pos, dev)
        rif_ = profs[0]
        n = pos_.shape[0]
        xt_, vt_ = _rays(xt, dev, n), _rays(vt, dev, n)
        rec_ = rec_steps.detach().to(device=dev).contiguous()
        if rec_.dtype != torch.int32 or rec_.numel() != n:
            raise RuntimeError(f"rec_steps must be {n} int32 record iterations of the forward call (trace_cable_{op}'s)")
        dx_, dv_ = (None if t is None else _rays(t, dev, n) for t in (dx, dv))
        dint_ = None if dint is None else _f32(dint, dev).reshape(-1)
        if dint_ is not None and dint_.numel() != n:
            raise RuntimeError(f"expected {n} per-ray values, got {dint_.numel()}")
        no_zero = any(want and into is not None for want, into, _ in grads)
        out = []
        for want, into, arg in grads:
            if want and into is not None:
                if into.dtype != torch.float32 or not into.is_contiguous() or into.numel() != rif_.numel() or into.device != dev:
                    raise RuntimeError(f"{who}: `{arg}` must be a contiguous fp32 tensor of the profile's size on its device")
                out.append(into.detach().view(-1))
            elif want:
                out.append(torch.zeros_like(rif_) if no_zero else torch.empty_like(rif_))
            else:
                out.append(None)
        # never a null pointer (n = 0): null dpos / dvel means "not asked for"
        dpos, dvel = (pos_.new_empty((max(n, 1), 3)), pos_.new_empty((max(n, 1), 3))) if rays else (None, None)
        ws, st = _workspace(n, 0, dev), _new_stats(dev)
        _lib.check(getattr(_lib.load(), f"drrt_{who}_f32")(
            *map(_p, profs), rif_.numel(), float(radius), float(length), n, _p(pos_), _p(xt_), _p(vt_), _p(rec_), _p(dx_),
            _p(dv_), _p(dint_), float(ds), *map(_p, out), _p(dpos), _p(dvel), _p(st), _p(ws), ws.numel(),
            _lib.FLAG_NO_ZERO if no_zero else 0, _stream(dev)))
        _warn_failed(st)
    return (out, dpos[:n], dvel[:n]) if rays else (out, None, None)


def _ray_format(pos: torch.Tensor, vel: torch.Tensor, seeds: tuple = ()):
    """The ray-state format of a trace / backtrace call, from the dtypes of its position and direction tensors (and, for
    the adjoint, of its `seeds`) -> (entry suffix, extra flag, how `_rays` converts each of (pos, vel, *seeds)).  All
    float16: the IEEE-half variant (half in, fp32 march, half out).  int16 positions AND directions (codes from
    ``encode_rays16``): the 16-bit ray state "q16", whose adjoint takes IEEE-half seeds.  int16 positions with
    floating-point directions: q16 positions only, directions and seeds fp32.  Anything else: fp32."""
    half, q16 = _is_half(pos, vel, *seeds), _is_q16(pos, vel)
    qpos = (not q16) and pos.dtype == torch.int16
    if q16 and seeds and not _is_half(*seeds):
        raise RuntimeError("q16 exit rays (int16) go with float16 seeds dx, dv")
    if not (half or q16 or qpos):
        return "_f32", 0, None
    how = [dict(half=half, q16=q16 or qpos), dict(half=half, q16=q16)] + [dict(half=half or q16)] * len(seeds)
    return "_q16io" if q16 or qpos else "_f16io", _lib.FLAG_Q16_POS_ONLY if qpos else 0, how


def _grid_inputs(rif, sdf, rays, dev: torch.device, how=None, planes: int = 1):
    """The inputs of a grid entry on `dev` -> (flat fp32 grid, flat fp32 SDF or None, the (n,3) ray tensors, n).  The
    first ray tensor fixes n; `how`: per ray tensor, the format `_rays` converts it to (`_ray_format`; None: all fp32);
    `planes`: the second grid is that many component planes of the first one's size (a vector field: 3)."""
    rif_ = _f32(rif, dev).reshape(-1)
    sdf_ = None if sdf is None else _f32(sdf, dev).reshape(-1)
    if sdf_ is not None and sdf_.numel() != planes * rif_.numel():
        raise RuntimeError("Resolution doesn't match data")      # src/volume.cpp:37
    if how is None:
        first = _rays(rays[0], dev)
        return rif_, sdf_, [first] + [_rays(t, dev, first.shape[0]) for t in rays[1:]], first.shape[0]
    first = _rays(rays[0], dev, **how[0])
    return rif_, sdf_, [first] + [_rays(t, dev, first.shape[0], **kw) for t, kw in zip(rays[1:], how[1:])], first.shape[0]


def _more_grid(grid, rif_, dev: torch.device) -> torch.Tensor:
    """A further grid of a grid entry on `dev`: flat fp32, of the first grid's size."""
    g = _f32(grid, dev).reshape(-1)
    if g.numel() != rif_.numel():
        raise RuntimeError("Resolution doesn't match data")      # src/volume.cpp:37
    return g


def _grid_call(name: str, rif, res, rays, h, ds, make_outputs, adjoint: bool, sdf=None, how=None, fwd_steps=None,
               order=None, replay: bool = False, flags: int = 0, steps: bool = True, warn: bool = False,
               counters: bool = False, per_ray=(), more_grids=(), planes: int = 1, scalars=()) -> tuple:
    """One call of a grid entry point (they share their shape: grid, [sdf], nvox, res, n, the inputs, h, ds, the outputs,
    the usual tail) -> (outputs, order, steps): the outputs, made by ``make_outputs(flat grid, ray tensors)``, and what
    a forward march left behind -- its visit order and per-ray iteration counts, the workspace views that are also
    published as `last_order` / `last_steps` (None, None for an adjoint).
    The inputs are the (n,3) tensors `rays` (converted as `_grid_inputs` does) and, for the one entry that takes them,
    `fwd_steps`: int32[n] behind the fourth ray tensor; `per_ray`: optional fp32[n] inputs behind the ray tensors (None is
    passed as a null pointer).  `adjoint`: a forward march, or an adjoint that may be paired
    with one through `order`; `replay`: an adjoint that marches its forward again (`_paired_adjoint`).  `steps`: the
    forward leaves iteration counts.  `warn`: failed rays are reported.  `counters`: the adjoint classifies its bundles
    (`last_bundle_counters`).  `more_grids`: further fp32 grids of the first one's size, passed behind `sdf`.  `planes`:
    `sdf` is that many component planes of the first grid's size.  `scalars`: further int arguments of the entry, passed
    behind ds."""
    dev = _dev(rif)
    with torch.cuda.device(dev):
        rif_, sdf_, rays_, n = _grid_inputs(rif, sdf, rays, dev, how, planes)
        more_ = [_more_grid(g, rif_, dev) for g in more_grids]
        if fwd_steps is not None:
            steps_ = fwd_steps.detach().to(device=dev).contiguous()
            if steps_.dtype != torch.int32 or steps_.numel() != n:
                raise RuntimeError(f"steps must be {n} int32 iteration counts of the forward call (drrt.last_steps)")
            rays_.insert(4, steps_)
        out = make_outputs(rif_, rays_)
        for t in per_ray:
            t = None if t is None else _f32(t, dev).reshape(-1)
            if t is not None and t.numel() != n:
                raise RuntimeError(f"expected {n} per-ray values, got {t.numel()}")
            rays_.append(t)
        grids = [_p(rif_)] if sdf_ is None else [_p(rif_), _p(sdf_)]
        grids += [_p(g) for g in more_]
        march = _paired_adjoint(rif_, res, n, h, ds, dev, order, replay, flags) if adjoint else \
            _forward_march(rif_, res, n, h, ds, dev, flags)
        with march as (fl, ws, st, _):
            _lib.check(getattr(_lib.load(), name)(
                *grids, rif_.numel(), _res3(res), n, *map(_p, rays_), float(h), float(ds), *map(int, scalars), *map(_p, out),
                _p(st), _p(ws), ws.numel(), fl, _stream(dev)))
            if counters:
                _capture_counters(ws)
        left_order = left_steps = None
        if not adjoint:
            left_order = _capture_order(n, dev)
            if steps:
                left_steps = _last_view(_lib.load().drrt_last_steps, n, dev)
                _publish(last_order=left_order, last_steps=left_steps)
            else:
                _publish(last_order=left_order)
        if warn:
            _warn_failed(st)
    return out, left_order, left_steps


def _like_rays(rif_, rays_) -> tuple:
    """Outputs of the shape and dtype of the call's first two ray tensors: (xt, vt), or (dpos, dvel)."""
    return torch.empty_like(rays_[0]), torch.empty_like(rays_[1])


def _like_grid(rif_, rays_) -> tuple:
    return (torch.empty_like(rif_),)


def _backtrace_integral(op: str, rif, more, res, pos, vel, xt, vt, steps, fwd_out, dx, dv, seeds, wanted, rays: bool, h, ds,
                        order, planes: int = 1, series=(), scalars=()) -> tuple:
    """What ``backtrace_opl`` / ``backtrace_field`` / ``backtrace_emission`` / ``backtrace_vector`` share: one call of drrt_backtrace_<op>_f32 ->
    (the grid gradients in the order of `wanted`, dpos, dvel), None for what is not asked for.  `more`: the operator's
    further grids; `fwd_out`: (name, tensor) of the forward outputs the adjoint needs besides xt, vt and steps; `seeds`:
    the per-ray seeds behind dx, dv (None: zeros); `wanted`: per grid gradient (asked for, accumulator or None, the name of
    the accumulator's argument).  An accumulator means DRRT_FLAG_NO_ZERO, which covers every grid of the call: those asked
    for without one are zeroed here.  `planes`: the operator's first further grid, and the gradient behind dL/drif, are that
    many component planes of the grid's size (a vector field: 3).  `series`: (seed or None, its shape with None for the ray
    count) of the seeds on outputs that are a series per ray, passed behind `seeds`; `scalars`: further int arguments of
    the entry, passed behind ds."""
    if not (rays or any(want for want, _, _ in wanted)):
        switches = [name.replace("into", "grid") for _, _, name in wanted] + ["rays"]
        raise RuntimeError(f"backtrace_{op}: nothing to compute ({' = '.join(switches)} = False)")
    dev = _dev(rif)
    with torch.cuda.device(dev):
        rif_, first_, (pos_, vel_, xt_, vt_), n = _grid_inputs(rif, more[0] if more else None, [pos, vel, xt, vt], dev,
                                                               planes=planes)
        more_ = ([first_] if more else []) + [_more_grid(g, rif_, dev) for g in more[1:]]
        steps_ = steps.detach().to(device=dev).contiguous()
        if steps_.dtype != torch.int32 or steps_.numel() != n:
            raise RuntimeError(f"steps must be {n} int32 iteration counts of the forward call (trace_{op}'s)")
        dx_, dv_ = (None if t is None else _rays(t, dev, n) for t in (dx, dv))
        per_ray = [None if t is None else _f32(t, dev).reshape(-1) for t in (*(t for _, t in fwd_out), *seeds)]
        for (name, _), t in zip(fwd_out, per_ray):
            if t is None:
                raise RuntimeError(f"backtrace_{op}: `{name}` is the forward call's {name} (trace_{op}'s)")
        for t in per_ray:
            if t is not None and t.numel() != n:
                raise RuntimeError(f"expected {n} per-ray values, got {t.numel()}")
        series_ = []
        for t, shape in series:
            t = None if t is None else _f32(t, dev)
            want = tuple(n if d is None else d for d in shape)
            if t is not None and tuple(t.shape) != want:
                raise RuntimeError(f"backtrace_{op}: expected a seed of shape {want}, got {tuple(t.shape)}")
            series_.append(t)
        no_zero = any(want and acc is not None for want, acc, _ in wanted)
        grads = []
        for k, (want, acc, name) in enumerate(wanted):
            size = rif_.numel() * (planes if k == 1 else 1)
            if not want:
                grads.append(None)
            elif acc is not None:
                if acc.dtype != torch.float32 or not acc.is_contiguous() or acc.numel() != size or acc.device != dev:
                    what = "the grid's size" if size == rif_.numel() else f"{planes} planes of the grid's size"
                    raise RuntimeError(f"backtrace_{op}: `{name}` must be a contiguous fp32 tensor of {what} on its device")
                grads.append(acc.detach().view(-1))
            else:
                grads.append(rif_.new_zeros(size) if no_zero else rif_.new_empty(size))
        dpos, dvel = (torch.empty_like(pos_), torch.empty_like(vel_)) if rays else (None, None)
        with _paired_adjoint(rif_, res, n, h, ds, dev, order, flags=_lib.FLAG_NO_ZERO if no_zero else 0) as (fl, ws, st, _):
            _lib.check(getattr(_lib.load(), f"drrt_backtrace_{op}_f32")(
                _p(rif_), *map(_p, more_), rif_.numel(), _res3(res), n, _p(pos_), _p(vel_), _p(xt_), _p(vt_), _p(steps_),
                *map(_p, per_ray[:len(fwd_out)]), _p(dx_), _p(dv_), *map(_p, per_ray[len(fwd_out):]), *map(_p, series_),
                float(h), float(ds), *map(int, scalars), *map(_p, grads), _p(dpos), _p(dvel), _p(st), _p(ws), ws.numel(), fl, _stream(dev)))
        _warn_failed(st)
    return (*grads, dpos, dvel)


def path_max_steps(res, h, ds) -> int:
    """The forward march's iteration bound, (int)(4 h max(res) / ds) in fp32 as the library forms it: what
    ``trace_path``'s default `samples` is sized by."""
    f = lambda a: torch.tensor(float(a), dtype=torch.float32)      # noqa: E731
    return int(f(4.0) * f(h) * f(max(int(r) for r in res)) / f(ds))


class TracerC:
    """GPU tracer without autodiff -- mirror of ``drrt.TracerC`` (``src/drrt.cpp:47-58``).  The forward grid marches
    come twice: ``_trace*`` -> (outputs, order, steps) as `_grid_call` returns them, for callers that hand the order to a
    paired adjoint (tracer.py, dist.py), and the public method, which returns the outputs."""

    # ---- forward ------------------------------------------------------------------------
    def _trace(self, rif, res, pos, vel, h, ds):
        _dev(rif)
        suffix, flag, how = _ray_format(pos, vel)
        return _grid_call("drrt_trace" + suffix, rif, res, [pos, vel], h, ds, _like_rays, adjoint=False, how=how,
                          flags=flag, warn=True)

    def trace(self, rif, res, pos, vel, h, ds) -> Tuple[torch.Tensor, torch.Tensor]:
        """Tracer::trace, src/tracer.cpp:35-100.  float16 pos AND vel select the IEEE-half ray-state variant
        (drrt_trace_f16io: half in, fp32 march, half out); int16 pos AND vel (codes from ``encode_rays16``) select the
        16-bit ray state "q16" (drrt_trace_q16io), which keeps sub-voxel positions -- see include/drrt_hip.h."""
        return self._trace(rif, res, pos, vel, h, ds)[0]

    def _trace_pln(self, rif, res, pos, vel, pln_o, pln_d, h, ds):
        return _grid_call("drrt_trace_pln_f32", rif, res, [pos, vel, pln_o, pln_d], h, ds,
                          lambda rif_, r: _like_rays(rif_, r) + (torch.empty(r[0].shape[0], dtype=torch.uint8, device=r[0].device),),
                          adjoint=False, warn=True)

    def trace_pln(self, rif, res, pos, vel, pln_o, pln_d, h, ds):
        """Tracer::trace_plane, src/tracer.cpp:102-172 -> (xt, vt, failmask uint8)."""
        return self._trace_pln(rif, res, pos, vel, pln_o, pln_d, h, ds)[0]

    def _trace_target(self, rif, res, pos, vel, target, h, ds):
        return _grid_call("drrt_trace_target_f32", rif, res, [pos, vel, target], h, ds,
                          lambda rif_, r: _like_rays(rif_, r) + (r[0].new_empty(r[0].shape[0]),),
                          adjoint=False, steps=False, warn=True)

    def trace_target(self, rif, res, pos, vel, target, h, ds):
        """Tracer::trace_target, src/tracer.cpp:174-242 -> (xt, vt, dist2)."""
        return self._trace_target(rif, res, pos, vel, target, h, ds)[0]

    def _trace_sdf(self, rif, sdf, res, pos, vel, h, ds):
        return _grid_call("drrt_trace_sdf_f32", rif, res, [pos, vel], h, ds, _like_rays, adjoint=False, sdf=sdf,
                          steps=False, warn=False)

    def trace_sdf(self, rif, sdf, res, pos, vel, h, ds):
        """Tracer::trace_sdf, src/tracer.cpp:244-310."""
        return self._trace_sdf(rif, sdf, res, pos, vel, h, ds)[0]

    def trace_cable(self, rif, radius, length, pos, vel, target, ds):
        """Tracer::trace_cable, src/tracer.cpp:312-382 -> (xt, vt, dist2)."""
        return _cable_call("drrt_trace_cable_f32", rif, radius, length, ds, (pos, vel, target),
                           lambda rif_, r: (torch.empty_like(r), torch.empty_like(r), r.new_empty(r.shape[0])), warn=True)

    def _trace_opl(self, rif, res, pos, vel, h, ds):
        return _grid_call("drrt_trace_opl_f32", rif, res, [pos, vel], h, ds,
                          lambda rif_, r: _like_rays(rif_, r) + (r[0].new_empty(r[0].shape[0]),
                                                                 torch.empty(r[0].shape[0], dtype=torch.int32, device=r[0].device)),
                          adjoint=False, steps=False, warn=True)

    def trace_opl(self, rif, res, pos, vel, h, ds):
        """``trace`` with the optical path length of every ray (drrt_trace_opl_f32, include/drrt_hip.h; not in the
        reference) -> (xt, vt, opl, steps): xt, vt and the per-ray iteration counts `steps` (int32[n], a tensor of the
        caller's, not a workspace view) are ``trace``'s bit for bit; ``opl = sum ds n_k^2`` over the samples the march takes
        inside the box (|v| = n, so this is the integral of n along the path).  fp32 rays only."""
        return self._trace_opl(rif, res, pos, vel, h, ds)[0]

    def _trace_field(self, rif, field, res, pos, vel, h, ds):
        return _grid_call("drrt_trace_field_f32", rif, res, [pos, vel], h, ds,
                          lambda rif_, r: _like_rays(rif_, r) + (r[0].new_empty(r[0].shape[0]),
                                                                 torch.empty(r[0].shape[0], dtype=torch.int32, device=r[0].device)),
                          adjoint=False, sdf=field, steps=False, warn=True)

    def trace_field(self, rif, field, res, pos, vel, h, ds):
        """``trace`` with the line integral of a second field along every bent ray (drrt_trace_field_f32,
        include/drrt_hip.h; not in the reference) -> (xt, vt, tau, steps).  `field`: an fp32 grid of `rif`'s shape and axis
        convention (an absorption or emission coefficient, a group index).  xt, vt and the per-ray iteration counts `steps`
        (int32[n], a tensor of the caller's, not a workspace view) are ``trace``'s bit for bit; ``tau = sum ds n_k a_k`` over
        the samples the march takes inside the box, a_k the field at the cell and weights of n_k (|v| = n, so this is the
        integral of the field along the path; with field = rif it is ``trace_opl``'s opl bit for bit).  fp32 rays only."""
        return self._trace_field(rif, field, res, pos, vel, h, ds)[0]

    def _trace_emission(self, rif, emission, absorption, res, pos, vel, h, ds):
        def outputs(rif_, r):
            n = r[0].shape[0]
            return _like_rays(rif_, r) + (r[0].new_empty(n), r[0].new_empty(n),
                                          torch.empty(n, dtype=torch.int32, device=r[0].device))
        return _grid_call("drrt_trace_emission_f32", rif, res, [pos, vel], h, ds, outputs, adjoint=False, sdf=emission,
                          more_grids=(absorption,), steps=False, warn=True)

    def trace_emission(self, rif, emission, absorption, res, pos, vel, h, ds):
        """``trace`` with the radiative-transfer line integral of an emitting, self-absorbing medium along every bent ray
        (drrt_trace_emission_f32, include/drrt_hip.h; not in the reference) -> (xt, vt, rad, tau, steps).  `emission`,
        `absorption`: fp32 grids of `rif`'s shape and axis convention.  xt, vt and the per-ray iteration counts `steps`
        (int32[n], a tensor of the caller's, not a workspace view) are ``trace``'s bit for bit.  Over the samples the march
        takes inside the box, with ``w_k = ds n_k``: ``rad = sum exp_neg(tau_k) w_k e_k`` (emit, then absorb: the
        transmittance is that in front of the sample) and ``tau = sum w_k a_k``, which is ``trace_field(rif, absorption)``'s
        tau bit for bit; with absorption = 0, rad is ``trace_field(rif, emission)``'s tau bit for bit.  |v| = n, so these
        are the integrals along the path.  Negative absorption (gain) is legal; the exponent is clamped to +-87.  fp32 rays
        only."""
        return self._trace_emission(rif, emission, absorption, res, pos, vel, h, ds)[0]

    def _trace_vector(self, rif, vfield, res, pos, vel, h, ds):
        return _grid_call("drrt_trace_vector_f32", rif, res, [pos, vel], h, ds,
                          lambda rif_, r: _like_rays(rif_, r) + (r[0].new_empty(r[0].shape[0]),
                                                                 torch.empty(r[0].shape[0], dtype=torch.int32, device=r[0].device)),
                          adjoint=False, sdf=vfield, steps=False, warn=True, planes=3)

    def trace_vector(self, rif, vfield, res, pos, vel, h, ds):
        """``trace`` with the line integral of a vector field projected on the ray's own direction, along every bent ray
        (drrt_trace_vector_f32, include/drrt_hip.h; not in the reference) -> (xt, vt, circ, steps).  `vfield`: fp32 of shape
        ``(3,) + rif.shape``, three component planes of `rif`'s shape and axis convention; plane c pairs with component c of
        pos / vel (x, y, z).  xt, vt and the per-ray iteration counts `steps` (int32[n], a tensor of the caller's, not a
        workspace view) are ``trace``'s bit for bit; ``circ = sum ds u_k . v_{k+1}`` over the samples the march takes inside
        the box, u_k the field at the cell and weights of n_k and v_{k+1} the velocity behind the step, which carries the
        ray from x_k to x_{k+1} (so this is ``sum u(x_k) . (x_{k+1} - x_k)``, the integral of u . dl along the path; for a
        uniform u it telescopes to ``u . (xt - x_e)``).  fp32 rays only."""
        return self._trace_vector(rif, vfield, res, pos, vel, h, ds)[0]

    def _trace_path(self, rif, res, pos, vel, h, ds, stride, samples=None, velocities=False):
        """The path march, and with `velocities` the phase march: the same call with vpath behind path."""
        stride = int(stride)
        if samples is None:
            samples = -(-max(path_max_steps(res, h, ds), 0) // max(stride, 1)) + 1
        samples = int(samples)

        def outputs(rif_, r):
            n, dev = r[0].shape[0], r[0].device
            series = tuple(r[0].new_empty((max(samples, 0), n, 3)) for _ in range(2 if velocities else 1))
            return _like_rays(rif_, r) + series + (torch.empty(n, dtype=torch.int32, device=dev),
                                                   torch.empty(n, dtype=torch.int32, device=dev))
        return _grid_call("drrt_trace_phase_f32" if velocities else "drrt_trace_path_f32", rif, res, [pos, vel], h, ds,
                          outputs, adjoint=False, steps=False, warn=True, scalars=(stride, samples))

    def trace_path(self, rif, res, pos, vel, h, ds, stride, samples=None):
        """``trace`` with the path of every ray (drrt_trace_path_f32, include/drrt_hip.h; not in the reference) ->
        (xt, vt, path, count, steps).  xt, vt and the per-ray iteration counts `steps` (int32[n]) are ``trace``'s bit for
        bit.  `path` is fp32 ``(samples, n, 3)``, sample-major: ``path[j]`` is every ray at sample j, ``path[:, i]`` ray i's
        polyline: the marching positions in front of iterations 0, stride, 2 stride, ... (``path[0] = pos``), `count`
        (int32[n]) of them, then xt repeated.  A ray that never samples inside the box has xt = pos, so its padding is pos;
        `count` says where to cut.  ``samples * stride < steps`` truncates a ray's series: no padding, no error.
        ``samples=None`` is ``ceil(max_steps / stride) + 1``, the smallest that always ends on xt.  fp32 rays only."""
        return self._trace_path(rif, res, pos, vel, h, ds, stride, samples)[0]

    def trace_phase(self, rif, res, pos, vel, h, ds, stride, samples=None):
        """``trace_path`` with the marching velocities beside the positions (drrt_trace_phase_f32, include/drrt_hip.h; not
        in the reference) -> (xt, vt, path, vpath, count, steps).  xt, vt, path, count and steps are ``trace_path``'s bit for
        bit.  `vpath` is fp32 ``(samples, n, 3)`` in `path`'s layout: ``vpath[j]`` is the velocity the march carries in front
        of iteration j stride (``vpath[0] = vel``; for j > 0 the velocity that carried the ray into ``path[j]``), `count` of
        them, then vt repeated.  ``(path[j], vpath[j])`` is the march's state at sample j, and ``|vpath[j]|`` the refractive
        index the ray saw there.  `samples`: as for ``trace_path``.  fp32 rays only."""
        return self._trace_path(rif, res, pos, vel, h, ds, stride, samples, velocities=True)[0]

    # ---- adjoint ------------------------------------------------------------------------
    def _backtrace_path(self, op, series, rif, res, pos, vel, xt, vt, steps, dx, dv, h, ds, stride, grid, rays, into, order,
                        samples):
        """What ``backtrace_path`` (`op` "path", `series` (dpath,)) and ``backtrace_phase`` ("phase", (dpath, dvpath)) share:
        `samples` is read off the first seed of `series` that is given."""
        if samples is None:
            samples = next((int(s.shape[0]) for s in series if s is not None), 1)
        shape = (int(samples), None, 3)
        return _backtrace_integral(op, rif, (), res, pos, vel, xt, vt, steps, (), dx, dv, (), ((grid, into, "into"),),
                                   rays, h, ds, order, series=tuple((s, shape) for s in series),
                                   scalars=(int(stride), int(samples)))

    def backtrace_phase(self, rif, res, pos, vel, xt, vt, steps, dx, dv, dpath, dvpath, h, ds, stride, grid: bool = True,
                        rays: bool = True, into: Optional[torch.Tensor] = None, order: Optional[torch.Tensor] = None,
                        samples: Optional[int] = None):
        """Adjoint of ``trace_phase`` (drrt_backtrace_phase_f32, include/drrt_hip.h) -> (grad | None, dpos | None, dvel |
        None): ``backtrace_path`` with one more seed, `dvpath` ((samples, n, 3), None: zeros), from ONE reverse march.  With
        `dvpath` None the results are ``backtrace_path``'s bit for bit.  `samples` is read off whichever of `dpath` and
        `dvpath` is given; it is needed only when both are None (then any value gives the same result, and the default is
        1).  Seeds on padded `vpath` entries are seeds on vt, added to dv in ascending j.  Everything else: as for
        ``backtrace_path``."""
        return self._backtrace_path("phase", (dpath, dvpath), rif, res, pos, vel, xt, vt, steps, dx, dv, h, ds, stride, grid,
                                    rays, into, order, samples)

    def backtrace_path(self, rif, res, pos, vel, xt, vt, steps, dx, dv, dpath, h, ds, stride, grid: bool = True,
                       rays: bool = True, into: Optional[torch.Tensor] = None, order: Optional[torch.Tensor] = None,
                       samples: Optional[int] = None):
        """Adjoint of ``trace_path`` (drrt_backtrace_path_f32, include/drrt_hip.h) -> (grad | None, dpos | None, dvel |
        None): flat dL/dn (fp32[nvox]), dL/dpos and dL/dvel ((n,3) fp32) from ONE reverse march, the derivative of the
        discrete forward with `steps` and `count` held fixed.  `pos`, `vel` are the forward call's inputs, `xt`, `vt`,
        `steps` its outputs, `stride` its stride; `dx`, `dv` ((n,3)) and `dpath` ((samples, n, 3)) the seeds on (xt, vt,
        path), each optional (None: zeros).  `samples` is read off `dpath`; it is needed only when `dpath` is None (then any
        value gives the same result, and the default is 1).  Seeds on padded entries are seeds on xt, added to dx in
        ascending j.  `grid` / `rays` / `into` / `order`: as for ``backtrace_opl``.  Honours ``options.corrected_h`` (with it
        the grid gradient is the exact discrete derivative; the ray gradients do not depend on it).  Rays that failed the
        forward get zeros and contribute nothing."""
        return self._backtrace_path("path", (dpath,), rif, res, pos, vel, xt, vt, steps, dx, dv, h, ds, stride, grid, rays,
                                    into, order, samples)

    def backtrace_vector(self, rif, vfield, res, pos, vel, xt, vt, steps, dx, dv, dcirc, h, ds, grid: bool = True,
                         vfield_grid: bool = True, rays: bool = True, into: Optional[torch.Tensor] = None,
                         vfield_into: Optional[torch.Tensor] = None, order: Optional[torch.Tensor] = None):
        """Adjoint of ``trace_vector`` (drrt_backtrace_vector_f32, include/drrt_hip.h) -> (grad | None, grad_vfield | None,
        dpos | None, dvel | None): flat dL/drif (fp32[nvox]) and dL/dvfield (fp32[3 nvox], the three planes as `vfield`),
        dL/dpos and dL/dvel ((n,3) fp32) from ONE reverse march.  `pos`, `vel` are the forward call's inputs, `xt`, `vt`,
        `steps` its outputs; `dx`, `dv` ((n,3)) and `dcirc` (n values) the seeds on (xt, vt, circ), each optional (None:
        zeros).  `grid` / `vfield_grid` / `rays`: which outputs are computed (at least one); `into` (flat fp32[nvox]) /
        `vfield_into` (flat fp32[3 nvox]): a tensor that gradient is ADDED to (DRRT_FLAG_NO_ZERO, which covers both: where
        only one of the two is given, the other is zeroed here) and that is returned in its place.  Honours
        ``options.corrected_h`` (with it dL/drif is the exact discrete derivative; dL/dvfield and the ray gradients are that
        either way).  Rays that failed the forward get zeros and contribute nothing.  `order`: the forward's visit order."""
        return _backtrace_integral("vector", rif, (vfield,), res, pos, vel, xt, vt, steps, (), dx, dv, (dcirc,),
                                   ((grid, into, "into"), (vfield_grid, vfield_into, "vfield_into")), rays, h, ds, order,
                                   planes=3)

    def backtrace_emission(self, rif, emission, absorption, res, pos, vel, xt, vt, steps, tau, dx, dv, drad, dtau, h, ds,
                           grid: bool = True, emission_grid: bool = True, absorption_grid: bool = True, rays: bool = True,
                           into: Optional[torch.Tensor] = None, emission_into: Optional[torch.Tensor] = None,
                           absorption_into: Optional[torch.Tensor] = None, order: Optional[torch.Tensor] = None):
        """Adjoint of ``trace_emission`` (drrt_backtrace_emission_f32, include/drrt_hip.h) -> (grad | None,
        grad_emission | None, grad_absorption | None, dpos | None, dvel | None): flat dL/drif, dL/demission and
        dL/dabsorption (fp32[nvox] each), dL/dpos and dL/dvel ((n,3) fp32) from ONE reverse march.  `pos`, `vel` are the
        forward call's inputs, `xt`, `vt`, `steps`, `tau` its outputs; `dx`, `dv` ((n,3)), `drad` and `dtau` (n values each)
        the seeds on (xt, vt, rad, tau), each optional (None: zeros).  `grid` / `emission_grid` / `absorption_grid` / `rays`:
        which outputs are computed (at least one); `into` / `emission_into` / `absorption_into`: a flat fp32[nvox] tensor
        that grid's gradient is ADDED to (DRRT_FLAG_NO_ZERO, which covers all three grids: those asked for without an
        accumulator are zeroed here) and that is returned in its place.  The reverse march recovers every transmittance from
        `tau` by subtraction, so dL/demission, dL/dabsorption and the ray gradients are the derivative of the discrete
        forward to fp32 rounding; dL/drif is the same derivative with ``options.corrected_h``.  Rays that failed the forward
        get zeros and contribute nothing.  `order`: the forward's visit order."""
        return _backtrace_integral("emission", rif, (emission, absorption), res, pos, vel, xt, vt, steps, (("tau", tau),), dx, dv,
                                   (drad, dtau), ((grid, into, "into"), (emission_grid, emission_into, "emission_into"),
                                                  (absorption_grid, absorption_into, "absorption_into")), rays, h, ds, order)

    def backtrace_field(self, rif, field, res, pos, vel, xt, vt, steps, dx, dv, dtau, h, ds, grid: bool = True,
                        field_grid: bool = True, rays: bool = True, into: Optional[torch.Tensor] = None,
                        field_into: Optional[torch.Tensor] = None, order: Optional[torch.Tensor] = None):
        """Adjoint of ``trace_field`` (drrt_backtrace_field_f32, include/drrt_hip.h) -> (grad | None, grad_field | None,
        dpos | None, dvel | None): flat dL/drif and dL/dfield (fp32[nvox] each), dL/dpos and dL/dvel ((n,3) fp32) from ONE
        reverse march.  `pos`, `vel` are the forward call's inputs, `xt`, `vt`, `steps` its outputs; `dx`, `dv` ((n,3)) and
        `dtau` (n values) the seeds on (xt, vt, tau), each optional (None: zeros).  `grid` / `field_grid` / `rays`: which
        outputs are computed (at least one); `into` / `field_into`: a flat fp32[nvox] tensor that grid's gradient is ADDED to
        (DRRT_FLAG_NO_ZERO, which covers both grids: where only one of the two is given, the other grid is zeroed here) and
        that is returned in its place.  Honours ``options.corrected_h`` (with it dL/drif is the exact discrete derivative;
        dL/dfield and the ray gradients are that either way).  Rays that failed the forward get zeros and contribute
        nothing.  `order`: the forward's visit order."""
        return _backtrace_integral("field", rif, (field,), res, pos, vel, xt, vt, steps, (), dx, dv, (dtau,),
                                   ((grid, into, "into"), (field_grid, field_into, "field_into")), rays, h, ds, order)

    def backtrace_opl(self, rif, res, pos, vel, xt, vt, steps, dx, dv, dopl, h, ds, grid: bool = True, rays: bool = True,
                      into: Optional[torch.Tensor] = None, order: Optional[torch.Tensor] = None):
        """Adjoint of ``trace_opl`` (drrt_backtrace_opl_f32, include/drrt_hip.h) -> (grad | None, dpos | None, dvel | None):
        flat dL/dn (fp32[nvox]), dL/dpos and dL/dvel ((n,3) fp32) from ONE reverse march.  `pos`, `vel` are the forward
        call's inputs, `xt`, `vt`, `steps` its outputs; `dx`, `dv` ((n,3)) and `dopl` (n values) the seeds on (xt, vt, opl),
        each optional (None: zeros).  `grid` / `rays`: which outputs are computed (at least one); `into`: a flat fp32[nvox]
        tensor the grid gradient is ADDED to (DRRT_FLAG_NO_ZERO) and that is returned as grad.  Honours
        ``options.corrected_h`` (with it the grid gradient is the exact discrete derivative; the ray gradients do not depend
        on it).  Rays that failed the forward get zeros and contribute nothing.  `order`: the forward's visit order."""
        return _backtrace_integral("opl", rif, (), res, pos, vel, xt, vt, steps, (), dx, dv, (dopl,), ((grid, into, "into"),),
                                   rays, h, ds, order)

    def backtrace(self, rif, res, xt, vt, dx, dv, h, ds, order: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Tracer::backtrace, src/tracer.cpp:384-440 -> flat dL/dn (fp32[nvox]).
        `order` (optional, not in the reference): visit order of the paired forward call.
        float16 xt, vt, dx, dv select the fp16 ray-state variant (fp32 recurrences and accumulation); q16 exit rays
        go with IEEE-half seeds (drrt_backtrace_q16io), q16 positions alone with fp32 directions and seeds."""
        _dev(rif)
        suffix, flag, how = _ray_format(xt, vt, (dx, dv))
        (grad,), _, _ = _grid_call("drrt_backtrace" + suffix, rif, res, [xt, vt, dx, dv], h, ds, _like_grid, adjoint=True,
                                   how=how, order=order, flags=flag, counters=True)
        return grad

    def backtrace_rays(self, rif, res, pos, vel, xt, vt, steps, dx, dv, h, ds,
                       order: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """Ray-state adjoint of ``trace`` (drrt_backtrace_rays_f32, include/drrt_hip.h) -> (dL/dpos, dL/dvel), (n,3) fp32.
        `pos`, `vel` are the forward call's inputs, `xt`, `vt` its outputs and `steps` its per-ray iteration counts
        (``keep_steps(last_steps)`` right after it); `dx`, `dv` the seeds on (xt, vt).  Rays that failed the forward get a
        zero gradient (and the "failed to exit all rays" message).  Not in the reference's C++ Tracer: its ADTracerC gets
        these through enoki autodiff (core/tracer.py:16-66).  fp32 rays only."""
        return _grid_call("drrt_backtrace_rays_f32", rif, res, [pos, vel, xt, vt, dx, dv], h, ds, _like_rays, adjoint=True,
                          fwd_steps=steps, order=order, warn=True)[0]

    def backtrace_chunked(self, rif, res, xt, vt, dx, dv, h, ds, order: Optional[torch.Tensor] = None, chunks: int = 4,
                          on_chunk=None) -> torch.Tensor:
        """Tracer::backtrace in `chunks` depth chunks (drrt_backtrace_chunk_f32, include/drrt_hip.h): the same gradient as
        ``backtrace`` (same per-ray contributions, another summation order), computed by `chunks` launches of
        max_steps / chunks iterations each.  After every chunk ``on_chunk(k, grad, progress)`` is called with the running
        gradient (flat fp32[nvox], still being accumulated into by the later chunks) and ``progress`` = a device tensor of
        20 int32 (decode with ``decode_chunk_progress``): the bounding box of the positions and velocities of the rays
        that are still marching -- what lies behind all of them, with none heading back, is final -- and the box of the
        samples this chunk contributed at.  Not in the reference;
        used by ``dist`` to reduce final slabs of dL/dn across ranks while the next chunk marches.  fp32 rays only."""
        dev = _dev(rif)
        with torch.cuda.device(dev):
            rif_, _, (xt_, vt_, dx_, dv_), n = _grid_inputs(rif, None, [xt, vt, dx, dv], dev)
            grad = torch.empty_like(rif_)
            lib = _lib.load()
            total = int(lib.drrt_backtrace_max_steps(_res3(res), float(h), float(ds)))
            if total < 0:
                raise RuntimeError("h and ds must be positive and finite")
            chunks = max(1, min(int(chunks), max(total, 1)))
            state = torch.empty(max(int(lib.drrt_backtrace_chunk_state_bytes(n)), 16), dtype=torch.uint8, device=dev)   # never a null pointer (n = 0)
            bounds = [total * k // chunks for k in range(chunks + 1)]
            with _paired_adjoint(rif_, res, n, h, ds, dev, order) as (fl, ws, st, order):     # armed for the first chunk
                if n == 1 and order is None and fl & _lib.FLAG_SORT_RAYS:
                    # one ray is not sorted, so the first chunk leaves no order behind (drrt_last_order() is null, or names
                    # an earlier call's): every chunk gets the trivial one, which a resumed chunk of a sorted march asks for
                    order = torch.zeros(1, dtype=torch.int32, device=dev)
                    _hint(order, n)
                for k in range(chunks):
                    if n == 0:
                        # no rays: the first call zeroes `grad` and the stats, nothing is launched and nothing writes a
                        # progress block -- every chunk reports the empty one (nothing marches, no samples)
                        progress = torch.tensor(_EMPTY_PROGRESS, dtype=torch.int32, device=dev)
                        if k > 0:
                            if on_chunk is not None:
                                on_chunk(k, grad, progress)
                            continue
                    else:
                        progress = torch.empty(20, dtype=torch.int32, device=dev)
                    if k > 0:                              # later chunks: the order the first chunk used
                        if not _hint(order, n) and fl & _lib.FLAG_SORT_RAYS:
                            lib.drrt_set_order_hint(lib.drrt_last_order(None), n)
                    _lib.check(lib.drrt_backtrace_chunk_f32(
                        _p(rif_), rif_.numel(), _res3(res), n, _p(xt_), _p(vt_), _p(dx_), _p(dv_), float(h), float(ds),
                        _p(grad), _p(st), _p(ws), ws.numel(), fl, _stream(dev), _p(state), state.numel(),
                        bounds[k], bounds[k + 1] - bounds[k], _p(progress)))
                    if on_chunk is not None:
                        on_chunk(k, grad, progress)
        return grad

    def backtrace_sdf(self, rif, sdf, res, xt, vt, dx, dv, h, ds, order: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Tracer::backtrace_sdf, src/tracer.cpp:443-509."""
        (grad,), _, _ = _grid_call("drrt_backtrace_sdf_f32", rif, res, [xt, vt, dx, dv], h, ds, _like_grid,
                                   adjoint=True, sdf=sdf, order=order, counters=True)
        return grad

    def backtrace_cable(self, rif, radius, length, xt, vt, dx, dv, ds) -> torch.Tensor:
        """Tracer::backtrace_cable, src/tracer.cpp:511-567 -> dL/d(profile) fp32[rres]."""
        return _cable_call("drrt_backtrace_cable_f32", rif, radius, length, ds, (xt, vt, dx, dv),
                           lambda rif_, r: (torch.empty_like(rif_),))[0]

    def backtrace_cable_rays(self, rif, radius, length, pos, vel, target, dx, dv, ds) -> Tuple[torch.Tensor, torch.Tensor]:
        """Ray-state adjoint of ``trace_cable`` (drrt_backtrace_cable_rays_f32, include/drrt_hip.h) -> (dL/dpos, dL/dvel),
        (n,3) fp32.  `pos`, `vel`, `target` are the forward call's inputs, `dx`, `dv` the seeds on its (xt, vt); the call
        replays the forward to find the iteration of the closest-approach record, so it takes neither (xt, vt) nor a step
        count.  A seed on dist2 does not enter.  Not in the reference's C++ Tracer: its ADCableTracerC gets these through
        enoki autodiff (core/tracer.py:237-291).  fp32 rays only."""
        return _cable_call("drrt_backtrace_cable_rays_f32", rif, radius, length, ds, (pos, vel, target, dx, dv),
                           lambda rif_, r: (torch.empty_like(r), torch.empty_like(r)))

    def trace_cable_opl(self, rif, radius, length, pos, vel, target, ds):
        """``trace_cable`` with the optical path length of every ray up to its record (drrt_trace_cable_opl_f32,
        include/drrt_hip.h; not in the reference) -> (xt, vt, dist2, opl, rec_steps): xt, vt and dist2 are ``trace_cable``'s
        bit for bit; ``opl = sum ds n_k^2`` over the iterations in front of the closest-approach record (the integral of n
        along the path -- the transit time -- when the rays enter with |v| = n; rays scaled otherwise get the same sum, not
        that integral); `rec_steps` (int32[n]) is the record's iteration, which ``backtrace_cable_opl`` takes.  fp32 rays
        only."""
        return _cable_call("drrt_trace_cable_opl_f32", rif, radius, length, ds, (pos, vel, target),
                           lambda rif_, r: (torch.empty_like(r), torch.empty_like(r), r.new_empty(r.shape[0]),
                                            r.new_empty(r.shape[0]),
                                            torch.empty(r.shape[0], dtype=torch.int32, device=r.device)), warn=True)

    def backtrace_cable_opl(self, rif, radius, length, pos, xt, vt, rec_steps, dx, dv, dopl, ds, profile: bool = True,
                            rays: bool = True, into: Optional[torch.Tensor] = None):
        """Adjoint of ``trace_cable_opl`` (drrt_backtrace_cable_opl_f32, include/drrt_hip.h) -> (grad | None, dpos | None,
        dvel | None): dL/d(profile) (fp32[rres]), dL/dpos and dL/dvel ((n,3) fp32) from ONE reverse march that replays
        nothing.  `pos` is the forward call's input, `xt`, `vt`, `rec_steps` its outputs; `dx`, `dv` ((n,3)) and `dopl` (n
        values) the seeds on (xt, vt, opl), each optional (None: zeros); a seed on dist2 does not enter and nothing flows to
        the target.  `profile` / `rays`: which outputs are computed (at least one); `into`: a flat fp32[rres] tensor the
        profile gradient is ADDED to (DRRT_FLAG_NO_ZERO) and that is returned as grad.  The record's iteration is held
        fixed.  A ray whose `rec_steps` exceeds the forward's step bound gets zero gradients and the "failed to exit all
        rays" message."""
        if not (profile or rays):
            raise RuntimeError("backtrace_cable_opl: nothing to compute (profile = rays = False)")
        (grad,), dpos, dvel = _backtrace_cable_integral("opl", rif, None, radius, length, pos, xt, vt, rec_steps, dx, dv, dopl,
                                                        ds, ((profile, into, "into"),), rays)
        return grad, dpos, dvel

    def trace_cable_field(self, rif, field, radius, length, pos, vel, target, ds):
        """``trace_cable`` with the line integral of a second radial profile `field` (rif's number of samples, same radius)
        along every ray up to its record (drrt_trace_cable_field_f32, include/drrt_hip.h; not in the reference) -> (xt, vt,
        dist2, tau, rec_steps): xt, vt and dist2 are ``trace_cable``'s bit for bit; ``tau = sum ds n_k a_k`` over the
        iterations in front of the closest-approach record, a_k the lerp of `field` in the cell of the march's own sample
        n_k (the integral of a along the path -- a group delay, an attenuation -- when the rays enter with |v| = n; rays
        scaled otherwise get the same sum, not that integral; with ``field = rif`` it is ``trace_cable_opl``'s opl bit for
        bit); `rec_steps` (int32[n]) is the record's iteration, which ``backtrace_cable_field`` takes.  fp32 rays only."""
        return _cable_call("drrt_trace_cable_field_f32", rif, radius, length, ds, (pos, vel, target),
                           lambda rif_, r: (torch.empty_like(r), torch.empty_like(r), r.new_empty(r.shape[0]),
                                            r.new_empty(r.shape[0]),
                                            torch.empty(r.shape[0], dtype=torch.int32, device=r.device)), warn=True,
                           field=field)

    def backtrace_cable_field(self, rif, field, radius, length, pos, xt, vt, rec_steps, dx, dv, dtau, ds,
                              want_rif: bool = True, want_field: bool = True, want_rays: bool = True,
                              into: Optional[torch.Tensor] = None, into_field: Optional[torch.Tensor] = None):
        """Adjoint of ``trace_cable_field`` (drrt_backtrace_cable_field_f32, include/drrt_hip.h) -> (grad | None,
        grad_field | None, dpos | None, dvel | None): dL/d(profile) and dL/d(field) (fp32[rres] each), dL/dpos and dL/dvel
        ((n,3) fp32) from ONE reverse march that replays nothing.  `pos` is the forward call's input, `xt`, `vt`,
        `rec_steps` its outputs; `dx`, `dv` ((n,3)) and `dtau` (n values) the seeds on (xt, vt, tau), each optional (None:
        zeros); a seed on dist2 does not enter and nothing flows to the target.  `want_rif` / `want_field` / `want_rays`:
        which outputs are computed (at least one).  `into` / `into_field`: flat fp32[rres] tensors the two gradients are
        ADDED to and that are returned; DRRT_FLAG_NO_ZERO covers both gradients, so with either given a requested gradient
        without one is added to fresh zeros.  The record's iteration is held fixed.  A ray whose `rec_steps` exceeds the
        forward's step bound gets zero gradients and the "failed to exit all rays" message."""
        if not (want_rif or want_field or want_rays):
            raise RuntimeError("backtrace_cable_field: nothing to compute (want_rif = want_field = want_rays = False)")
        (grad, grad_field), dpos, dvel = _backtrace_cable_integral(
            "field", rif, field, radius, length, pos, xt, vt, rec_steps, dx, dv, dtau, ds,
            ((want_rif, into, "into"), (want_field, into_field, "into_field")), want_rays)
        return grad, grad_field, dpos, dvel

    def backtrace_pln_rays(self, rif, res, pos, vel, pln_o, pln_d, dx, dv, h, ds,
                           order: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """Ray-state adjoint of ``trace_pln`` (drrt_backtrace_pln_rays_f32, include/drrt_hip.h) -> (dL/dpos, dL/dvel),
        (n,3) fp32.  `pos`, `vel`, `pln_o`, `pln_d` are the forward call's inputs, `dx`, `dv` the seeds on its (xt, vt); the
        call replays the forward (both of its passes) to find the iteration of each ray's record and which iterations
        were refracted, so it takes neither (xt, vt) nor a step count.  Rays that failed the forward get a zero gradient
        (and the "failed to exit all rays" message).  Not in the reference's C++ Tracer: it gets these through enoki
        autodiff (core/tracer.py:122-178).  fp32 rays only."""
        return _grid_call("drrt_backtrace_pln_rays_f32", rif, res, [pos, vel, pln_o, pln_d, dx, dv], h, ds, _like_rays,
                          adjoint=True, order=order, replay=True, warn=True)[0]

    def backtrace_sdf_rays(self, rif, sdf, res, pos, vel, dx, dv, h, ds,
                           order: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """Ray-state adjoint of ``trace_sdf`` (drrt_backtrace_sdf_rays_f32) -> (dL/dpos, dL/dvel), (n,3) fp32; as
        ``backtrace_pln_rays``, without the message: like ``trace_sdf`` it reports failed rays through its stats block
        only.  A ray that never crosses the surface keeps its input as the record and gets (dx, dv).
        The reference: enoki autodiff, core/tracer.py:181-234.  fp32 rays only."""
        return _grid_call("drrt_backtrace_sdf_rays_f32", rif, res, [pos, vel, dx, dv], h, ds, _like_rays,
                          adjoint=True, sdf=sdf, order=order, replay=True, warn=False)[0]

    def backtrace_target_rays(self, rif, res, pos, vel, target, dx, dv, h, ds, ddist2: Optional[torch.Tensor] = None,
                              order: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """Ray-state adjoint of ``trace_target`` (drrt_backtrace_target_rays_f32, include/drrt_hip.h) -> (dL/dpos, dL/dvel),
        (n,3) fp32.  `pos`, `vel`, `target` are the forward call's inputs, `dx`, `dv` the seeds on its (xt, vt) and `ddist2`
        (n values, optional) the seed on its dist2; the call replays the forward over the call's global iteration count to
        find the iteration of each ray's closest-approach record, so it takes neither (xt, vt) nor a step count.  A ray that
        ran out of steps keeps its record and its gradient (and draws the "failed to exit all rays" message).
        dL/dtarget = -2 ddist2 (xt - target) needs no call.  Not in the reference's C++ Tracer: it binds trace_target on its
        enoki autodiff tracer (src/drrt.cpp:34).  fp32 rays only."""
        return _grid_call("drrt_backtrace_target_rays_f32", rif, res, [pos, vel, target, dx, dv], h, ds, _like_rays,
                          adjoint=True, order=order, replay=True, warn=True, per_ray=(ddist2,))[0]

    # ---- print-only smoke methods of the reference (src/tracer.cpp:16-33) ------------------
    def test(self) -> torch.Tensor:
        """Tracer::tester: returns a zero 3-vector."""
        return torch.zeros(1, 3)

    def testscale(self, p) -> None:
        """Tracer::test_in: prints 1.1+0.5 and its floor2int (print-only in the reference)."""
        one = torch.full((1, 3), 1.1) + 0.5
        print(one)
        print(torch.floor(one).to(torch.int32))


class TracerS:
    """Host-tensor tracer -- mirror of ``drrt.TracerS`` (``src/drrt.cpp:38-45``): binds only
    ``trace``, ``trace_sdf``, ``trace_target``, ``backtrace``.  Inputs may live on
    the CPU; compute happens on ``cuda:0`` through ``TracerC`` and results return to the
    inputs' device.  No CPU compute path exists in this package."""

    def __init__(self, device: str = "cuda:0"):
        self._dev = torch.device(device)
        self._c = TracerC()

    def _staged(self, method, out_dev, *args):
        """``method(*args)`` of the TracerC with the tensors among `args` staged to the GPU and the results on `out_dev`."""
        out = method(*(t.to(self._dev) if isinstance(t, torch.Tensor) else t for t in args))
        return out.to(out_dev) if isinstance(out, torch.Tensor) else tuple(t.to(out_dev) for t in out)

    def trace(self, rif, res, pos, vel, h, ds):
        return self._staged(self._c.trace, pos.device, rif, res, pos, vel, h, ds)

    def trace_sdf(self, rif, sdf, res, pos, vel, h, ds):
        return self._staged(self._c.trace_sdf, pos.device, rif, sdf, res, pos, vel, h, ds)

    def trace_target(self, rif, res, pos, vel, target, h, ds):
        return self._staged(self._c.trace_target, pos.device, rif, res, pos, vel, target, h, ds)

    def backtrace(self, rif, res, xt, vt, dx, dv, h, ds):
        return self._staged(self._c.backtrace, rif.device, rif, res, xt, vt, dx, dv, h, ds)

    test = TracerC.test
    testscale = TracerC.testscale


class TracerD:
    """enoki-autodiff tracer of the reference (``src/drrt.cpp:28-36``): not provided -- the
    hand-written adjoint (``TracerC.backtrace*``) is the supported gradient path."""

    def __init__(self, *a, **k):
        raise NotImplementedError(
            "drrt.TracerD (enoki autodiff) is out of scope; use TracerC + tracer.BackTracerC")
