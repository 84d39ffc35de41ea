// drrt_ray_adjoints.hip -- gfx950 kernels of the ray-state adjoints of the grid marches: dL/dpos and dL/dvel of the rays that
// entered a call of
//   Tracer::trace          drrt_backtrace_rays_f32         backtrace_ray_state, from the forward's (xt, vt) and its per-ray
//                                                          iteration counts (the reference's ADTracerC: core/tracer.py:16-66)
//   Tracer::trace_plane    drrt_backtrace_pln_rays_f32     stop_backtrace_ray_state<1> and <2>, from the forward's inputs
//   Tracer::trace_sdf      drrt_backtrace_sdf_rays_f32     alone: the forward is replayed (core/tracer.py:122-234)
//   Tracer::trace_target   drrt_backtrace_target_rays_f32  target_backtrace_ray_state, replayed too, with a seed on dist2
//                                                          (src/drrt.cpp:34)
// The reference gets all of them through enoki autodiff.  Per-ray arithmetic: the routines named above (drrt_device.h: one
// seeded reverse run under all of them), which tests/hostcheck runs on the host; shared pieces: drrt_march.h.
//
// One ray per lane, everything in registers: the replay of the forward where there is one, then the reverse march --
// (x, v, lambda, mu) and the taps of the current cell.  Nothing is written to the grid -- no LDS window, no atomics but the
// statistics -- so, unlike the dL/dn adjoint, these marches are bound by their gathers and their arithmetic alone, like the
// forward march.  A lane keeps the taps of a strictly interior cell while it stays in it (HeldTaps: the forward's rule,
// k_trace_flat); boundary cells are fetched with their clamps (fetch of drrt_device.h).
//
// trace_plane / trace_sdf take two passes, as the forward (k_trace_flat / k_trace + k_trace_again): the first replays every
// ray with per-ray termination, undoes the rays whose record is final, flags the others (`again` bytes in the workspace) and
// leaves the maximum of the per-ray iteration counts -- the reference's global loop count -- in stats->iters; the second, a
// near-empty launch behind it on the same stream, replays the flagged rays over exactly that many iterations and undoes them.
//
// The record of trace_target depends on the call's GLOBAL loop count (an escaped ray flies on while any ray marches, and its
// record is updated on the way, src/tracer.cpp:225-227), so it takes two launches on the call's stream too: the first replays
// phase A of every ray and leaves only the maximum of the iteration counts in stats->iters; the second reads it, replays
// phases A and B and undoes them.  No per-ray state is kept between the two, so the call writes nothing to its workspace
// but what the sort and the pair copy put there.
#include "drrt_march.h"

namespace drrt {

// What the kernels share: the lane's ray and seeds, its march, the store of the gradients and the block's statistics.
// `march(i, r, taps)` -> LaneGrad runs the routine on ray i.
struct LaneRay { float p0[3], v0[3], dx[3], dv[3]; };
struct LaneGrad {
  float dp[3], dv[3];
  unsigned steps, iters, failed;     // the lane's shares of stats->ray_steps (sum), iters (maximum) and n_failed (sum)
  bool store;                        // false: (dpos, dvel) of this ray are left to a later launch
};
template <typename Grad>
__device__ __forceinline__ LaneGrad lane_grad(const Grad& g, unsigned steps, unsigned iters, bool store = true) {
  return LaneGrad{{g.dp[0], g.dp[1], g.dp[2]}, {g.dv[0], g.dv[1], g.dv[2]}, steps, iters, g.failed ? 1u : 0u, store};
}

template <typename Args>
__device__ __forceinline__ LaneRay lane_ray(const Args& a, size_t i) {
  const Ray3 p = ld3(a.pos, i), u = ld3(a.vel, i), gx = ld3(a.dx, i), gv = ld3(a.dv, i);
  return LaneRay{{p.x, p.y, p.z}, {u.x, u.y, u.z}, {gx.x, gx.y, gx.z}, {gv.x, gv.y, gv.z}};
}

template <bool PAIR, typename Args, typename March>
__device__ __forceinline__ void ray_adjoint_lanes(const Args& a, March&& march) {
  const Vol& V = a.vol;
  const size_t t = (size_t)xcd_block(blockIdx.x, gridDim.x, a.xcd_order ? kXcdRuns16 : kXcdOff) * kBlock + threadIdx.x;
  const TapRows R = tap_rows<PAIR>(V);
  unsigned steps = 0, iters = 0, failed = 0;
  size_t i;
  if (ray_index(a.perm, t, a.n, i)) {
    const LaneRay r = lane_ray(a, i);
    HeldTaps<PAIR> taps(V, R);
    const LaneGrad g = march(i, r, taps);
    steps = g.steps; iters = g.iters; failed = g.failed;
    if (g.store) {
      st3(a.dpos, i, g.dp[0], g.dp[1], g.dp[2]);
      st3(a.dvel, i, g.dv[0], g.dv[1], g.dv[2]);
    }
  }
  block_stats(a.stats, steps, iters, failed);
}

// ---- trace ---------------------------------------------------------------------------------------------------------------
template <bool PAIR>
__global__ void __launch_bounds__(kBlock) k_backtrace_rays(RayGradArgs a) {
  ray_adjoint_lanes<PAIR>(a, [&](size_t i, const LaneRay& r, HeldTaps<PAIR>& taps) {
    const Ray3 xe = ld3(a.xt, i), ve = ld3(a.vt, i);
    const float xt[3] = {xe.x, xe.y, xe.z}, vt[3] = {ve.x, ve.y, ve.z};
    const RayGrad g = backtrace_ray_state(a.vol, a.ds, a.max_steps, a.fsteps[i], r.p0, r.v0, xt, vt, r.dx, r.dv, taps);
    return lane_grad(g, g.steps, g.steps);
  });
}

void launch_backtrace_rays(const RayGradArgs& a, hipStream_t s) {
  const dim3 g(grid_for(a.n)), b(kBlock);
  if (a.vol.pair != nullptr) hipLaunchKernelGGL(k_backtrace_rays<true>, g, b, 0, s, a);
  else                       hipLaunchKernelGGL(k_backtrace_rays<false>, g, b, 0, s, a);
}

// ---- trace_plane (MODE 1), trace_sdf (MODE 2) ------------------------------------------------------------------------------
template <int MODE, bool FULL, typename TapFn>
__device__ __forceinline__ StopGrad stop_ray(const StopRayGradArgs& a, size_t i, const LaneRay& r, unsigned total, TapFn& taps) {
  float po[3] = {0.f, 0.f, 0.f}, pd[3] = {0.f, 0.f, 0.f};
  if (MODE == 1) {
    const Ray3 o = ld3(a.pln_o, i), d = ld3(a.pln_d, i);
    po[0] = o.x; po[1] = o.y; po[2] = o.z; pd[0] = d.x; pd[1] = d.y; pd[2] = d.z;
  }
  return stop_backtrace_ray_state<MODE, FULL>(a.vol, a.sdf, a.ds, a.max_steps, total, r.p0, r.v0, po, pd, r.dx, r.dv, taps);
}

// first pass: every ray; ray_steps sums replay + reverse iterations, iters is the maximum of the first replay's counts
template <int MODE, bool PAIR>
__global__ void __launch_bounds__(kBlock) k_backtrace_stop_rays(StopRayGradArgs a) {
  ray_adjoint_lanes<PAIR>(a, [&](size_t i, const LaneRay& r, HeldTaps<PAIR>& taps) {
    const StopGrad g = stop_ray<MODE, false>(a, i, r, 0u, taps);
    a.again[i] = g.again ? 1 : 0;
    return lane_grad(g, g.steps, g.fwd, !g.again);
  });
}

// second pass: the rays the first one flagged, over the global loop count it left in stats->iters (stream-ordered)
template <int MODE, bool PAIR>
__global__ void __launch_bounds__(kBlock) k_backtrace_stop_rays_again(StopRayGradArgs a) {
  const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= a.n || !a.again[i]) return;
  const TapRows R = tap_rows<PAIR>(a.vol);
  HeldTaps<PAIR> taps(a.vol, R);
  const StopGrad g = stop_ray<MODE, true>(a, i, lane_ray(a, i), a.stats->iters, taps);
  st3(a.dpos, i, g.dp[0], g.dp[1], g.dp[2]);
  st3(a.dvel, i, g.dv[0], g.dv[1], g.dv[2]);
  if (g.steps) atomicAdd(&a.stats->ray_steps, (unsigned long long)g.steps);
}

template <int MODE, bool PAIR>
static void launch_stop(const StopRayGradArgs& a, hipStream_t s) {
  const dim3 g(grid_for(a.n)), b(kBlock);
  hipLaunchKernelGGL((k_backtrace_stop_rays<MODE, PAIR>), g, b, 0, s, a);
  hipLaunchKernelGGL((k_backtrace_stop_rays_again<MODE, PAIR>), g, b, 0, s, a);
}

void launch_backtrace_stop_rays(int mode, const StopRayGradArgs& a, hipStream_t s) {
  const bool pair = a.vol.pair != nullptr;
  if (mode == 1) { if (pair) launch_stop<1, true>(a, s); else launch_stop<1, false>(a, s); }
  else           { if (pair) launch_stop<2, true>(a, s); else launch_stop<2, false>(a, s); }
}

// ---- trace_target --------------------------------------------------------------------------------------------------------
// first launch: phase A of every ray, for its iteration count alone (which does not depend on the target); nothing is stored
template <bool PAIR>
__global__ void __launch_bounds__(kBlock) k_target_rays_count(TargetRayGradArgs a) {
  ray_adjoint_lanes<PAIR>(a, [&](size_t, const LaneRay& r, HeldTaps<PAIR>& taps) {
    TargetReplay rp;
    target_replay_a(a.vol, a.ds, a.max_steps, r.p0, r.v0, r.p0, taps, rp);
    return LaneGrad{{}, {}, 0u, rp.done, 0u, false};
  });
}

// second launch: replay over the global loop count the first one left in stats->iters (stream-ordered), then the reverse march
template <bool PAIR>
__global__ void __launch_bounds__(kBlock) k_backtrace_target_rays(TargetRayGradArgs a) {
  const unsigned total = a.stats->iters;
  ray_adjoint_lanes<PAIR>(a, [&](size_t i, const LaneRay& r, HeldTaps<PAIR>& taps) {
    const Ray3 tg = ld3(a.target, i);
    const float tt[3] = {tg.x, tg.y, tg.z};
    const float dd2 = a.dd2 ? a.dd2[i] : 0.f;
    const TargetGrad g = target_backtrace_ray_state(a.vol, a.ds, a.max_steps, total, r.p0, r.v0, tt, r.dx, r.dv, dd2, taps);
    return lane_grad(g, g.steps, 0u);
  });
}

template <bool PAIR>
static void launch_target_rays(const TargetRayGradArgs& a, hipStream_t s) {
  const dim3 g(grid_for(a.n)), b(kBlock);
  hipLaunchKernelGGL((k_target_rays_count<PAIR>), g, b, 0, s, a);
  hipLaunchKernelGGL((k_backtrace_target_rays<PAIR>), g, b, 0, s, a);
}

void launch_backtrace_target_rays(const TargetRayGradArgs& a, hipStream_t s) {
  if (a.vol.pair != nullptr) launch_target_rays<true>(a, s); else launch_target_rays<false>(a, s);
}

}  // namespace drrt
