// drrt_stop_rays.hip -- gfx950 kernels of the ray-state adjoints of Tracer::trace_plane and Tracer::trace_sdf: dL/dpos and
// dL/dvel of the rays that entered such a call (drrt_backtrace_pln_rays_f32, drrt_backtrace_sdf_rays_f32; the reference gets
// them through enoki autodiff, core/tracer.py:122-234).  Per-ray arithmetic: stop_backtrace_ray_state of drrt_device.h, which
// tests/hostcheck runs on the host; shared pieces: drrt_march.h.
//
// One ray per lane: the replay of the forward, then the reverse march, all in registers -- (x, v, lambda, mu) and the taps of
// the current cell.  Nothing is written to the grid: no LDS window, no atomics.  A lane keeps the taps of a strictly interior
// cell while it stays in it; boundary cells are fetched with their clamps (fetch of drrt_device.h).
//
// Two passes, as the forward (k_trace_flat / k_trace + k_trace_again): the first replays every ray with per-ray termination,
// undoes the rays whose record is final, flags the others (`again` bytes in the workspace) and leaves the maximum of the
// per-ray iteration counts -- the reference's global loop count -- in stats->iters; the second, a near-empty launch behind it
// on the same stream, replays the flagged rays over exactly that many iterations and undoes them.
#include "drrt_march.h"

namespace drrt {

// block_stats with the sum and the maximum taken from different counts: ray_steps sums replay + reverse iterations, iters is
// the maximum of the first replay's iteration counts
__device__ __forceinline__ void stop_block_stats(drrt_stats* stats, unsigned steps, unsigned fwd, unsigned failed) {
  __shared__ unsigned s_sum[kBlock / kWave], s_max[kBlock / kWave], s_fail[kBlock / kWave];
  const unsigned ws = wave_sum_u32(steps), wm = wave_max_u32(fwd), wf = wave_sum_u32(failed);
  const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
  if (lane == 0) { s_sum[wid] = ws; s_max[wid] = wm; s_fail[wid] = wf; }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long sum = 0, fail = 0; unsigned mx = 0;
#pragma unroll
    for (int w = 0; w < kBlock / kWave; ++w) { sum += s_sum[w]; fail += s_fail[w]; mx = max(mx, s_max[w]); }
    if (sum)  atomicAdd(&stats->ray_steps, sum);
    if (fail) atomicAdd(&stats->n_failed, fail);
    if (mx)   atomicMax(&stats->iters, mx);
  }
}

template <int MODE, bool PAIR, bool FULL>
__device__ __forceinline__ StopGrad stop_ray(const StopRayGradArgs& a, const TapRows& R, size_t i, unsigned total) {
  const Vol& V = a.vol;
  const Ray3 p = ld3(a.pos, i), u = ld3(a.vel, i), gx = ld3(a.dx, i), gv = ld3(a.dv, i);
  const float p0[3] = {p.x, p.y, p.z}, v0[3] = {u.x, u.y, u.z};
  const float dx[3] = {gx.x, gx.y, gx.z}, dv[3] = {gv.x, gv.y, gv.z};
  float po[3] = {0.f, 0.f, 0.f}, pd[3] = {0.f, 0.f, 0.f};
  if (MODE == 1) {
    const Ray3 o = ld3(a.pln_o, i), d = ld3(a.pln_d, i);
    po[0] = o.x; po[1] = o.y; po[2] = o.z; pd[0] = d.x; pd[1] = d.y; pd[2] = d.z;
  }
  unsigned off = 0;          // byte offset (tap_offset) of the interior cell whose taps the lane holds
  bool held = false;
  f4 q0 = f4{0.f, 0.f, 0.f, 0.f}, q1 = q0;
  return stop_backtrace_ray_state<MODE, FULL>(V, a.sdf, a.ds, a.max_steps, total, p0, v0, po, pd, dx, dv,
    [&](const Cell& c) -> Taps {
      if (!c.interior) { held = false; return fetch(V.data, c); }
      const unsigned noff = tap_offset<PAIR>(c.base);
      if (!(held & (noff == off))) { gather_rows<PAIR>(R, noff, q0, q1); off = noff; held = true; }
      return taps_of<PAIR>(q0, q1);
    });
}

// first pass: every ray
template <int MODE, bool PAIR>
__global__ void __launch_bounds__(kBlock) k_backtrace_stop_rays(StopRayGradArgs a) {
  const size_t t = (size_t)xcd_block(blockIdx.x, gridDim.x, a.xcd_order ? kXcdRuns16 : kXcdOff) * kBlock + threadIdx.x;
  const TapRows R = tap_rows<PAIR>(a.vol);
  unsigned steps = 0, fwd = 0, failed = 0;
  size_t i;
  if (ray_index(a.perm, t, a.n, i)) {
    const StopGrad g = stop_ray<MODE, PAIR, false>(a, R, i, 0u);
    steps = g.steps; fwd = g.fwd; failed = g.failed ? 1u : 0u;
    a.again[i] = g.again ? 1 : 0;
    if (!g.again) {
      st3(a.dpos, i, g.dp[0], g.dp[1], g.dp[2]);
      st3(a.dvel, i, g.dv[0], g.dv[1], g.dv[2]);
    }
  }
  stop_block_stats(a.stats, steps, fwd, failed);
}

// second pass: the rays the first one flagged, over the global loop count it left in stats->iters (stream-ordered)
template <int MODE, bool PAIR>
__global__ void __launch_bounds__(kBlock) k_backtrace_stop_rays_again(StopRayGradArgs a) {
  const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= a.n || !a.again[i]) return;
  const TapRows R = tap_rows<PAIR>(a.vol);
  const StopGrad g = stop_ray<MODE, PAIR, true>(a, R, i, a.stats->iters);
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

}  // namespace drrt
