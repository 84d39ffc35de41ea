// drrt_target_rays.hip -- gfx950 kernels of the ray-state adjoint of Tracer::trace_target: dL/dpos and dL/dvel of the rays that
// entered such a call, from seeds on its closest-approach record (xt, vt) and on dist2 (drrt_backtrace_target_rays_f32; the
// reference gets them through enoki autodiff, src/drrt.cpp:34).  Per-ray arithmetic: target_backtrace_ray_state of
// drrt_device.h, which tests/hostcheck runs on the host; shared pieces: drrt_march.h.
//
// One ray per lane, everything in registers, as drrt_stop_rays.hip: the replay of the forward, then the reverse march --
// (x, v, lambda, mu) and the taps of the current cell.  Nothing is written to the grid: no LDS window, no atomics but the
// statistics.  A lane keeps the taps of a strictly interior cell while it stays in it; boundary cells are fetched with their
// clamps (fetch of drrt_device.h).
//
// The record of trace_target depends on the call's GLOBAL loop count (an escaped ray flies on while any ray marches, and its
// record is updated on the way, src/tracer.cpp:225-227), so there are two launches on the call's stream: the first replays
// phase A of every ray and leaves only the maximum of the iteration counts in stats->iters; the second reads it, replays
// phases A and B and undoes them.  No per-ray state is kept between the two, so the call writes nothing to its workspace
// but what the sort and the pair copy put there.
#include "drrt_march.h"

namespace drrt {

// the statistics of one block: sum of `steps` and of `failed`, maximum of `fwd`, one atomic each where non-zero
__device__ __forceinline__ void target_block_stats(drrt_stats* stats, unsigned steps, unsigned fwd, unsigned failed) {
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

// the taps of cell c for the lane: gathered through R, kept while the lane stays in a strictly interior cell
template <bool PAIR>
struct HeldTaps {
  const Vol& V;
  const TapRows& R;
  unsigned off = 0;          // byte offset (tap_offset) of the interior cell whose taps the lane holds
  bool held = false;
  f4 q0 = f4{0.f, 0.f, 0.f, 0.f}, q1 = f4{0.f, 0.f, 0.f, 0.f};
  __device__ __forceinline__ HeldTaps(const Vol& v, const TapRows& r) : V(v), R(r) {}
  __device__ __forceinline__ Taps operator()(const Cell& c) {
    if (!c.interior) { held = false; return fetch(V.data, c); }
    const unsigned noff = tap_offset<PAIR>(c.base);
    if (!(held & (noff == off))) { gather_rows<PAIR>(R, noff, q0, q1); off = noff; held = true; }
    return taps_of<PAIR>(q0, q1);
  }
};

// first pass: phase A of every ray, for its iteration count alone (which does not depend on the target)
template <bool PAIR>
__global__ void __launch_bounds__(kBlock) k_target_rays_count(TargetRayGradArgs a) {
  const size_t t = (size_t)xcd_block(blockIdx.x, gridDim.x, a.xcd_order ? kXcdRuns16 : kXcdOff) * kBlock + threadIdx.x;
  const TapRows R = tap_rows<PAIR>(a.vol);
  unsigned fwd = 0;
  size_t i;
  if (ray_index(a.perm, t, a.n, i)) {
    const Ray3 p = ld3(a.pos, i), u = ld3(a.vel, i);
    const float p0[3] = {p.x, p.y, p.z}, v0[3] = {u.x, u.y, u.z};
    HeldTaps<PAIR> taps(a.vol, R);
    TargetReplay r;
    target_replay_a(a.vol, a.ds, a.max_steps, p0, v0, p0, taps, r);
    fwd = r.done;
  }
  target_block_stats(a.stats, 0u, fwd, 0u);
}

// second pass: replay over the global loop count the first one left in stats->iters (stream-ordered), then the reverse march
template <bool PAIR>
__global__ void __launch_bounds__(kBlock) k_backtrace_target_rays(TargetRayGradArgs a) {
  const size_t t = (size_t)xcd_block(blockIdx.x, gridDim.x, a.xcd_order ? kXcdRuns16 : kXcdOff) * kBlock + threadIdx.x;
  const TapRows R = tap_rows<PAIR>(a.vol);
  const unsigned total = a.stats->iters;
  unsigned steps = 0, failed = 0;
  size_t i;
  if (ray_index(a.perm, t, a.n, i)) {
    const Ray3 p = ld3(a.pos, i), u = ld3(a.vel, i), tg = ld3(a.target, i), gx = ld3(a.dx, i), gv = ld3(a.dv, i);
    const float p0[3] = {p.x, p.y, p.z}, v0[3] = {u.x, u.y, u.z}, tt[3] = {tg.x, tg.y, tg.z};
    const float dx[3] = {gx.x, gx.y, gx.z}, dv[3] = {gv.x, gv.y, gv.z};
    const float dd2 = a.dd2 ? a.dd2[i] : 0.f;
    HeldTaps<PAIR> taps(a.vol, R);
    const TargetGrad g = target_backtrace_ray_state(a.vol, a.ds, a.max_steps, total, p0, v0, tt, dx, dv, dd2, taps);
    steps = g.steps; failed = g.failed ? 1u : 0u;
    st3(a.dpos, i, g.dp[0], g.dp[1], g.dp[2]);
    st3(a.dvel, i, g.dv[0], g.dv[1], g.dv[2]);
  }
  target_block_stats(a.stats, steps, 0u, failed);
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
