// drrt_opl.hip -- gfx950 kernels of the optical path length: drrt_trace_opl_f32 (trace, plus opl = sum ds n_k^2 over the
// samples the march takes anyway) and drrt_backtrace_opl_f32 (its adjoint: dL/dn, dL/dpos and dL/dvel from seeds on
// (xt, vt, opl) in ONE reverse march).  Not in the reference.  Per-ray arithmetic: trace_opl_ray / opl_backtrace_ray of
// drrt_device.h, which tests/hostcheck/opl_rays.hip runs on the host; shared pieces: drrt_march.h.
//
// One ray per lane, everything in registers, as drrt_adjoint_rays.hip: a lane keeps the taps of a strictly interior cell
// while it stays in it; boundary cells are fetched with their clamps (fetch of drrt_device.h).
//
// The adjoint scatters with one global fp32 atomic per tap, like k_backtrace_direct, with one refinement: a lane keeps the
// eight corner sums of its cell in registers while consecutive samples fall in the same cell, and flushes them when the
// cell changes and after its last iteration (with ds = h / 2 that roughly halves the atomics).  There is NO LDS window: the
// ring kernel's fixed-point window is scaled for backtrace's contributions and a per-step source term does not fit its
// overflow budget, so this kernel pays the memory-side atomic rate where many rays cross the same voxels.
// OplTaps and HeldCorners live in drrt_march.h: drrt_field.hip uses them too.
#include "drrt_march.h"

namespace drrt {

template <bool PAIR>
__global__ void __launch_bounds__(kBlock) k_trace_opl(OplTraceArgs a) {
  const Vol& V = a.vol;
  const size_t t = (size_t)xcd_block(blockIdx.x, gridDim.x, a.xcd_order ? kXcdRuns16 : kXcdOff) * kBlock + threadIdx.x;
  const TapRows R = tap_rows<PAIR>(V);
  unsigned steps = 0, failed = 0;
  size_t i;
  if (ray_index(a.perm, t, a.n, i)) {
    const Ray3 p = ld3(a.pos, i), u = ld3(a.vel, i);
    const float p0[3] = {p.x, p.y, p.z}, v0[3] = {u.x, u.y, u.z};
    OplTaps<PAIR> taps(V, R);
    float opl;
    const RayOut r = trace_opl_ray(V, a.ds, a.max_steps, p0, v0, taps, opl);
    steps = r.steps; failed = r.act ? 1u : 0u;
    st3(a.xt, i, r.xt[0], r.xt[1], r.xt[2]);
    st3(a.vt, i, r.vt[0], r.vt[1], r.vt[2]);
    a.opl[i] = opl;
    a.steps_out[i] = r.steps;
  }
  block_stats(a.stats, steps, failed);
}

template <bool PAIR>
__global__ void __launch_bounds__(kBlock) k_backtrace_opl(OplBackArgs a) {
  const Vol& V = a.vol;
  const size_t t = (size_t)xcd_block(blockIdx.x, gridDim.x, a.xcd_order ? kXcdRuns16 : kXcdOff) * kBlock + threadIdx.x;
  const TapRows R = tap_rows<PAIR>(V);
  unsigned steps = 0, failed = 0;
  size_t i;
  if (ray_index(a.perm, t, a.n, i)) {
    const Ray3 zero{0.f, 0.f, 0.f};
    const Ray3 p = ld3(a.pos, i), u = ld3(a.vel, i), xe = ld3(a.xt, i), ve = ld3(a.vt, i);
    const Ray3 gx = a.dx ? ld3(a.dx, i) : zero, gv = a.dv ? ld3(a.dv, i) : zero;
    const float p0[3] = {p.x, p.y, p.z}, v0[3] = {u.x, u.y, u.z}, xt[3] = {xe.x, xe.y, xe.z}, vt[3] = {ve.x, ve.y, ve.z};
    const float dx[3] = {gx.x, gx.y, gx.z}, dv[3] = {gv.x, gv.y, gv.z};
    const float dopl = a.dopl ? a.dopl[i] : 0.f;
    OplTaps<PAIR> taps(V, R);
    HeldCorners acc(a.grad);
    const bool scatter = a.grad != nullptr;
    const RayGrad g = opl_backtrace_ray(V, a.ds, a.grad_scale, a.max_steps, a.fsteps[i], p0, v0, xt, vt, dx, dv, dopl, taps,
      [&](const Cell& c, float val, float sx, float sy, float sz) {
        if (scatter) acc.add(c, splat_weights(c.wx, c.wy, c.wz, val, sx, sy, sz));
      });
    acc.flush();
    steps = g.steps; failed = g.failed ? 1u : 0u;
    if (a.dpos) {
      st3(a.dpos, i, g.dp[0], g.dp[1], g.dp[2]);
      st3(a.dvel, i, g.dv[0], g.dv[1], g.dv[2]);
    }
  }
  block_stats(a.stats, steps, failed);
}

void launch_trace_opl(const OplTraceArgs& a, hipStream_t s) {
  const dim3 g(grid_for(a.n)), b(kBlock);
  if (a.vol.pair != nullptr) hipLaunchKernelGGL(k_trace_opl<true>, g, b, 0, s, a);
  else                       hipLaunchKernelGGL(k_trace_opl<false>, g, b, 0, s, a);
}

void launch_backtrace_opl(const OplBackArgs& a, hipStream_t s) {
  const dim3 g(grid_for(a.n)), b(kBlock);
  if (a.vol.pair != nullptr) hipLaunchKernelGGL(k_backtrace_opl<true>, g, b, 0, s, a);
  else                       hipLaunchKernelGGL(k_backtrace_opl<false>, g, b, 0, s, a);
}

}  // namespace drrt
