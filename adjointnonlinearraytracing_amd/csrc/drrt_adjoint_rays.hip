// drrt_adjoint_rays.hip -- gfx950 kernel of the ray-state adjoint of Tracer::trace: dL/dpos and dL/dvel of the rays
// that entered a trace call (drrt_backtrace_rays_f32; the reference's ADTracerC returns them through enoki autodiff,
// core/tracer.py:16-66).  Per-ray arithmetic: backtrace_ray_state of drrt_device.h, which tests/hostcheck runs on the
// host; shared pieces: drrt_march.h.
//
// One ray per lane, the whole reverse march in registers: (x, v, lambda, mu) and the taps of the current cell.  Nothing
// is written to the grid -- no LDS window, no atomics -- so, unlike the dL/dn adjoint, this march is bound by its gathers
// and its arithmetic alone, like the forward march.  A lane keeps the taps of a strictly interior cell while it stays
// in it (the forward's rule, k_trace_flat); boundary cells are fetched with their clamps (fetch of drrt_device.h).
#include "drrt_march.h"

namespace drrt {

template <bool PAIR>
__global__ void __launch_bounds__(kBlock) k_backtrace_rays(RayGradArgs a) {
  const Vol& V = a.vol;
  const size_t t = (size_t)xcd_block(blockIdx.x, gridDim.x, a.xcd_order ? kXcdRuns16 : kXcdOff) * kBlock + threadIdx.x;
  const TapRows R = tap_rows<PAIR>(V);
  unsigned steps = 0, failed = 0;
  size_t i;
  if (ray_index(a.perm, t, a.n, i)) {
    const Ray3 p = ld3(a.pos, i), u = ld3(a.vel, i), xe = ld3(a.xt, i), ve = ld3(a.vt, i);
    const Ray3 gx = ld3(a.dx, i), gv = ld3(a.dv, i);
    const float p0[3] = {p.x, p.y, p.z}, v0[3] = {u.x, u.y, u.z}, xt[3] = {xe.x, xe.y, xe.z}, vt[3] = {ve.x, ve.y, ve.z};
    const float dx[3] = {gx.x, gx.y, gx.z}, dv[3] = {gv.x, gv.y, gv.z};
    unsigned off = 0;          // byte offset (tap_offset) of the interior cell whose taps the lane holds
    bool held = false;
    f4 q0 = f4{0.f, 0.f, 0.f, 0.f}, q1 = q0;
    const RayGrad g = backtrace_ray_state(V, a.ds, a.max_steps, a.fsteps[i], p0, v0, xt, vt, dx, dv,
      [&](const Cell& c) -> Taps {
        if (!c.interior) { held = false; return fetch(V.data, c); }
        const unsigned noff = tap_offset<PAIR>(c.base);
        if (!(held & (noff == off))) { gather_rows<PAIR>(R, noff, q0, q1); off = noff; held = true; }
        return taps_of<PAIR>(q0, q1);
      });
    steps = g.steps; failed = g.failed ? 1u : 0u;
    st3(a.dpos, i, g.dp[0], g.dp[1], g.dp[2]);
    st3(a.dvel, i, g.dv[0], g.dv[1], g.dv[2]);
  }
  block_stats(a.stats, steps, failed);
}

void launch_backtrace_rays(const RayGradArgs& a, hipStream_t s) {
  const dim3 g(grid_for(a.n)), b(kBlock);
  if (a.vol.pair != nullptr) hipLaunchKernelGGL(k_backtrace_rays<true>, g, b, 0, s, a);
  else                       hipLaunchKernelGGL(k_backtrace_rays<false>, g, b, 0, s, a);
}

}  // namespace drrt
