// drrt_cable_rays.hip -- gfx950 kernel of the ray-state adjoint of Tracer::trace_cable: dL/dpos and dL/dvel of the rays
// that entered a fibre march (drrt_backtrace_cable_rays_f32; the reference's ADCableTracerC returns them through enoki
// autodiff, core/tracer.py:237-291).  Per-ray arithmetic: cable_backtrace_ray_state of drrt_device.h, which
// tests/hostcheck runs on the host; shared pieces: drrt_march.h.
//
// One ray per lane, grid-stride like the two cable kernels, the profile staged into LDS under their rule.  A lane replays
// the forward march of its ray to find the iteration j of the closest-approach record (the forward does not report it),
// then runs j reverse iterations in registers.  Nothing is accumulated into the profile: no LDS accumulators, no atomics
// but the statistics; the only stores are dpos and dvel.
#include "drrt_march.h"

namespace drrt {

__global__ void __launch_bounds__(kBlock) k_backtrace_cable_rays(CableRayGradArgs a) {
  extern __shared__ float s_prof[];
  const bool use_lds = a.rres <= kCableMaxRes;
  if (use_lds) {
    for (int k = threadIdx.x; k < a.rres; k += kBlock) s_prof[k] = a.rif[k];
    __syncthreads();
  }
  const Cyl C = make_cyl(use_lds ? s_prof : a.rif, a.rres, a.radius, a.length);
  unsigned steps_tot = 0, steps_max = 0;
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < a.n; i += (size_t)gridDim.x * kBlock) {
    const Ray3 p = ld3(a.pos, i), u = ld3(a.vel, i), tg = ld3(a.target, i), gx = ld3(a.dx, i), gv = ld3(a.dv, i);
    const float p0[3] = {p.x, p.y, p.z}, v0[3] = {u.x, u.y, u.z}, tt[3] = {tg.x, tg.y, tg.z};
    const float dx[3] = {gx.x, gx.y, gx.z}, dv[3] = {gv.x, gv.y, gv.z};
    const RayGrad g = cable_backtrace_ray_state(C, a.ds, a.max_steps, p0, v0, tt, dx, dv);
    st3(a.dpos, i, g.dp[0], g.dp[1], g.dp[2]);
    st3(a.dvel, i, g.dv[0], g.dv[1], g.dv[2]);
    steps_tot += g.steps; steps_max = max(steps_max, g.steps);
  }
  cable_stats(a.stats, steps_tot, steps_max, 0u);
}

void launch_backtrace_cable_rays(const CableRayGradArgs& a, hipStream_t s) {
  const size_t lds = (a.rres <= kCableMaxRes) ? a.rres * sizeof(float) : 0;
  hipLaunchKernelGGL(k_backtrace_cable_rays, dim3(cable_grid(a.n)), dim3(kBlock), lds, s, a);
}

}  // namespace drrt
