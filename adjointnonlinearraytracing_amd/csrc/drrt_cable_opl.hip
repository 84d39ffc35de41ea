// drrt_cable_opl.hip -- gfx950 kernels of the fibre march with its optical path length and of its ONE adjoint
// (drrt_trace_cable_opl_f32, drrt_backtrace_cable_opl_f32; not in the reference).  Per-ray arithmetic: cable_trace_opl_ray
// and cable_opl_backtrace_ray of drrt_device.h, which tests/hostcheck/cable_opl_rays.hip runs on the host; shared pieces:
// drrt_march.h.
//
// One ray per lane, grid-stride like the other cable kernels, the profile staged into LDS under their rule.  The forward
// stores the iteration of every ray's record, so the adjoint replays nothing: a lane runs that many reverse iterations in
// registers.  That count comes from caller memory and is the only loop bound of the adjoint; cable_opl_backtrace_ray
// refuses one above the forward's own bound (zero gradients, counted in stats->n_failed).
//   k_backtrace_cable_opl<PROFILE, RAYS>   PROFILE: the contributions to dL/d(profile) go into k_backtrace_cable's f64 LDS
//                                          accumulators (cable_grad_add / cable_grad_flush), or into global atomics above
//                                          kCableMaxRes; without it there are no accumulators and no atomics but the
//                                          statistics.  RAYS: dpos and dvel are stored.
#include "drrt_march.h"

namespace drrt {

__global__ void __launch_bounds__(kBlock) k_trace_cable_opl(CableOplTraceArgs a) {
  extern __shared__ float s_prof[];
  const bool use_lds = a.rres <= kCableMaxRes;
  if (use_lds) {
    for (int k = threadIdx.x; k < a.rres; k += kBlock) s_prof[k] = a.rif[k];
    __syncthreads();
  }
  const Cyl C = make_cyl(use_lds ? s_prof : a.rif, a.rres, a.radius, a.length);
  unsigned steps_tot = 0, fail_tot = 0, steps_max = 0;
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < a.n; i += (size_t)gridDim.x * kBlock) {
    const Ray3 p = ld3(a.pos, i), u = ld3(a.vel, i), tg = ld3(a.target, i);
    const float pp[3] = {p.x, p.y, p.z}, vv[3] = {u.x, u.y, u.z}, tt[3] = {tg.x, tg.y, tg.z};
    float opl; unsigned j;
    const RayOut r = cable_trace_opl_ray(C, a.ds, a.max_steps, pp, vv, tt, opl, j);
    st3(a.xt, i, r.xt[0], r.xt[1], r.xt[2]); st3(a.vt, i, r.vt[0], r.vt[1], r.vt[2]); a.dist2[i] = r.dist2;
    a.opl[i] = opl; a.rec_steps[i] = j;
    steps_tot += r.steps; steps_max = max(steps_max, r.steps); fail_tot += r.esc ? 0u : 1u;
  }
  cable_stats(a.stats, steps_tot, steps_max, fail_tot);
}

template <bool PROFILE, bool RAYS>
__global__ void __launch_bounds__(kBlock) k_backtrace_cable_opl(CableOplBackArgs a) {
  // LDS as in k_backtrace_cable: the gradient accumulators (doubles, PROFILE only) followed by the profile (floats)
  extern __shared__ double s_mem64[];
  const bool use_lds = a.rres <= kCableMaxRes;
  double* s_grad = s_mem64;
  float* s_prof = reinterpret_cast<float*>(s_mem64 + (PROFILE && use_lds ? a.rres : 0));
  if (use_lds) {
    for (int k = threadIdx.x; k < a.rres; k += kBlock) {
      s_prof[k] = a.rif[k];
      if (PROFILE) s_grad[k] = 0.0;
    }
    __syncthreads();
  }
  const Cyl C = make_cyl(use_lds ? s_prof : a.rif, a.rres, a.radius, a.length);
  float* gacc = a.grad;
  unsigned steps_tot = 0, steps_max = 0, fail_tot = 0;
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < a.n; i += (size_t)gridDim.x * kBlock) {
    const Ray3 zero = {0.f, 0.f, 0.f};
    const Ray3 p = ld3(a.pos, i), x = ld3(a.xt, i), u = ld3(a.vt, i);
    const Ray3 gx = a.dx ? ld3(a.dx, i) : zero, gv = a.dv ? ld3(a.dv, i) : zero;
    const float p0[3] = {p.x, p.y, p.z}, xt[3] = {x.x, x.y, x.z}, vt[3] = {u.x, u.y, u.z};
    const float dx[3] = {gx.x, gx.y, gx.z}, dv[3] = {gv.x, gv.y, gv.z};
    const RayGrad g = cable_opl_backtrace_ray(C, a.ds, a.max_steps, p0, xt, vt, a.rec_steps[i], dx, dv,
                                              a.dopl ? a.dopl[i] : 0.f,
      [s_grad, gacc, use_lds](int i0, int i1, float a0, float a1) {
        if (PROFILE) cable_grad_add(s_grad, gacc, use_lds, i0, i1, a0, a1);
      });
    if (RAYS) {
      st3(a.dpos, i, g.dp[0], g.dp[1], g.dp[2]);
      st3(a.dvel, i, g.dv[0], g.dv[1], g.dv[2]);
    }
    steps_tot += g.steps; steps_max = max(steps_max, g.steps); fail_tot += g.failed ? 1u : 0u;
  }
  if (PROFILE && use_lds) cable_grad_flush(s_grad, a.grad, a.rres);
  cable_stats(a.stats, steps_tot, steps_max, fail_tot);
}

// ---- launchers ----------------------------------------------------------------------------------
void launch_trace_cable_opl(const CableOplTraceArgs& a, hipStream_t s) {
  const size_t lds = (a.rres <= kCableMaxRes) ? a.rres * sizeof(float) : 0;
  hipLaunchKernelGGL(k_trace_cable_opl, dim3(cable_grid(a.n)), dim3(kBlock), lds, s, a);
}
void launch_backtrace_cable_opl(const CableOplBackArgs& a, hipStream_t s) {
  const bool profile = a.grad != nullptr, rays = a.dpos != nullptr;
  const size_t lds = (a.rres <= kCableMaxRes) ? a.rres * (sizeof(float) + (profile ? sizeof(double) : 0)) : 0;
  const dim3 grid(cable_grid(a.n)), block(kBlock);
  if (profile && rays) hipLaunchKernelGGL((k_backtrace_cable_opl<true, true>), grid, block, lds, s, a);
  else if (profile) hipLaunchKernelGGL((k_backtrace_cable_opl<true, false>), grid, block, lds, s, a);
  else hipLaunchKernelGGL((k_backtrace_cable_opl<false, true>), grid, block, lds, s, a);
}

}  // namespace drrt
