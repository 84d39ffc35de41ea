// drrt_cable.hip -- gfx950 kernels of the radial-profile (fibre) march and its adjoint: Tracer::trace_cable,
// backtrace_cable (/root/reference/src/tracer.cpp:312-382, 511-567; src/cylinder_volume.cpp).
#include "drrt_march.h"

namespace drrt {

__global__ void __launch_bounds__(kBlock) k_trace_cable(CableArgs a) {
  extern __shared__ float s_prof[];
  const bool use_lds = a.rres <= kCableMaxRes;
  if (use_lds) {
    for (int k = threadIdx.x; k < a.rres; k += kBlock) s_prof[k] = a.rif[k];
    __syncthreads();
  }
  const Cyl C = make_cyl(use_lds ? s_prof : a.rif, a.rres, a.radius, a.length);
  unsigned steps_tot = 0, fail_tot = 0, steps_max = 0;
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < a.n; i += (size_t)gridDim.x * kBlock) {
    Ray3 p = ld3(a.pos, i), u = ld3(a.vel, i), tg = ld3(a.target, i);
    const float pp[3] = {p.x, p.y, p.z}, vv[3] = {u.x, u.y, u.z}, tt[3] = {tg.x, tg.y, tg.z};
    RayOut r = cable_trace_ray(C, a.ds, a.max_steps, pp, vv, tt);
    st3(a.xt, i, r.xt[0], r.xt[1], r.xt[2]); st3(a.vt, i, r.vt[0], r.vt[1], r.vt[2]); a.dist2[i] = r.dist2;
    steps_tot += r.steps; steps_max = max(steps_max, r.steps); fail_tot += r.esc ? 0u : 1u;
  }
  cable_stats(a.stats, steps_tot, steps_max, fail_tot);
}

__global__ void __launch_bounds__(kBlock) k_backtrace_cable(CableArgs a) {
  // LDS: the profile (floats) followed by the gradient accumulators (doubles: ds_add_f64 is ~25x
  // cheaper than ds_add_f32 on gfx950, tools/lds_atomic_bench.hip, and sums are more accurate)
  extern __shared__ double s_mem64[];
  const bool use_lds = a.rres <= kCableMaxRes;
  double* s_grad = s_mem64;
  float* s_prof = reinterpret_cast<float*>(s_mem64 + (use_lds ? a.rres : 0));
  if (use_lds) {
    for (int k = threadIdx.x; k < a.rres; k += kBlock) { s_prof[k] = a.rif[k]; s_grad[k] = 0.0; }
    __syncthreads();
  }
  const Cyl C = make_cyl(use_lds ? s_prof : a.rif, a.rres, a.radius, a.length);
  float* gacc = a.grad;
  unsigned steps_tot = 0, steps_max = 0;
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < a.n; i += (size_t)gridDim.x * kBlock) {
    Ray3 p = ld3(a.pos, i), u = ld3(a.vel, i), gxv = ld3(a.dx, i), gvv = ld3(a.dv, i);
    const float pp[3] = {p.x, p.y, p.z}, vv[3] = {u.x, u.y, u.z};
    const float dxx[3] = {gxv.x, gxv.y, gxv.z}, dvv[3] = {gvv.x, gvv.y, gvv.z};
    unsigned steps = cable_backtrace_ray(C, a.ds, a.max_steps, pp, vv, dxx, dvv,
      [s_grad, gacc, use_lds](int i0, int i1, float a0, float a1) { cable_grad_add(s_grad, gacc, use_lds, i0, i1, a0, a1); });
    steps_tot += steps; steps_max = max(steps_max, steps);
  }
  if (use_lds) cable_grad_flush(s_grad, a.grad, a.rres);
  cable_stats(a.stats, steps_tot, steps_max, 0u);
}

// ---- launchers ----------------------------------------------------------------------------------
void launch_trace_cable(const CableArgs& a, hipStream_t s) {
  const size_t lds = (a.rres <= kCableMaxRes) ? a.rres * sizeof(float) : 0;
  hipLaunchKernelGGL(k_trace_cable, dim3(cable_grid(a.n)), dim3(kBlock), lds, s, a);
}
void launch_backtrace_cable(const CableArgs& a, hipStream_t s) {
  const size_t lds = (a.rres <= kCableMaxRes) ? a.rres * (sizeof(double) + sizeof(float)) : 0;
  hipLaunchKernelGGL(k_backtrace_cable, dim3(cable_grid(a.n)), dim3(kBlock), lds, s, a);
}

}  // namespace drrt
