// drrt_cable_field.hip -- gfx950 kernels of the fibre march with the line integral of a second radial profile and of its
// ONE adjoint (drrt_trace_cable_field_f32, drrt_backtrace_cable_field_f32; not in the reference).  Per-ray arithmetic:
// cable_trace_field_ray and cable_field_backtrace_ray of drrt_device.h, which tests/hostcheck/cable_field_rays.hip runs on
// the host; shared pieces: drrt_march.h.
//
// One ray per lane, grid-stride like the other cable kernels.  Both profiles are staged into LDS, and every requested
// profile gradient has its own f64 LDS accumulator array (cable_grad_add / cable_grad_flush), as long as
// cable_field_lds_bytes -- the one expression launcher and kernel share -- says it fits; otherwise the profiles are read
// from global memory and the contributions go into global atomics.  As in drrt_cable_opl.hip the forward stores the
// iteration of every ray's record, the adjoint replays nothing, and that count is the adjoint's only loop bound
// (cable_field_backtrace_ray refuses one above the forward's own bound: zero gradients, counted in stats->n_failed).
//   k_backtrace_cable_field<PROFILE, FIELD, RAYS>   PROFILE: dL/d(profile) is accumulated; FIELD: dL/d(field) is; RAYS: dpos
//                                                   and dvel are stored.  The seven combinations with an output exist.
#include "drrt_march.h"

namespace drrt {

__global__ void __launch_bounds__(kBlock) k_trace_cable_field(CableFieldTraceArgs a) {
  extern __shared__ float s_prof[];
  const bool use_lds = cable_field_lds_bytes(a.rres, false, false) != 0;
  float* s_field = s_prof + a.rres;
  if (use_lds) {
    for (int k = threadIdx.x; k < a.rres; k += kBlock) { s_prof[k] = a.rif[k]; s_field[k] = a.field[k]; }
    __syncthreads();
  }
  const Cyl C = make_cyl(use_lds ? s_prof : a.rif, a.rres, a.radius, a.length);
  const float* fa = use_lds ? s_field : a.field;
  unsigned steps_tot = 0, fail_tot = 0, steps_max = 0;
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < a.n; i += (size_t)gridDim.x * kBlock) {
    const Ray3 p = ld3(a.pos, i), u = ld3(a.vel, i), tg = ld3(a.target, i);
    const float pp[3] = {p.x, p.y, p.z}, vv[3] = {u.x, u.y, u.z}, tt[3] = {tg.x, tg.y, tg.z};
    float tau; unsigned j;
    const RayOut r = cable_trace_field_ray(C, fa, a.ds, a.max_steps, pp, vv, tt, tau, j);
    st3(a.xt, i, r.xt[0], r.xt[1], r.xt[2]); st3(a.vt, i, r.vt[0], r.vt[1], r.vt[2]); a.dist2[i] = r.dist2;
    a.tau[i] = tau; a.rec_steps[i] = j;
    steps_tot += r.steps; steps_max = max(steps_max, r.steps); fail_tot += r.esc ? 0u : 1u;
  }
  cable_stats(a.stats, steps_tot, steps_max, fail_tot);
}

template <bool PROFILE, bool FIELD, bool RAYS>
__global__ void __launch_bounds__(kBlock) k_backtrace_cable_field(CableFieldBackArgs a) {
  // LDS: the accumulators of dL/d(profile) (doubles, PROFILE only), those of dL/d(field) (doubles, FIELD only), the
  // profile and the field (floats)
  extern __shared__ double s_mem64[];
  const bool use_lds = cable_field_lds_bytes(a.rres, PROFILE, FIELD) != 0;
  const int res = use_lds ? a.rres : 0;
  double* s_grad = s_mem64;
  double* s_gfield = s_grad + (PROFILE ? res : 0);
  float* s_prof = reinterpret_cast<float*>(s_gfield + (FIELD ? res : 0));
  float* s_field = s_prof + res;
  if (use_lds) {
    for (int k = threadIdx.x; k < a.rres; k += kBlock) {
      s_prof[k] = a.rif[k]; s_field[k] = a.field[k];
      if (PROFILE) s_grad[k] = 0.0;
      if (FIELD) s_gfield[k] = 0.0;
    }
    __syncthreads();
  }
  const Cyl C = make_cyl(use_lds ? s_prof : a.rif, a.rres, a.radius, a.length);
  const float* fa = use_lds ? s_field : a.field;
  float* gacc = a.grad;
  float* facc = a.grad_field;
  unsigned steps_tot = 0, steps_max = 0, fail_tot = 0;
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < a.n; i += (size_t)gridDim.x * kBlock) {
    const Ray3 zero = {0.f, 0.f, 0.f};
    const Ray3 p = ld3(a.pos, i), x = ld3(a.xt, i), u = ld3(a.vt, i);
    const Ray3 gx = a.dx ? ld3(a.dx, i) : zero, gv = a.dv ? ld3(a.dv, i) : zero;
    const float p0[3] = {p.x, p.y, p.z}, xt[3] = {x.x, x.y, x.z}, vt[3] = {u.x, u.y, u.z};
    const float dx[3] = {gx.x, gx.y, gx.z}, dv[3] = {gv.x, gv.y, gv.z};
    const RayGrad g = cable_field_backtrace_ray(C, fa, a.ds, a.max_steps, p0, xt, vt, a.rec_steps[i], dx, dv,
                                                a.dtau ? a.dtau[i] : 0.f,
      [s_grad, gacc, use_lds](int i0, int i1, float a0, float a1) {
        if (PROFILE) cable_grad_add(s_grad, gacc, use_lds, i0, i1, a0, a1);
      },
      [s_gfield, facc, use_lds](int i0, int i1, float a0, float a1) {
        if (FIELD) cable_grad_add(s_gfield, facc, use_lds, i0, i1, a0, a1);
      });
    if (RAYS) {
      st3(a.dpos, i, g.dp[0], g.dp[1], g.dp[2]);
      st3(a.dvel, i, g.dv[0], g.dv[1], g.dv[2]);
    }
    steps_tot += g.steps; steps_max = max(steps_max, g.steps); fail_tot += g.failed ? 1u : 0u;
  }
  if (PROFILE && use_lds) cable_grad_flush(s_grad, a.grad, a.rres);
  if (FIELD && use_lds) cable_grad_flush(s_gfield, a.grad_field, a.rres);
  cable_stats(a.stats, steps_tot, steps_max, fail_tot);
}

// ---- launchers ----------------------------------------------------------------------------------
void launch_trace_cable_field(const CableFieldTraceArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_trace_cable_field, dim3(cable_grid(a.n)), dim3(kBlock), cable_field_lds_bytes(a.rres, false, false),
                     s, a);
}

template <bool PROFILE, bool FIELD, bool RAYS>
static void launch_one(const CableFieldBackArgs& a, hipStream_t s) {
  hipLaunchKernelGGL((k_backtrace_cable_field<PROFILE, FIELD, RAYS>), dim3(cable_grid(a.n)), dim3(kBlock),
                     cable_field_lds_bytes(a.rres, PROFILE, FIELD), s, a);
}

void launch_backtrace_cable_field(const CableFieldBackArgs& a, hipStream_t s) {
  const bool profile = a.grad != nullptr, field = a.grad_field != nullptr, rays = a.dpos != nullptr;
  switch ((profile ? 4 : 0) | (field ? 2 : 0) | (rays ? 1 : 0)) {
    case 7: launch_one<true, true, true>(a, s); break;
    case 6: launch_one<true, true, false>(a, s); break;
    case 5: launch_one<true, false, true>(a, s); break;
    case 4: launch_one<true, false, false>(a, s); break;
    case 3: launch_one<false, true, true>(a, s); break;
    case 2: launch_one<false, true, false>(a, s); break;
    case 1: launch_one<false, false, true>(a, s); break;
    default: break;                                  // nothing asked for: the entry point refuses that
  }
}

}  // namespace drrt
