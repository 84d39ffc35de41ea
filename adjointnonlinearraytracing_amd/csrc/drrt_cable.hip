// drrt_cable.hip -- gfx950 kernels of the radial-profile (fibre) march family:
//   k_trace_cable, k_backtrace_cable     Tracer::trace_cable, backtrace_cable (/root/reference/src/tracer.cpp:312-382,
//                                        511-567; src/cylinder_volume.cpp)
//   k_backtrace_cable_rays               ray-state adjoint of trace_cable: dL/dpos, dL/dvel (the reference's ADCableTracerC
//                                        returns them through enoki autodiff, core/tracer.py:237-291).  A lane replays the
//                                        forward march of its ray to find the iteration j of the record (the forward does
//                                        not report it), then runs j reverse iterations in registers.  Nothing is
//                                        accumulated into the profile: no LDS accumulators, no atomics but the statistics
//   k_trace_cable_opl, k_backtrace_cable_opl<PROFILE, RAYS>             the march with its optical path length, ONE adjoint
//   k_trace_cable_field, k_backtrace_cable_field<PROFILE, FIELD, RAYS>  the march with the line integral of a second radial
//                                        profile, ONE adjoint (neither is in the reference).  These forwards store the
//                                        iteration of every ray's record, so the adjoints replay nothing; that count comes
//                                        from caller memory and is the adjoint's only loop bound (one above the forward's
//                                        own bound is refused: zero gradients, counted in stats->n_failed).  PROFILE:
//                                        dL/d(profile) is accumulated; FIELD: dL/d(field) is; RAYS: dpos and dvel are
//                                        stored.  The combinations with an output exist.
// Per-ray arithmetic: the cable routines of drrt_device.h, which tests/hostcheck runs on the host; shared pieces:
// drrt_march.h.  One ray per lane, grid-stride, rays in caller order.  The profiles are staged into LDS, followed -- in the
// adjoints that accumulate -- by one f64 accumulator array per requested gradient, laid out accumulators first (doubles:
// ds_add_f64 is ~25x cheaper than ds_add_f32 on gfx950, tools/lds_atomic_bench.hip, and sums are more accurate;
// cable_grad_add / cable_grad_flush), as long as cable_lds_bytes (drrt_device.h), the launchers' rule, says it fits:
// otherwise the profiles are read from global memory and the contributions go into global atomics.  For one profile that
// is rres <= kCableMaxRes with or without its accumulators, which is how the single-profile kernels spell it.
// The kernel bodies are written out one by one: folded onto shared staging and lane helpers they compiled to other
// prologues and epilogues around the same loops and measured up to 2 % slower (NOTES.md 2026-10-20).
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

__global__ void __launch_bounds__(kBlock) k_trace_cable_field(CableFieldTraceArgs a) {
  extern __shared__ float s_prof[];
  const bool use_lds = cable_lds_bytes(a.rres, 2, 0) != 0;
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
  // LDS: the accumulators of dL/d(profile) (PROFILE only), those of dL/d(field) (FIELD only), the profile and the field
  extern __shared__ double s_mem64[];
  const bool use_lds = cable_lds_bytes(a.rres, 2, (PROFILE ? 1 : 0) + (FIELD ? 1 : 0)) != 0;
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
#define LAUNCH_CABLE(kernel, nprof, ngrad, a, s) \
  hipLaunchKernelGGL(kernel, dim3(cable_grid((a).n)), dim3(kBlock), cable_lds_bytes((a).rres, nprof, ngrad), s, a)

void launch_trace_cable(const CableArgs& a, hipStream_t s) { LAUNCH_CABLE(k_trace_cable, 1, 0, a, s); }
void launch_backtrace_cable(const CableArgs& a, hipStream_t s) { LAUNCH_CABLE(k_backtrace_cable, 1, 1, a, s); }
void launch_backtrace_cable_rays(const CableRayGradArgs& a, hipStream_t s) { LAUNCH_CABLE(k_backtrace_cable_rays, 1, 0, a, s); }
void launch_trace_cable_opl(const CableOplTraceArgs& a, hipStream_t s) { LAUNCH_CABLE(k_trace_cable_opl, 1, 0, a, s); }
void launch_trace_cable_field(const CableFieldTraceArgs& a, hipStream_t s) { LAUNCH_CABLE(k_trace_cable_field, 2, 0, a, s); }

// grad, grad_field and / or (dpos, dvel), whichever are non-null; nothing asked for launches nothing (the entry points
// refuse that)
void launch_backtrace_cable_opl(const CableOplBackArgs& a, hipStream_t s) {
  with_bools([&](auto profile, auto rays) {
    constexpr bool P = decltype(profile)::value, R = decltype(rays)::value;
    if constexpr (P || R) LAUNCH_CABLE((k_backtrace_cable_opl<P, R>), 1, P ? 1 : 0, a, s);
  }, a.grad != nullptr, a.dpos != nullptr);
}
void launch_backtrace_cable_field(const CableFieldBackArgs& a, hipStream_t s) {
  with_bools([&](auto profile, auto field, auto rays) {
    constexpr bool P = decltype(profile)::value, F = decltype(field)::value, R = decltype(rays)::value;
    if constexpr (P || F || R) LAUNCH_CABLE((k_backtrace_cable_field<P, F, R>), 2, (P ? 1 : 0) + (F ? 1 : 0), a, s);
  }, a.grad != nullptr, a.grad_field != nullptr, a.dpos != nullptr);
}

}  // namespace drrt
