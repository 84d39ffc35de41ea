// cable_raygrad_host.hip -- TEST INFRASTRUCTURE ONLY (never built or loaded by the package).
//
// The per-ray routine of the cable march's ray-state adjoint (cable_backtrace_ray_state,
// adjointnonlinearraytracing_amd/csrc/drrt_device.h) compiled for the HOST with `hipcc --cuda-host-only
// -ffp-contract=off`, as tests/raygrad_host does for the box march: the CPU tier compares it with float64 autograd, the
// GPU tier compares k_backtrace_cable_rays with it bit for bit.
#include <stdint.h>
#include <stddef.h>

#include "../../adjointnonlinearraytracing_amd/csrc/drrt_device.h"

using namespace drrt;

#define EXPORT extern "C" __attribute__((visibility("default")))

// dpos, dvel, xt, vt: (n,3); jstar: the iteration of the replayed closest-approach record; steps: replay + reverse
// iterations per ray (their sum is drrt_stats.ray_steps, their maximum drrt_stats.iters)
EXPORT int cable_raygrad_host_backtrace_rays(const float* rif, int rres, float radius, float length, size_t n,
                                             const float* pos, const float* vel, const float* target, const float* dx,
                                             const float* dv, float ds, float* dpos, float* dvel, float* xt, float* vt,
                                             uint32_t* jstar, uint32_t* steps) {
  const Cyl C = make_cyl(rif, rres, radius, length);
  const int max_steps = (int)(4.0f * length / ds);                   // the forward's bound (drrt_trace_cable_f32)
  for (size_t i = 0; i < n; ++i) {
    CableRecord rec;
    const RayGrad g = cable_backtrace_ray_state(C, ds, max_steps, pos + 3 * i, vel + 3 * i, target + 3 * i, dx + 3 * i,
                                                dv + 3 * i, &rec);
    for (int k = 0; k < 3; ++k) {
      dpos[3 * i + k] = g.dp[k]; dvel[3 * i + k] = g.dv[k]; xt[3 * i + k] = rec.xt[k]; vt[3 * i + k] = rec.vt[k];
    }
    jstar[i] = rec.j; steps[i] = g.steps;
    if (g.failed) return 1;
  }
  return 0;
}
