// raygrad_host.hip -- TEST INFRASTRUCTURE ONLY (never built or loaded by the package).
//
// The per-ray routine of the ray-state adjoint (backtrace_ray_state, adjointnonlinearraytracing_amd/csrc/drrt_device.h)
// compiled for the HOST with `hipcc --cuda-host-only -ffp-contract=off`, as tests/hostcheck does for the march: the CPU
// tier compares it with float64 autograd, the GPU tier compares k_backtrace_rays with it bit for bit.
#include <stdint.h>
#include <stddef.h>

#include "../../adjointnonlinearraytracing_amd/csrc/drrt_device.h"

using namespace drrt;

#define EXPORT extern "C" __attribute__((visibility("default")))

// dpos, dvel: (n,3); steps: the forward's per-ray iteration counts; *ray_steps, *n_failed as in drrt_stats
EXPORT int raygrad_host_backtrace_rays(const float* rif, const int* res, size_t n, const float* pos, const float* vel,
                                       const float* xt, const float* vt, const uint32_t* steps, const float* dx,
                                       const float* dv, float h, float ds, float* dpos, float* dvel,
                                       long long* ray_steps, long long* n_failed) {
  Vol V;
  V.data = rif; V.W = res[0]; V.H = res[1]; V.D = res[2];
  vol_finish(V, h);
  const int m = res[0] > res[1] ? (res[0] > res[2] ? res[0] : res[2]) : (res[1] > res[2] ? res[1] : res[2]);
  const int max_steps = (int)(4.0f * h * (float)m / ds);             // the forward's bound (drrt_api.hip steps_fwd)
  long long st = 0, nf = 0;
  for (size_t i = 0; i < n; ++i) {
    const RayGrad g = backtrace_ray_state(V, ds, max_steps, steps[i], pos + 3 * i, vel + 3 * i, xt + 3 * i, vt + 3 * i,
                                          dx + 3 * i, dv + 3 * i, [&](const Cell& c) { return fetch(V.data, c); });
    for (int k = 0; k < 3; ++k) { dpos[3 * i + k] = g.dp[k]; dvel[3 * i + k] = g.dv[k]; }
    st += g.steps; nf += g.failed ? 1 : 0;
  }
  *ray_steps = st; *n_failed = nf;
  return 0;
}
