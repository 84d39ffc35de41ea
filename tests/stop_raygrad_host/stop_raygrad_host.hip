// stop_raygrad_host.hip -- TEST INFRASTRUCTURE ONLY (never built or loaded by the package).
//
// The per-ray routine of the ray-state adjoints of trace_plane and trace_sdf (stop_backtrace_ray_state,
// adjointnonlinearraytracing_amd/csrc/drrt_device.h) compiled for the HOST with `hipcc --cuda-host-only
// -ffp-contract=off`, as tests/raygrad_host and tests/cable_raygrad_host do for the other two marches: the CPU tier
// compares it with float64 autograd, the GPU tier compares the kernels of drrt_stop_rays.hip with it bit for bit.  The
// two passes are looped as drrt_api.hip launches them: every ray with per-ray termination, then the flagged rays over
// the maximum of the first pass's iteration counts.
#include <stdint.h>
#include <stddef.h>

#include <vector>

#include "../../adjointnonlinearraytracing_amd/csrc/drrt_device.h"

using namespace drrt;

#define EXPORT extern "C" __attribute__((visibility("default")))

static int max3(const int r[3]) { return r[0] > r[1] ? (r[0] > r[2] ? r[0] : r[2]) : (r[1] > r[2] ? r[1] : r[2]); }

template <int MODE>
static void run(const float* rif, const float* sdf, const int* res, size_t n, const float* pos, const float* vel,
                const float* pln_o, const float* pln_d, const float* dx, const float* dv, float h, float ds, float* dpos,
                float* dvel, float* xt, float* vt, uint32_t* jstar, uint32_t* steps, uint32_t* fwd, uint8_t* flags, uint32_t* iters) {
  Vol V;
  V.data = rif; V.W = res[0]; V.H = res[1]; V.D = res[2];
  vol_finish(V, h);
  const int max_steps = MODE == 2 ? (int)(2.0f * h * (float)max3(res) / ds) : (int)(4.0f * h * (float)max3(res) / ds);
  auto taps = [&](const Cell& c) -> Taps { return fetch(V.data, c); };
  const float zero[3] = {0.f, 0.f, 0.f};
  unsigned total = 0;
  auto store = [&](size_t i, const StopGrad& g, const StopRecord& rec) {
    for (int k = 0; k < 3; ++k) {
      dpos[3 * i + k] = g.dp[k]; dvel[3 * i + k] = g.dv[k]; xt[3 * i + k] = rec.xt[k]; vt[3 * i + k] = rec.vt[k];
    }
    jstar[i] = rec.j;
  };
  std::vector<size_t> again;
  for (size_t i = 0; i < n; ++i) {
    const float* po = MODE == 1 ? pln_o + 3 * i : zero; const float* pd = MODE == 1 ? pln_d + 3 * i : zero;
    StopRecord rec;
    const StopGrad g = stop_backtrace_ray_state<MODE, false>(V, sdf, ds, max_steps, 0u, pos + 3 * i, vel + 3 * i, po, pd,
                                                             dx + 3 * i, dv + 3 * i, taps, &rec);
    steps[i] = g.steps; fwd[i] = g.fwd;
    flags[i] = (g.failed ? 1 : 0) | (g.again ? 2 : 0);
    if (g.fwd > total) total = g.fwd;
    if (g.again) again.push_back(i); else store(i, g, rec);
  }
  for (size_t i : again) {
    const float* po = MODE == 1 ? pln_o + 3 * i : zero; const float* pd = MODE == 1 ? pln_d + 3 * i : zero;
    StopRecord rec;
    const StopGrad g = stop_backtrace_ray_state<MODE, true>(V, sdf, ds, max_steps, total, pos + 3 * i, vel + 3 * i, po, pd,
                                                            dx + 3 * i, dv + 3 * i, taps, &rec);
    steps[i] += g.steps;
    store(i, g, rec);
  }
  *iters = total;
}

// mode 1 = trace_plane, 2 = trace_sdf.  dpos, dvel, xt, vt: (n,3); jstar: the iteration of the replayed record; steps:
// replayed forward + reverse iterations per ray (their sum is drrt_stats.ray_steps); fwd: the iterations of the first
// pass's replay (the forward's own per-ray count); flags: bit 0 failed, bit 1 the ray went
// through the second pass; iters: the global loop count (drrt_stats.iters)
EXPORT int stop_raygrad_host_backtrace_rays(int mode, const float* rif, const float* sdf, const int* res, size_t n,
                                            const float* pos, const float* vel, const float* pln_o, const float* pln_d,
                                            const float* dx, const float* dv, float h, float ds, float* dpos, float* dvel,
                                            float* xt, float* vt, uint32_t* jstar, uint32_t* steps, uint32_t* fwd,
                                            uint8_t* flags, uint32_t* iters) {
  if (mode == 1) run<1>(rif, sdf, res, n, pos, vel, pln_o, pln_d, dx, dv, h, ds, dpos, dvel, xt, vt, jstar, steps, fwd, flags, iters);
  else if (mode == 2) run<2>(rif, sdf, res, n, pos, vel, pln_o, pln_d, dx, dv, h, ds, dpos, dvel, xt, vt, jstar, steps, fwd, flags, iters);
  else return 1;
  return 0;
}
