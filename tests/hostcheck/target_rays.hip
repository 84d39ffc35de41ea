// target_rays.hip -- TEST INFRASTRUCTURE ONLY (never built or loaded by the package).
//
// The host build of the ray-state adjoint of trace_target: target_backtrace_ray_state of
// adjointnonlinearraytracing_amd/csrc/drrt_device.h, looped as drrt_ray_adjoints.hip launches it -- a first pass for the
// call's global loop count, a second for the replay and the reverse march.  Compiled by tests/target_raygrad_host.py with the
// line of tests/hostcheck_lib.py (`hipcc --cuda-host-only -O2 -ffp-contract=off -mfma`): the CPU tier compares it with float64
// autograd (tests/target_ad.py), the GPU tier compares the kernels with it bit for bit.
//
// With -DTARGET_RAYS_MAIN it is a stand-alone program (its own main, nothing preloaded) for a build under AddressSanitizer
// + UndefinedBehaviorSanitizer: argv[1] names a file with one case (see main), the routine runs on it, 0 = no report.
#include "host_common.h"

// dpos, dvel, xt, vt: (n,3); dd2: n floats or null; dist2, jstar (the iteration of the replayed record), fwd (phase A's
// iteration count), steps (replayed + reverse iterations of the second pass), failed: n each; *iters: the global loop count
EXPORT int target_raygrad_host_backtrace_rays(const float* rif, const int* res, size_t n, const float* pos, const float* vel,
                                              const float* target, const float* dx, const float* dv, const float* dd2,
                                              float h, float ds, float* dpos, float* dvel, float* xt, float* vt, float* dist2,
                                              uint32_t* jstar, uint32_t* fwd, uint32_t* steps, uint8_t* failed,
                                              uint32_t* iters) {
  const Vol V = vol(rif, res, h);
  const int max_steps = max_steps_of(res, h, ds);
  const GridTaps taps{rif};
  unsigned total = 0;
  for (size_t i = 0; i < n; ++i) {                                   // k_target_rays_count
    TargetReplay r;
    target_replay_a(V, ds, max_steps, pos + 3 * i, vel + 3 * i, pos + 3 * i, taps, r);
    if (r.done > total) total = r.done;
  }
  for (size_t i = 0; i < n; ++i) {                                   // k_backtrace_target_rays
    TargetRecord rec;
    const TargetGrad g = target_backtrace_ray_state(V, ds, max_steps, total, pos + 3 * i, vel + 3 * i, target + 3 * i,
                                                    dx + 3 * i, dv + 3 * i, dd2 ? dd2[i] : 0.f, taps, &rec);
    for (int k = 0; k < 3; ++k) {
      dpos[3 * i + k] = g.dp[k]; dvel[3 * i + k] = g.dv[k]; xt[3 * i + k] = rec.xt[k]; vt[3 * i + k] = rec.vt[k];
    }
    dist2[i] = rec.dist2; jstar[i] = rec.j; fwd[i] = g.fwd; steps[i] = g.steps; failed[i] = g.failed ? 1 : 0;
  }
  *iters = total;
  return 0;
}

#ifdef TARGET_RAYS_MAIN
// The case file: int32 W, H, D, n; float32 h, ds; then float32 arrays rif[W*H*D], pos, vel, target, dx, dv (n*3 each), dd2[n].
int main(int argc, char** argv) {
  CaseFile c(argc, argv);
  const size_t n = c.n;
  const std::vector<float> rif = c.floats(c.nvox), pos = c.floats(3 * n), vel = c.floats(3 * n), tg = c.floats(3 * n),
                           dx = c.floats(3 * n), dv = c.floats(3 * n), dd2 = c.floats(n);
  if (!c.ok) return 2;
  std::vector<float> out[4], d2(n);
  for (auto& a : out) a.resize(3 * n);
  std::vector<uint32_t> js(n), fw(n), st(n);
  std::vector<uint8_t> fl(n);
  uint32_t iters = 0;
  unsigned long long sum = 0;
  for (int with_dd2 = 0; with_dd2 < 2; ++with_dd2) {
    target_raygrad_host_backtrace_rays(rif.data(), c.hd, n, pos.data(), vel.data(), tg.data(), dx.data(), dv.data(),
                                       with_dd2 ? dd2.data() : nullptr, c.h, c.ds, out[0].data(), out[1].data(),
                                       out[2].data(), out[3].data(), d2.data(), js.data(), fw.data(), st.data(), fl.data(),
                                       &iters);
    for (size_t i = 0; i < n; ++i) sum += st[i] + js[i] + fl[i];
  }
  return finished("%zu rays, global loop %u, checksum %llu", n, iters, sum);
}
#endif
