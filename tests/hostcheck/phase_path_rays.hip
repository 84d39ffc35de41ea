// phase_path_rays.hip -- TEST INFRASTRUCTURE ONLY (never built or loaded by the package).
//
// The host build of trace_phase_ray and phase_backtrace_ray of adjointnonlinearraytracing_amd/csrc/drrt_device.h (ray paths
// with velocities), looped as drrt_integral.hip launches them: the exports name their taps, stores, seeds and sink and the
// one call per ray, the loops are host_common.h's.  Compiled by tests/phase_path_host.py with the line of
// tests/hostcheck_lib.py: the CPU tier compares it with the host build of the path routines (integral_rays.hip) and with
// float64 autograd (tests/phase_path_ad.py), the GPU tier compares the kernels with it.  The grid gradient is summed in
// double here, in ray order.
//
// With -DPHASE_MAIN it is a stand-alone program (its own main, nothing preloaded) for a build under AddressSanitizer +
// UndefinedBehaviorSanitizer: argv[1] names a file with one case (see main), both routines run on it, 0 = no report.
#include "host_common.h"

// stride, samples >= 1.  xt, vt: (n,3); path, vpath: (samples, n, 3); count, steps: n; *n_failed as in drrt_stats
EXPORT int phase_host_trace(const float* rif, const int* res, size_t n, const float* pos, const float* vel, float h, float ds,
                            int stride, int samples, float* xt, float* vt, float* path, float* vpath, int32_t* count,
                            uint32_t* steps, long long* n_failed) {
  if (stride < 1 || samples < 1) return 1;
  const Vol V = vol(rif, res, h);
  const int max_steps = max_steps_of(res, h, ds);
  const GridTaps taps{rif};
  return trace_rays(n, pos, vel, xt, vt, steps, n_failed, [&](size_t i, const float* p, const float* v) {
    auto store = [&](unsigned j, float x, float y, float z, float vx, float vy, float vz) {
      const size_t e = ((size_t)j * n + i) * 3;
      path[e] = x; path[e + 1] = y; path[e + 2] = z;
      vpath[e] = vx; vpath[e + 1] = vy; vpath[e + 2] = vz;
    };
    unsigned cnt = 0;
    const RayOut r = trace_phase_ray(V, ds, max_steps, p, v, (unsigned)stride, (unsigned)samples, taps, store, cnt);
    count[i] = (int32_t)cnt;
    return r;
  });
}

// dx, dv, dpath, dvpath: nullable (zeros; a null dvpath is no seed at all).  grad: double[nvox], zeroed here.  dpos, dvel:
// (n,3); rsteps (reverse iterations), failed: n each.
EXPORT int phase_host_backtrace(const float* rif, const int* res, size_t n, const float* pos, const float* vel,
                                const float* xt, const float* vt, const uint32_t* fsteps, const float* dx, const float* dv,
                                const float* dpath, const float* dvpath, float h, float ds, int stride, int samples,
                                int corrected_h, double* grad, float* dpos, float* dvel, uint32_t* rsteps, uint8_t* failed) {
  if (stride < 1 || samples < 1) return 1;
  const Vol V = vol(rif, res, h);
  const int max_steps = max_steps_of(res, h, ds);
  const float grad_scale = corrected_h ? V.inv_h : 1.0f;
  const GridTaps taps{rif};
  const SplatSink sink = zeroed<SplatSink>(grad, (size_t)res[0] * res[1] * res[2]);
  const float zero[3] = {0.f, 0.f, 0.f};
  return backtrace_rays(n, dx, dv, dpos, dvel, rsteps, failed, [&](size_t i, const float* gx, const float* gv) {
    auto seed = [&](unsigned j, float* g) {
      const float* q = dpath ? dpath + ((size_t)j * n + i) * 3 : zero;
      g[0] = q[0]; g[1] = q[1]; g[2] = q[2];
    };
    auto vseed = [&](unsigned j, float* g) {
      if (!dvpath) return false;
      const float* q = dvpath + ((size_t)j * n + i) * 3;
      g[0] = q[0]; g[1] = q[1]; g[2] = q[2];
      return true;
    };
    return phase_backtrace_ray(V, ds, grad_scale, max_steps, fsteps[i], pos + 3 * i, vel + 3 * i, xt + 3 * i, vt + 3 * i, gx,
                               gv, (unsigned)stride, (unsigned)samples, seed, vseed, taps, sink);
  });
}

#ifdef PHASE_MAIN
// The case file: int32 W, H, D, n, stride, samples; float32 h, ds; then float32 arrays rif[W*H*D], pos, vel, dx, dv (n*3
// each), dpath, dvpath (samples*n*3 each).  n = 0 is a case.
int main(int argc, char** argv) {
  CaseFile c(argc, argv, 6);
  const size_t n = c.n, m = (size_t)c.hd[5];
  const std::vector<float> rif = c.floats(c.nvox), pos = c.floats(3 * n), vel = c.floats(3 * n), dx = c.floats(3 * n),
                           dv = c.floats(3 * n), dpath = c.floats(m * n * 3), dvpath = c.floats(m * n * 3);
  if (!c.ok) return 2;
  RayRun o(n);
  std::vector<float> path(m * n * 3), vpath(m * n * 3);
  std::vector<int32_t> cnt(n);
  std::vector<double> grad(c.nvox);
  if (phase_host_trace(rif.data(), c.hd, n, pos.data(), vel.data(), c.h, c.ds, c.hd[4], c.hd[5], o.xt.data(), o.vt.data(),
                       path.data(), vpath.data(), cnt.data(), o.st.data(), &o.nf)) return 2;
  o.three_passes([&](int pass) {               // all seeds, flag on; no seeds on the rays or path, flag off; no dvpath
    phase_host_backtrace(rif.data(), c.hd, n, pos.data(), vel.data(), o.xt.data(), o.vt.data(), o.st.data(),
                         pass == 1 ? nullptr : dx.data(), pass == 1 ? nullptr : dv.data(),
                         pass == 1 ? nullptr : dpath.data(), pass == 2 ? nullptr : dvpath.data(), c.h, c.ds, c.hd[4],
                         c.hd[5], pass != 1, grad.data(), o.dpos.data(), o.dvel.data(), o.rs.data(), o.fl.data());
  });
  for (size_t i = 0; i < n; ++i) o.sum += (unsigned)cnt[i];
  return finished("%zu rays, %lld failed, checksum %llu", n, o.nf, o.sum);
}
#endif
