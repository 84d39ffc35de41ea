// path_rays.hip -- TEST INFRASTRUCTURE ONLY (never built or loaded by the package).
//
// The host build of the routines of the ray-path operator (trace_path_ray, path_backtrace_ray of
// adjointnonlinearraytracing_amd/csrc/drrt_device.h), looped as drrt_integral.hip launches them.  Compiled by
// tests/path_host.py with the line of tests/hostcheck_lib.py (`hipcc --cuda-host-only -O2 -ffp-contract=off -mfma`): the
// CPU tier compares it with float64 autograd (tests/path_ad.py), the GPU tier compares the kernels with it.  The grid
// gradient is summed in double here (the kernels sum fp32 atomics in another order anyway).
//
// With -DPATH_MAIN it is a stand-alone program (its own main, nothing preloaded) for a build under AddressSanitizer +
// UndefinedBehaviorSanitizer: argv[1] names a file with one case (see main), both routines run on it, 0 = no report.
#include <stdint.h>
#include <stddef.h>
#include <stdio.h>

#include <vector>

#include "../../adjointnonlinearraytracing_amd/csrc/drrt_device.h"

using namespace drrt;

#define EXPORT extern "C" __attribute__((visibility("default")))

static Vol vol(const float* rif, const int* res, float h) {
  Vol V;
  V.data = rif; V.W = res[0]; V.H = res[1]; V.D = res[2];
  vol_finish(V, h);
  return V;
}
static int max_steps_of(const int* res, float h, float ds) {             // the forward's bound (drrt_api.hip steps_fwd)
  const int mx = res[0] > res[1] ? (res[0] > res[2] ? res[0] : res[2]) : (res[1] > res[2] ? res[1] : res[2]);
  return (int)(4.0f * h * (float)mx / ds);
}
static void add_corners(double* grad, const Cell& c, const Corners& w) {
  double* g = grad + c.base;
  g[0] += w.c000;            g[c.ox] += w.c100;
  g[c.oy] += w.c010;         g[c.oy + c.ox] += w.c110;
  g[c.oz] += w.c001;         g[c.oz + c.ox] += w.c101;
  g[c.oz + c.oy] += w.c011;  g[c.oz + c.oy + c.ox] += w.c111;
}

// stride, samples >= 1.  xt, vt: (n,3); path: (samples, n, 3); count, steps: n; *n_failed as in drrt_stats
EXPORT int path_host_trace(const float* rif, const int* res, size_t n, const float* pos, const float* vel, float h, float ds,
                           int stride, int samples, float* xt, float* vt, float* path, int32_t* count, uint32_t* steps,
                           long long* n_failed) {
  if (stride < 1 || samples < 1) return 1;
  const Vol V = vol(rif, res, h);
  const int max_steps = max_steps_of(res, h, ds);
  auto taps = [&](const Cell& c) -> Taps { return fetch(V.data, c); };
  long long nf = 0;
  for (size_t i = 0; i < n; ++i) {
    auto store = [&](unsigned j, float x, float y, float z) {
      float* q = path + ((size_t)j * n + i) * 3;
      q[0] = x; q[1] = y; q[2] = z;
    };
    unsigned cnt = 0;
    const RayOut r = trace_path_ray(V, ds, max_steps, pos + 3 * i, vel + 3 * i, (unsigned)stride, (unsigned)samples, taps,
                                    store, cnt);
    for (int k = 0; k < 3; ++k) { xt[3 * i + k] = r.xt[k]; vt[3 * i + k] = r.vt[k]; }
    steps[i] = r.steps; count[i] = (int32_t)cnt;
    nf += r.act ? 1 : 0;
  }
  *n_failed = nf;
  return 0;
}

// dx, dv, dpath: nullable (zeros).  grad: double[nvox], zeroed here.  dpos, dvel: (n,3); rsteps (reverse iterations),
// failed: n each.
EXPORT int path_host_backtrace(const float* rif, const int* res, size_t n, const float* pos, const float* vel,
                               const float* xt, const float* vt, const uint32_t* fsteps, const float* dx, const float* dv,
                               const float* dpath, float h, float ds, int stride, int samples, int corrected_h, double* grad,
                               float* dpos, float* dvel, uint32_t* rsteps, uint8_t* failed) {
  if (stride < 1 || samples < 1) return 1;
  const Vol V = vol(rif, res, h);
  const int max_steps = max_steps_of(res, h, ds);
  const float grad_scale = corrected_h ? V.inv_h : 1.0f;
  const size_t nvox = (size_t)res[0] * res[1] * res[2];
  for (size_t k = 0; k < nvox; ++k) grad[k] = 0.0;
  auto taps = [&](const Cell& c) -> Taps { return fetch(V.data, c); };
  auto sink = [&](const Cell& c, float val, float gx, float gy, float gz) {
    add_corners(grad, c, splat_weights(c.wx, c.wy, c.wz, val, gx, gy, gz));
  };
  const float zero[3] = {0.f, 0.f, 0.f};
  for (size_t i = 0; i < n; ++i) {
    auto seed = [&](unsigned j, float* g) {
      const float* q = dpath ? dpath + ((size_t)j * n + i) * 3 : zero;
      g[0] = q[0]; g[1] = q[1]; g[2] = q[2];
    };
    const RayGrad r = path_backtrace_ray(V, ds, grad_scale, max_steps, fsteps[i], pos + 3 * i, vel + 3 * i, xt + 3 * i,
                                         vt + 3 * i, dx ? dx + 3 * i : zero, dv ? dv + 3 * i : zero, (unsigned)stride,
                                         (unsigned)samples, seed, taps, sink);
    for (int k = 0; k < 3; ++k) { dpos[3 * i + k] = r.dp[k]; dvel[3 * i + k] = r.dv[k]; }
    rsteps[i] = r.steps; failed[i] = r.failed ? 1 : 0;
  }
  return 0;
}

#ifdef PATH_MAIN
// The case file: int32 W, H, D, n, stride, samples; float32 h, ds; then float32 arrays rif[W*H*D], pos, vel, dx, dv (n*3
// each), dpath[samples*n*3].  n = 0 is a case.
int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  int hd[6]; float sc[2];
  if (fread(hd, sizeof(int), 6, f) != 6 || fread(sc, sizeof(float), 2, f) != 2) return 2;
  if (hd[0] < 1 || hd[1] < 1 || hd[2] < 1 || hd[3] < 0 || hd[4] < 1 || hd[5] < 1) return 2;
  const size_t nvox = (size_t)hd[0] * hd[1] * hd[2], n = (size_t)hd[3], m = (size_t)hd[5];
  std::vector<float> rif(nvox), ray[4], dpath(m * n * 3);
  bool ok = fread(rif.data(), sizeof(float), nvox, f) == nvox;
  for (auto& a : ray) { a.resize(3 * n); ok = ok && fread(a.data(), sizeof(float), 3 * n, f) == 3 * n; }
  ok = ok && fread(dpath.data(), sizeof(float), dpath.size(), f) == dpath.size();
  fclose(f);
  if (!ok) return 2;
  std::vector<float> out[4], path(m * n * 3);
  for (auto& a : out) a.resize(3 * n);
  std::vector<uint32_t> st(n), rs(n);
  std::vector<int32_t> cnt(n);
  std::vector<uint8_t> fl(n);
  std::vector<double> grad(nvox);
  const int res[3] = {hd[0], hd[1], hd[2]};
  long long nf = 0;
  unsigned long long sum = 0;
  if (path_host_trace(rif.data(), res, n, ray[0].data(), ray[1].data(), sc[0], sc[1], hd[4], hd[5], out[0].data(),
                      out[1].data(), path.data(), cnt.data(), st.data(), &nf)) return 2;
  for (int pass = 0; pass < 3; ++pass) {                  // all seeds, flag on; no seeds on the rays, flag off; no dpath
    path_host_backtrace(rif.data(), res, n, ray[0].data(), ray[1].data(), out[0].data(), out[1].data(), st.data(),
                        pass == 1 ? nullptr : ray[2].data(), pass == 1 ? nullptr : ray[3].data(),
                        pass == 2 ? nullptr : dpath.data(), sc[0], sc[1], hd[4], hd[5], pass != 1, grad.data(), out[2].data(),
                        out[3].data(), rs.data(), fl.data());
    for (size_t i = 0; i < n; ++i) sum += rs[i] + fl[i];
  }
  for (size_t i = 0; i < n; ++i) sum += st[i] + (unsigned)cnt[i];
  printf("%zu rays, %lld failed, checksum %llu\nsanitizer run finished without reports\n", n, nf, sum);
  return 0;
}
#endif
