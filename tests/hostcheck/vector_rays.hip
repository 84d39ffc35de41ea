// vector_rays.hip -- TEST INFRASTRUCTURE ONLY (never built or loaded by the package).
//
// The host build of the routines of the line integral of a vector field (trace_vector_ray, vector_backtrace_ray of
// adjointnonlinearraytracing_amd/csrc/drrt_device.h), looped as drrt_integral.hip launches them.  Compiled by
// tests/vector_host.py with the line of tests/hostcheck_lib.py (`hipcc --cuda-host-only -O2 -ffp-contract=off -mfma`): the
// CPU tier compares it with float64 autograd (tests/vector_ad.py), the GPU tier compares the kernels with it.  Every grid
// gradient is summed in double here (the kernels sum fp32 atomics in another order anyway), and the two parts of a
// contribution to dL/dn -- the value weights and the gradient splat that DRRT_FLAG_CORRECTED_H scales -- can be had
// separately (`parts`); a contribution to a plane of dL/du has value weights only, so `parts` = 2 leaves those planes zero.
//
// With -DVECTOR_MAIN it is a stand-alone program (its own main, nothing preloaded) for a build under AddressSanitizer +
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

// vfield: 3 nvox floats, plane c at + c nvox.  xt, vt: (n,3); circ, steps: n; *n_failed as in drrt_stats
EXPORT int vector_host_trace(const float* rif, const float* vfield, const int* res, size_t n, const float* pos,
                             const float* vel, float h, float ds, float* xt, float* vt, float* circ, uint32_t* steps,
                             long long* n_failed) {
  const Vol V = vol(rif, res, h);
  const int max_steps = max_steps_of(res, h, ds);
  const size_t nvox = (size_t)res[0] * res[1] * res[2];
  auto taps = [&](const Cell& c) -> Taps { return fetch(V.data, c); };
  auto vtaps = [&](const Cell& c, int k) -> Taps { return fetch(vfield + (size_t)k * nvox, c); };
  long long nf = 0;
  for (size_t i = 0; i < n; ++i) {
    const RayOut r = trace_vector_ray(V, ds, max_steps, pos + 3 * i, vel + 3 * i, taps, vtaps, circ[i]);
    for (int k = 0; k < 3; ++k) { xt[3 * i + k] = r.xt[k]; vt[3 * i + k] = r.vt[k]; }
    steps[i] = r.steps;
    nf += r.act ? 1 : 0;
  }
  *n_failed = nf;
  return 0;
}

// dx, dv, dcirc: nullable (zeros).  grad: double[nvox], grad_vfield: double[3 nvox], zeroed here.  parts: 0 = the whole
// contribution, 1 = its value weights alone, 2 = its gradient splat alone.  dpos, dvel: (n,3); rsteps (reverse iterations),
// failed: n each.
EXPORT int vector_host_backtrace(const float* rif, const float* vfield, const int* res, size_t n, const float* pos,
                                 const float* vel, const float* xt, const float* vt, const uint32_t* fsteps,
                                 const float* dx, const float* dv, const float* dcirc, float h, float ds, int corrected_h,
                                 int parts, double* grad, double* grad_vfield, float* dpos, float* dvel, uint32_t* rsteps,
                                 uint8_t* failed) {
  const Vol V = vol(rif, res, h);
  const int max_steps = max_steps_of(res, h, ds);
  const float grad_scale = corrected_h ? V.inv_h : 1.0f;
  const size_t nvox = (size_t)res[0] * res[1] * res[2];
  for (size_t k = 0; k < nvox; ++k) grad[k] = 0.0;
  for (size_t k = 0; k < 3 * nvox; ++k) grad_vfield[k] = 0.0;
  auto taps = [&](const Cell& c) -> Taps { return fetch(V.data, c); };
  auto vtaps = [&](const Cell& c, int k) -> Taps { return fetch(vfield + (size_t)k * nvox, c); };
  auto sink = [&](const Cell& c, float val, float gx, float gy, float gz) {
    if (parts == 1) gx = gy = gz = 0.f;
    if (parts == 2) val = 0.f;
    add_corners(grad, c, splat_weights(c.wx, c.wy, c.wz, val, gx, gy, gz));
  };
  auto vsink = [&](int k, const Cell& c, float val) {
    if (parts != 2) add_corners(grad_vfield + (size_t)k * nvox, c, value_weights(c.wx, c.wy, c.wz, val));
  };
  const float zero[3] = {0.f, 0.f, 0.f};
  for (size_t i = 0; i < n; ++i) {
    const RayGrad r = vector_backtrace_ray(V, ds, grad_scale, max_steps, fsteps[i], pos + 3 * i, vel + 3 * i, xt + 3 * i,
                                           vt + 3 * i, dx ? dx + 3 * i : zero, dv ? dv + 3 * i : zero,
                                           dcirc ? dcirc[i] : 0.f, taps, vtaps, sink, vsink);
    for (int k = 0; k < 3; ++k) { dpos[3 * i + k] = r.dp[k]; dvel[3 * i + k] = r.dv[k]; }
    rsteps[i] = r.steps; failed[i] = r.failed ? 1 : 0;
  }
  return 0;
}

#ifdef VECTOR_MAIN
// The case file: int32 W, H, D, n; float32 h, ds; then float32 arrays rif[W*H*D], vfield[3*W*H*D], pos, vel, dx, dv (n*3
// each), dcirc[n].
int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  int hd[4]; float sc[2];
  if (fread(hd, sizeof(int), 4, f) != 4 || fread(sc, sizeof(float), 2, f) != 2) return 2;
  if (hd[0] < 1 || hd[1] < 1 || hd[2] < 1 || hd[3] < 0) return 2;
  const size_t nvox = (size_t)hd[0] * hd[1] * hd[2], n = (size_t)hd[3];
  std::vector<float> rif(nvox), vfield(3 * nvox), ray[4], dcirc(n);
  bool ok = fread(rif.data(), sizeof(float), nvox, f) == nvox && fread(vfield.data(), sizeof(float), 3 * nvox, f) == 3 * nvox;
  for (auto& a : ray) { a.resize(3 * n); ok = ok && fread(a.data(), sizeof(float), 3 * n, f) == 3 * n; }
  ok = ok && fread(dcirc.data(), sizeof(float), n, f) == n;
  fclose(f);
  if (!ok) return 2;
  std::vector<float> out[4], circ(n);
  for (auto& a : out) a.resize(3 * n);
  std::vector<uint32_t> st(n), rs(n);
  std::vector<uint8_t> fl(n);
  std::vector<double> grad(nvox), gv(3 * nvox);
  const int res[3] = {hd[0], hd[1], hd[2]};
  long long nf = 0;
  unsigned long long sum = 0;
  vector_host_trace(rif.data(), vfield.data(), res, n, ray[0].data(), ray[1].data(), sc[0], sc[1], out[0].data(),
                    out[1].data(), circ.data(), st.data(), &nf);
  for (int pass = 0; pass < 3; ++pass) {                  // all seeds, flag on; no seeds on the rays, flag off, one part
    vector_host_backtrace(rif.data(), vfield.data(), res, n, ray[0].data(), ray[1].data(), out[0].data(), out[1].data(),
                          st.data(), pass == 1 ? nullptr : ray[2].data(), pass == 1 ? nullptr : ray[3].data(),
                          pass == 2 ? nullptr : dcirc.data(), sc[0], sc[1], pass != 1, pass, grad.data(), gv.data(),
                          out[2].data(), out[3].data(), rs.data(), fl.data());
    for (size_t i = 0; i < n; ++i) sum += rs[i] + fl[i];
  }
  for (size_t i = 0; i < n; ++i) sum += st[i];
  printf("%zu rays, %lld failed, checksum %llu\nsanitizer run finished without reports\n", n, nf, sum);
  return 0;
}
#endif
