// integral_rays.hip -- TEST INFRASTRUCTURE ONLY (never built or loaded by the package).
//
// The host build of the routines of the integral operators -- optical path length (trace_opl_ray, opl_backtrace_ray), line
// integral of a second field (trace_field_ray, field_backtrace_ray) and emission with self-absorption (exp_neg,
// trace_emission_ray, emission_backtrace_ray) of adjointnonlinearraytracing_amd/csrc/drrt_device.h -- looped as
// drrt_integral.hip launches them.  Compiled by tests/integral_host.py with the line of tests/hostcheck_lib.py (`hipcc
// --cuda-host-only -O2 -ffp-contract=off -mfma`): the CPU tier compares it with float64 autograd (tests/opl_ad.py,
// field_ad.py, emission_ad.py), the GPU tier compares the kernels with it.  Every grid gradient is summed in double here
// (the kernels sum fp32 atomics in another order anyway), and the two parts of a contribution to dL/dn -- the value weights
// and the gradient splat that DRRT_FLAG_CORRECTED_H scales -- can be had separately (`parts`); a contribution to a further
// grid (dL/dfield, dL/de, dL/da) has value weights only, so `parts` = 2 leaves those grids zero.
//
// With -DOPL_MAIN, -DFIELD_MAIN or -DEMISSION_MAIN it is a stand-alone program (its own main, nothing preloaded) for a
// build under AddressSanitizer + UndefinedBehaviorSanitizer: argv[1] names a file with one case of that operator (see its
// main), all its routines run on it, 0 = no report.
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

// ---- optical path length ---------------------------------------------------------------------------------------------
// xt, vt: (n,3); opl, steps: n; *n_failed as in drrt_stats
EXPORT int opl_host_trace(const float* rif, const int* res, size_t n, const float* pos, const float* vel, float h, float ds,
                          float* xt, float* vt, float* opl, uint32_t* steps, long long* n_failed) {
  const Vol V = vol(rif, res, h);
  const int max_steps = max_steps_of(res, h, ds);
  auto taps = [&](const Cell& c) -> Taps { return fetch(V.data, c); };
  long long nf = 0;
  for (size_t i = 0; i < n; ++i) {
    const RayOut r = trace_opl_ray(V, ds, max_steps, pos + 3 * i, vel + 3 * i, taps, opl[i]);
    for (int k = 0; k < 3; ++k) { xt[3 * i + k] = r.xt[k]; vt[3 * i + k] = r.vt[k]; }
    steps[i] = r.steps;
    nf += r.act ? 1 : 0;
  }
  *n_failed = nf;
  return 0;
}

// dx, dv, dopl: nullable (zeros).  grad: double[nvox], zeroed here.  parts: 0 = the whole contribution, 1 = its value
// weights alone, 2 = its gradient splat alone.  dpos, dvel: (n,3); rsteps (reverse iterations), failed: n each.
EXPORT int opl_host_backtrace(const float* rif, const int* res, size_t n, const float* pos, const float* vel,
                              const float* xt, const float* vt, const uint32_t* fsteps, const float* dx, const float* dv,
                              const float* dopl, float h, float ds, int corrected_h, int parts, double* grad, float* dpos,
                              float* dvel, uint32_t* rsteps, uint8_t* failed) {
  const Vol V = vol(rif, res, h);
  const int max_steps = max_steps_of(res, h, ds);
  const float grad_scale = corrected_h ? V.inv_h : 1.0f;
  const size_t nvox = (size_t)res[0] * res[1] * res[2];
  for (size_t k = 0; k < nvox; ++k) grad[k] = 0.0;
  auto taps = [&](const Cell& c) -> Taps { return fetch(V.data, c); };
  auto sink = [&](const Cell& c, float val, float gx, float gy, float gz) {
    if (parts == 1) gx = gy = gz = 0.f;
    if (parts == 2) val = 0.f;
    add_corners(grad, c, splat_weights(c.wx, c.wy, c.wz, val, gx, gy, gz));
  };
  const float zero[3] = {0.f, 0.f, 0.f};
  for (size_t i = 0; i < n; ++i) {
    const RayGrad r = opl_backtrace_ray(V, ds, grad_scale, max_steps, fsteps[i], pos + 3 * i, vel + 3 * i, xt + 3 * i,
                                        vt + 3 * i, dx ? dx + 3 * i : zero, dv ? dv + 3 * i : zero, dopl ? dopl[i] : 0.f,
                                        taps, sink);
    for (int k = 0; k < 3; ++k) { dpos[3 * i + k] = r.dp[k]; dvel[3 * i + k] = r.dv[k]; }
    rsteps[i] = r.steps; failed[i] = r.failed ? 1 : 0;
  }
  return 0;
}

#ifdef OPL_MAIN
// The case file: int32 W, H, D, n; float32 h, ds; then float32 arrays rif[W*H*D], pos, vel, dx, dv (n*3 each), dopl[n].
int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  int hd[4]; float sc[2];
  if (fread(hd, sizeof(int), 4, f) != 4 || fread(sc, sizeof(float), 2, f) != 2) return 2;
  if (hd[0] < 1 || hd[1] < 1 || hd[2] < 1 || hd[3] < 0) return 2;
  const size_t nvox = (size_t)hd[0] * hd[1] * hd[2], n = (size_t)hd[3];
  std::vector<float> rif(nvox), ray[4], dopl(n);
  bool ok = fread(rif.data(), sizeof(float), nvox, f) == nvox;
  for (auto& a : ray) { a.resize(3 * n); ok = ok && fread(a.data(), sizeof(float), 3 * n, f) == 3 * n; }
  ok = ok && fread(dopl.data(), sizeof(float), n, f) == n;
  fclose(f);
  if (!ok) return 2;
  std::vector<float> out[4], opl(n);
  for (auto& a : out) a.resize(3 * n);
  std::vector<uint32_t> st(n), rs(n);
  std::vector<uint8_t> fl(n);
  std::vector<double> grad(nvox);
  const int res[3] = {hd[0], hd[1], hd[2]};
  long long nf = 0;
  unsigned long long sum = 0;
  opl_host_trace(rif.data(), res, n, ray[0].data(), ray[1].data(), sc[0], sc[1], out[0].data(), out[1].data(), opl.data(),
                 st.data(), &nf);
  for (int pass = 0; pass < 3; ++pass) {                  // all seeds, flag on; no seeds on the rays, flag off, one part
    opl_host_backtrace(rif.data(), res, n, ray[0].data(), ray[1].data(), out[0].data(), out[1].data(), st.data(),
                       pass == 1 ? nullptr : ray[2].data(), pass == 1 ? nullptr : ray[3].data(),
                       pass == 2 ? nullptr : dopl.data(), sc[0], sc[1], pass != 1, pass, grad.data(), out[2].data(),
                       out[3].data(), rs.data(), fl.data());
    for (size_t i = 0; i < n; ++i) sum += rs[i] + fl[i];
  }
  for (size_t i = 0; i < n; ++i) sum += st[i];
  printf("%zu rays, %lld failed, checksum %llu\nsanitizer run finished without reports\n", n, nf, sum);
  return 0;
}
#endif

// ---- line integral of a second field -----------------------------------------------------------------------------------
// xt, vt: (n,3); tau, steps: n; *n_failed as in drrt_stats
EXPORT int field_host_trace(const float* rif, const float* field, const int* res, size_t n, const float* pos,
                            const float* vel, float h, float ds, float* xt, float* vt, float* tau, uint32_t* steps,
                            long long* n_failed) {
  const Vol V = vol(rif, res, h);
  const int max_steps = max_steps_of(res, h, ds);
  auto taps = [&](const Cell& c) -> Taps { return fetch(V.data, c); };
  auto ftaps = [&](const Cell& c) -> Taps { return fetch(field, c); };
  long long nf = 0;
  for (size_t i = 0; i < n; ++i) {
    const RayOut r = trace_field_ray(V, ds, max_steps, pos + 3 * i, vel + 3 * i, taps, ftaps, tau[i]);
    for (int k = 0; k < 3; ++k) { xt[3 * i + k] = r.xt[k]; vt[3 * i + k] = r.vt[k]; }
    steps[i] = r.steps;
    nf += r.act ? 1 : 0;
  }
  *n_failed = nf;
  return 0;
}

// dx, dv, dtau: nullable (zeros).  grad, grad_field: double[nvox], zeroed here.  parts: 0 = the whole contribution, 1 = its
// value weights alone, 2 = its gradient splat alone.  dpos, dvel: (n,3); rsteps (reverse iterations), failed: n each.
EXPORT int field_host_backtrace(const float* rif, const float* field, const int* res, size_t n, const float* pos,
                                const float* vel, const float* xt, const float* vt, const uint32_t* fsteps, const float* dx,
                                const float* dv, const float* dtau, float h, float ds, int corrected_h, int parts,
                                double* grad, double* grad_field, float* dpos, float* dvel, uint32_t* rsteps,
                                uint8_t* failed) {
  const Vol V = vol(rif, res, h);
  const int max_steps = max_steps_of(res, h, ds);
  const float grad_scale = corrected_h ? V.inv_h : 1.0f;
  const size_t nvox = (size_t)res[0] * res[1] * res[2];
  for (size_t k = 0; k < nvox; ++k) grad[k] = grad_field[k] = 0.0;
  auto taps = [&](const Cell& c) -> Taps { return fetch(V.data, c); };
  auto ftaps = [&](const Cell& c) -> Taps { return fetch(field, c); };
  auto sink = [&](const Cell& c, float val, float gx, float gy, float gz) {
    if (parts == 1) gx = gy = gz = 0.f;
    if (parts == 2) val = 0.f;
    add_corners(grad, c, splat_weights(c.wx, c.wy, c.wz, val, gx, gy, gz));
  };
  auto fsink = [&](const Cell& c, float val) {
    if (parts != 2) add_corners(grad_field, c, value_weights(c.wx, c.wy, c.wz, val));
  };
  const float zero[3] = {0.f, 0.f, 0.f};
  for (size_t i = 0; i < n; ++i) {
    const RayGrad r = field_backtrace_ray(V, ds, grad_scale, max_steps, fsteps[i], pos + 3 * i, vel + 3 * i, xt + 3 * i,
                                          vt + 3 * i, dx ? dx + 3 * i : zero, dv ? dv + 3 * i : zero, dtau ? dtau[i] : 0.f,
                                          taps, ftaps, sink, fsink);
    for (int k = 0; k < 3; ++k) { dpos[3 * i + k] = r.dp[k]; dvel[3 * i + k] = r.dv[k]; }
    rsteps[i] = r.steps; failed[i] = r.failed ? 1 : 0;
  }
  return 0;
}

#ifdef FIELD_MAIN
// The case file: int32 W, H, D, n; float32 h, ds; then float32 arrays rif[W*H*D], field[W*H*D], pos, vel, dx, dv (n*3 each),
// dtau[n].
int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  int hd[4]; float sc[2];
  if (fread(hd, sizeof(int), 4, f) != 4 || fread(sc, sizeof(float), 2, f) != 2) return 2;
  if (hd[0] < 1 || hd[1] < 1 || hd[2] < 1 || hd[3] < 0) return 2;
  const size_t nvox = (size_t)hd[0] * hd[1] * hd[2], n = (size_t)hd[3];
  std::vector<float> rif(nvox), field(nvox), ray[4], dtau(n);
  bool ok = fread(rif.data(), sizeof(float), nvox, f) == nvox && fread(field.data(), sizeof(float), nvox, f) == nvox;
  for (auto& a : ray) { a.resize(3 * n); ok = ok && fread(a.data(), sizeof(float), 3 * n, f) == 3 * n; }
  ok = ok && fread(dtau.data(), sizeof(float), n, f) == n;
  fclose(f);
  if (!ok) return 2;
  std::vector<float> out[4], tau(n);
  for (auto& a : out) a.resize(3 * n);
  std::vector<uint32_t> st(n), rs(n);
  std::vector<uint8_t> fl(n);
  std::vector<double> grad(nvox), gfield(nvox);
  const int res[3] = {hd[0], hd[1], hd[2]};
  long long nf = 0;
  unsigned long long sum = 0;
  field_host_trace(rif.data(), field.data(), res, n, ray[0].data(), ray[1].data(), sc[0], sc[1], out[0].data(),
                   out[1].data(), tau.data(), st.data(), &nf);
  for (int pass = 0; pass < 3; ++pass) {                  // all seeds, flag on; no seeds on the rays, flag off, one part
    field_host_backtrace(rif.data(), field.data(), res, n, ray[0].data(), ray[1].data(), out[0].data(), out[1].data(),
                         st.data(), pass == 1 ? nullptr : ray[2].data(), pass == 1 ? nullptr : ray[3].data(),
                         pass == 2 ? nullptr : dtau.data(), sc[0], sc[1], pass != 1, pass, grad.data(), gfield.data(),
                         out[2].data(), out[3].data(), rs.data(), fl.data());
    for (size_t i = 0; i < n; ++i) sum += rs[i] + fl[i];
  }
  for (size_t i = 0; i < n; ++i) sum += st[i];
  printf("%zu rays, %lld failed, checksum %llu\nsanitizer run finished without reports\n", n, nf, sum);
  return 0;
}
#endif

// ---- emission with self-absorption -----------------------------------------------------------------------------------
// out[i] = exp_neg(t[i])
EXPORT int emission_host_exp_neg(const float* t, size_t n, float* out) {
  for (size_t i = 0; i < n; ++i) out[i] = exp_neg(t[i]);
  return 0;
}

// xt, vt: (n,3); rad, tau, steps: n; *n_failed as in drrt_stats
EXPORT int emission_host_trace(const float* rif, const float* emis, const float* absb, const int* res, size_t n,
                               const float* pos, const float* vel, float h, float ds, float* xt, float* vt, float* rad,
                               float* tau, uint32_t* steps, long long* n_failed) {
  const Vol V = vol(rif, res, h);
  const int max_steps = max_steps_of(res, h, ds);
  auto taps = [&](const Cell& c) -> Taps { return fetch(V.data, c); };
  auto etaps = [&](const Cell& c) -> Taps { return fetch(emis, c); };
  auto ataps = [&](const Cell& c) -> Taps { return fetch(absb, c); };
  long long nf = 0;
  for (size_t i = 0; i < n; ++i) {
    const RayOut r = trace_emission_ray(V, ds, max_steps, pos + 3 * i, vel + 3 * i, taps, etaps, ataps, rad[i], tau[i]);
    for (int k = 0; k < 3; ++k) { xt[3 * i + k] = r.xt[k]; vt[3 * i + k] = r.vt[k]; }
    steps[i] = r.steps;
    nf += r.act ? 1 : 0;
  }
  *n_failed = nf;
  return 0;
}

// tau: the forward's.  dx, dv, drad, dtau: nullable (zeros).  grad, grad_e, grad_a: double[nvox], zeroed here.  parts: 0 =
// the whole contribution, 1 = its value weights alone, 2 = its gradient splat alone.  dpos, dvel: (n,3); rsteps (reverse
// iterations), failed: n each.
EXPORT int emission_host_backtrace(const float* rif, const float* emis, const float* absb, const int* res, size_t n,
                                   const float* pos, const float* vel, const float* xt, const float* vt,
                                   const uint32_t* fsteps, const float* tau, const float* dx, const float* dv,
                                   const float* drad, const float* dtau, float h, float ds, int corrected_h, int parts,
                                   double* grad, double* grad_e, double* grad_a, float* dpos, float* dvel, uint32_t* rsteps,
                                   uint8_t* failed) {
  const Vol V = vol(rif, res, h);
  const int max_steps = max_steps_of(res, h, ds);
  const float grad_scale = corrected_h ? V.inv_h : 1.0f;
  const size_t nvox = (size_t)res[0] * res[1] * res[2];
  for (size_t k = 0; k < nvox; ++k) grad[k] = grad_e[k] = grad_a[k] = 0.0;
  auto taps = [&](const Cell& c) -> Taps { return fetch(V.data, c); };
  auto etaps = [&](const Cell& c) -> Taps { return fetch(emis, c); };
  auto ataps = [&](const Cell& c) -> Taps { return fetch(absb, c); };
  auto sink = [&](const Cell& c, float val, float gx, float gy, float gz) {
    if (parts == 1) gx = gy = gz = 0.f;
    if (parts == 2) val = 0.f;
    add_corners(grad, c, splat_weights(c.wx, c.wy, c.wz, val, gx, gy, gz));
  };
  auto esink = [&](const Cell& c, float val) {
    if (parts != 2) add_corners(grad_e, c, value_weights(c.wx, c.wy, c.wz, val));
  };
  auto asink = [&](const Cell& c, float val) {
    if (parts != 2) add_corners(grad_a, c, value_weights(c.wx, c.wy, c.wz, val));
  };
  const float zero[3] = {0.f, 0.f, 0.f};
  for (size_t i = 0; i < n; ++i) {
    const RayGrad r = emission_backtrace_ray(V, ds, grad_scale, max_steps, fsteps[i], pos + 3 * i, vel + 3 * i, xt + 3 * i,
                                             vt + 3 * i, tau[i], dx ? dx + 3 * i : zero, dv ? dv + 3 * i : zero,
                                             drad ? drad[i] : 0.f, dtau ? dtau[i] : 0.f, taps, etaps, ataps, sink, esink,
                                             asink);
    for (int k = 0; k < 3; ++k) { dpos[3 * i + k] = r.dp[k]; dvel[3 * i + k] = r.dv[k]; }
    rsteps[i] = r.steps; failed[i] = r.failed ? 1 : 0;
  }
  return 0;
}

#ifdef EMISSION_MAIN
// The case file: int32 W, H, D, n; float32 h, ds; then float32 arrays rif[W*H*D], emission[W*H*D], absorption[W*H*D], pos,
// vel, dx, dv (n*3 each), drad[n], dtau[n].
int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  int hd[4]; float sc[2];
  if (fread(hd, sizeof(int), 4, f) != 4 || fread(sc, sizeof(float), 2, f) != 2) return 2;
  if (hd[0] < 1 || hd[1] < 1 || hd[2] < 1 || hd[3] < 0) return 2;
  const size_t nvox = (size_t)hd[0] * hd[1] * hd[2], n = (size_t)hd[3];
  std::vector<float> grid[3], ray[4], seed[2];
  bool ok = true;
  for (auto& a : grid) { a.resize(nvox); ok = ok && fread(a.data(), sizeof(float), nvox, f) == nvox; }
  for (auto& a : ray) { a.resize(3 * n); ok = ok && fread(a.data(), sizeof(float), 3 * n, f) == 3 * n; }
  for (auto& a : seed) { a.resize(n); ok = ok && fread(a.data(), sizeof(float), n, f) == n; }
  fclose(f);
  if (!ok) return 2;
  std::vector<float> out[4], rad(n), tau(n), ex(n);
  for (auto& a : out) a.resize(3 * n);
  std::vector<uint32_t> st(n), rs(n);
  std::vector<uint8_t> fl(n);
  std::vector<double> grad(nvox), ge(nvox), ga(nvox);
  const int res[3] = {hd[0], hd[1], hd[2]};
  long long nf = 0;
  unsigned long long sum = 0;
  emission_host_exp_neg(seed[1].data(), n, ex.data());     // the seeds on tau carry NaN, +-Inf, +-3e38 and denormals
  const float edge[8] = {0.f, -0.f, 87.f, -87.f, 88.f, -88.f, 1e-40f, -1e-40f};
  float eout[8];
  emission_host_exp_neg(edge, 8, eout);
  emission_host_trace(grid[0].data(), grid[1].data(), grid[2].data(), res, n, ray[0].data(), ray[1].data(), sc[0], sc[1],
                      out[0].data(), out[1].data(), rad.data(), tau.data(), st.data(), &nf);
  for (int pass = 0; pass < 3; ++pass) {                  // all seeds, flag on; no seeds on the rays, flag off, one part
    emission_host_backtrace(grid[0].data(), grid[1].data(), grid[2].data(), res, n, ray[0].data(), ray[1].data(),
                            out[0].data(), out[1].data(), st.data(), tau.data(), pass == 1 ? nullptr : ray[2].data(),
                            pass == 1 ? nullptr : ray[3].data(), seed[0].data(), pass == 2 ? nullptr : seed[1].data(), sc[0],
                            sc[1], pass != 1, pass, grad.data(), ge.data(), ga.data(), out[2].data(), out[3].data(), rs.data(),
                            fl.data());
    for (size_t i = 0; i < n; ++i) sum += rs[i] + fl[i];
  }
  for (size_t i = 0; i < n; ++i) sum += st[i];
  printf("%zu rays, %lld failed, checksum %llu, exp_neg(0) %.9g\nsanitizer run finished without reports\n", n, nf, sum,
         (double)eout[0]);
  return 0;
}
#endif
