// hostcheck.hip -- TEST INFRASTRUCTURE ONLY (never built or loaded by the package).
//
// Compiles the product's own per-ray code (adjointnonlinearraytracing_amd/csrc/drrt_device.h,
// the __host__ __device__ step functions and whole-ray drivers the kernels call) for the HOST
// with `hipcc --cuda-host-only -ffp-contract=off`, so that the CPU-only test tier can compare the
// product's arithmetic and control flow with the oracle's `factored` mode bit for bit, without a
// GPU.  The real kernels are exercised by the `-m gpu` tests.
//
// The ray-state adjoints (backtrace_ray_state, cable_backtrace_ray_state, stop_backtrace_ray_state) follow the marches:
// the CPU tier compares them with float64 autograd, the GPU tier compares their kernels with them bit for bit.
#include <stdint.h>
#include <stddef.h>
#include <string.h>

#include <vector>

#include "../../adjointnonlinearraytracing_amd/csrc/drrt_device.h"
#include "../../adjointnonlinearraytracing_amd/csrc/drrt_keys.h"

using namespace drrt;

static Vol make_vol(const float* data, const int res[3], float h) {
  Vol V;
  V.data = data; V.W = res[0]; V.H = res[1]; V.D = res[2];
  vol_finish(V, h);
  return V;
}
static int max3(const int r[3]) { return r[0] > r[1] ? (r[0] > r[2] ? r[0] : r[2]) : (r[1] > r[2] ? r[1] : r[2]); }

#define EXPORT extern "C" __attribute__((visibility("default")))

// mode 0 trace, 1 plane, 2 sdf
EXPORT int hostcheck_trace(int mode, const float* rif, const float* sdf, const int* res, size_t n,
                           const float* pos, const float* vel, const float* pln_o, const float* pln_d,
                           float h, float ds, float* xt, float* vt, uint8_t* failmask, int* steps,
                           long long* n_failed) {
  Vol V = make_vol(rif, res, h);
  int max_steps = (mode == 2) ? (int)(2.0f * h * (float)max3(res) / ds) : (int)(4.0f * h * (float)max3(res) / ds);
  long long nf = 0;
  const float zero[3] = {0, 0, 0};
  unsigned total = 0;
  std::vector<size_t> again;
  for (size_t i = 0; i < n; ++i) {
    const float* po = pln_o ? pln_o + 3 * i : zero; const float* pd = pln_d ? pln_d + 3 * i : zero;
    RayOut r = mode == 0 ? trace_ray<0>(V, sdf, ds, max_steps, pos + 3 * i, vel + 3 * i, po, pd)
             : mode == 1 ? trace_ray<1>(V, sdf, ds, max_steps, pos + 3 * i, vel + 3 * i, po, pd)
                         : trace_ray<2>(V, sdf, ds, max_steps, pos + 3 * i, vel + 3 * i, po, pd);
    memcpy(xt + 3 * i, r.xt, 12); memcpy(vt + 3 * i, r.vt, 12);
    if (failmask) failmask[i] = r.esc ? 0 : 1;
    if (steps) steps[i] = (int)r.steps;
    nf += r.act ? 1 : 0;
    if (r.steps > total) total = r.steps;
    if (r.again) again.push_back(i);
  }
  for (size_t i : again) {                               // k_trace_again
    RayOut r = mode == 1 ? ray_full<1>(V, sdf, ds, total, pos + 3 * i, vel + 3 * i, pln_o + 3 * i, pln_d + 3 * i)
                         : ray_full<2>(V, sdf, ds, total, pos + 3 * i, vel + 3 * i, zero, zero);
    memcpy(xt + 3 * i, r.xt, 12); memcpy(vt + 3 * i, r.vt, 12);
    if (failmask) failmask[i] = r.esc ? 0 : 1;
  }
  if (n_failed) *n_failed = nf;
  return 0;
}

EXPORT int hostcheck_trace_target(const float* rif, const int* res, size_t n, const float* pos, const float* vel,
                                  const float* target, float h, float ds, float* xt, float* vt, float* dist2,
                                  int* iters) {
  Vol V = make_vol(rif, res, h);
  int max_steps = (int)(4.0f * h * (float)max3(res) / ds);
  float* cont = new float[6 * (n ? n : 1)];
  unsigned* done = new unsigned[n ? n : 1];
  unsigned total = 0;
  for (size_t i = 0; i < n; ++i) {                       // phase A (k_target_a)
    RayOut r = target_ray_a(V, ds, max_steps, pos + 3 * i, vel + 3 * i, target + 3 * i, cont + 6 * i);
    memcpy(xt + 3 * i, r.xt, 12); memcpy(vt + 3 * i, r.vt, 12); dist2[i] = r.dist2;
    done[i] = r.steps; if (r.steps > total) total = r.steps;
  }
  for (size_t i = 0; i < n; ++i) {                       // phase B (k_target_b)
    if (done[i] >= total) continue;
    float best = dist2[i], x3[3], v3[3];
    if (target_ray_b(ds, done[i], total, cont + 6 * i, target + 3 * i, best, x3, v3)) {
      memcpy(xt + 3 * i, x3, 12); memcpy(vt + 3 * i, v3, 12); dist2[i] = best;
    }
  }
  if (iters) *iters = (int)total;
  delete[] cont; delete[] done;
  return 0;
}

EXPORT int hostcheck_backtrace(int use_sdf, const float* rif, const float* sdf, const int* res, size_t n,
                               const float* xt, const float* vt, const float* dx, const float* dv,
                               float h, float ds, float grad_scale, float* grad, long long* steps_total) {
  Vol V = make_vol(rif, res, h);
  int max_steps = (int)(2.0f * h * (float)max3(res) / ds);
  memset(grad, 0, sizeof(float) * (size_t)res[0] * res[1] * res[2]);
  long long st = 0;
  auto sink = [grad](const Cell& c, const Corners& w) {
    float* g = grad + c.base;
    g[0] += w.c000;            g[c.ox] += w.c100;
    g[c.oy] += w.c010;         g[c.oy + c.ox] += w.c110;
    g[c.oz] += w.c001;         g[c.oz + c.ox] += w.c101;
    g[c.oz + c.oy] += w.c011;  g[c.oz + c.oy + c.ox] += w.c111;
  };
  for (size_t i = 0; i < n; ++i)
    st += use_sdf ? backtrace_ray<1>(V, sdf, ds, grad_scale, max_steps, xt + 3 * i, vt + 3 * i, dx + 3 * i, dv + 3 * i, sink)
                  : backtrace_ray<0>(V, sdf, ds, grad_scale, max_steps, xt + 3 * i, vt + 3 * i, dx + 3 * i, dv + 3 * i, sink);
  if (steps_total) *steps_total = st;
  return 0;
}

EXPORT int hostcheck_trace_cable(const float* rif, int rres, float radius, float length, size_t n,
                                 const float* pos, const float* vel, const float* target, float ds,
                                 float* xt, float* vt, float* dist2, long long* steps_total) {
  Cyl C = make_cyl(rif, rres, radius, length);
  int max_steps = (int)(4.0f * length / ds);
  long long st = 0;
  for (size_t i = 0; i < n; ++i) {
    RayOut r = cable_trace_ray(C, ds, max_steps, pos + 3 * i, vel + 3 * i, target + 3 * i);
    memcpy(xt + 3 * i, r.xt, 12); memcpy(vt + 3 * i, r.vt, 12); dist2[i] = r.dist2; st += r.steps;
  }
  if (steps_total) *steps_total = st;
  return 0;
}

EXPORT int hostcheck_backtrace_cable(const float* rif, int rres, float radius, float length, size_t n,
                                     const float* xt, const float* vt, const float* dx, const float* dv,
                                     float ds, float* grad, long long* steps_total) {
  Cyl C = make_cyl(rif, rres, radius, length);
  int max_steps = (int)(4.0f * length / ds);
  memset(grad, 0, sizeof(float) * rres);
  long long st = 0;
  auto sink = [grad](int i0, int i1, float a0, float a1) { grad[i0] += a0; grad[i1] += a1; };
  for (size_t i = 0; i < n; ++i)
    st += cable_backtrace_ray(C, ds, max_steps, xt + 3 * i, vt + 3 * i, dx + 3 * i, dv + 3 * i, sink);
  if (steps_total) *steps_total = st;
  return 0;
}

// ---- ray-state adjoints: dL/dpos, dL/dvel --------------------------------------------------------------------------

// dpos, dvel: (n,3); steps: the forward's per-ray iteration counts; *ray_steps, *n_failed as in drrt_stats
EXPORT int raygrad_host_backtrace_rays(const float* rif, const int* res, size_t n, const float* pos, const float* vel,
                                       const float* xt, const float* vt, const uint32_t* steps, const float* dx,
                                       const float* dv, float h, float ds, float* dpos, float* dvel,
                                       long long* ray_steps, long long* n_failed) {
  Vol V = make_vol(rif, res, h);
  const int max_steps = (int)(4.0f * h * (float)max3(res) / ds);     // the forward's bound (drrt_api.hip steps_fwd)
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

// The two passes of the plane / SDF ray-state adjoint, looped as drrt_api.hip launches them: every ray with per-ray
// termination, then the flagged rays over the maximum of the first pass's iteration counts.
template <int MODE>
static void stop_backtrace_rays(const float* rif, const float* sdf, const int* res, size_t n, const float* pos,
                                const float* vel, const float* pln_o, const float* pln_d, const float* dx, const float* dv,
                                float h, float ds, float* dpos, float* dvel, float* xt, float* vt, uint32_t* jstar,
                                uint32_t* steps, uint32_t* fwd, uint8_t* flags, uint32_t* iters) {
  Vol V = make_vol(rif, res, h);
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
  if (mode == 1) stop_backtrace_rays<1>(rif, sdf, res, n, pos, vel, pln_o, pln_d, dx, dv, h, ds, dpos, dvel, xt, vt, jstar, steps, fwd, flags, iters);
  else if (mode == 2) stop_backtrace_rays<2>(rif, sdf, res, n, pos, vel, pln_o, pln_d, dx, dv, h, ds, dpos, dvel, xt, vt, jstar, steps, fwd, flags, iters);
  else return 1;
  return 0;
}

// ---- 16-bit ray state: the codecs ld3 / st3 call, array in / array out, on the Vol that vol_finish builds ------------
// out: q_min, q_step, q_inv_step
EXPORT int hostcheck_q16_params(const int* res, float h, float* out) {
  const Vol V = make_vol(nullptr, res, h);
  out[0] = V.q_min; out[1] = V.q_step; out[2] = V.q_inv_step;
  return 0;
}
EXPORT int hostcheck_q16_pos_enc(const int* res, float h, size_t n, const float* x, uint16_t* code) {
  const Vol V = make_vol(nullptr, res, h);
  for (size_t i = 0; i < n; ++i) code[i] = q16_pos_enc(V, x[i]);
  return 0;
}
EXPORT int hostcheck_q16_pos_dec(const int* res, float h, size_t n, const uint16_t* code, float* x) {
  const Vol V = make_vol(nullptr, res, h);
  for (size_t i = 0; i < n; ++i) x[i] = q16_pos_dec(V, code[i]);
  return 0;
}
EXPORT int hostcheck_q16_vel_enc(const int* res, float h, size_t n, const float* v, int16_t* code) {
  const Vol V = make_vol(nullptr, res, h);
  (void)V;
  for (size_t i = 0; i < n; ++i) code[i] = q16_vel_enc(v[i]);
  return 0;
}
EXPORT int hostcheck_q16_vel_dec(const int* res, float h, size_t n, const int16_t* code, float* v) {
  const Vol V = make_vol(nullptr, res, h);
  (void)V;
  for (size_t i = 0; i < n; ++i) v[i] = q16_vel_dec(code[i]);
  return 0;
}

// ---- locality-sort keys: the per-ray functions of drrt_keys.h that k_lightfield_keys / k_chord_keys call ----------------
EXPORT int hostcheck_hilbert2(size_t n, const uint32_t* x, const uint32_t* y, uint32_t* d) {
  for (size_t i = 0; i < n; ++i) d[i] = hilbert2(x[i], y[i]);
  return 0;
}
// a, b: n cells in [-15, 15]; c, t1, t2: (n,3)
EXPORT int hostcheck_lf_cell_frame(size_t n, const int* a, const int* b, float* c, float* t1, float* t2) {
  for (size_t i = 0; i < n; ++i) lf_cell_frame(a[i], b[i], c + 3 * i, t1 + 3 * i, t2 + 3 * i);
  return 0;
}
// the keys of the fp32 rays (pos, vel) heading along sign * vel, as the kernels form them
EXPORT int hostcheck_lightfield_keys(const int* res, float h, size_t n, const float* pos, const float* vel, float sign,
                                     uint32_t* keys) {
  const Vol V = make_vol(nullptr, res, h);
  for (size_t i = 0; i < n; ++i) {
    const float d[3] = {sign * vel[3 * i], sign * vel[3 * i + 1], sign * vel[3 * i + 2]};
    keys[i] = lightfield_key(V, pos + 3 * i, d);
  }
  return 0;
}
EXPORT int hostcheck_chord_keys(const int* res, float h, size_t n, const float* pos, const float* vel, float sign,
                                uint64_t* keys) {
  const Vol V = make_vol(nullptr, res, h);
  for (size_t i = 0; i < n; ++i) {
    const float d[3] = {sign * vel[3 * i], sign * vel[3 * i + 1], sign * vel[3 * i + 2]};
    keys[i] = chord_key(V, pos + 3 * i, d);
  }
  return 0;
}
