// cable_integral_rays.hip -- TEST INFRASTRUCTURE ONLY (never built or loaded by the package).
//
// The host build of the per-ray routines of the fibre march with a line integral up to its record: the optical path length
// (cable_trace_opl_ray, cable_opl_backtrace_ray) and the integral of a second radial profile (cable_trace_field_ray,
// cable_field_backtrace_ray of adjointnonlinearraytracing_amd/csrc/drrt_device.h), looped as drrt_cable.hip launches them,
// and the LDS rule of its kernels (cable_lds_bytes).  Compiled by tests/cable_integral_host.py with the line of
// tests/hostcheck_lib.py (`hipcc --cuda-host-only -O2 -ffp-contract=off -mfma`): the CPU tier compares it with float64
// autograd (tests/cable_opl_ad.py, tests/cable_field_ad.py), the GPU tier compares the kernels with it.  The profile
// gradients are summed in double here (the kernels sum f64 LDS atomics and fp32 global atomics in another order anyway).
//
// With -DCABLE_OPL_MAIN or -DCABLE_FIELD_MAIN it is a stand-alone program (its own main, nothing preloaded) for a build
// under AddressSanitizer + UndefinedBehaviorSanitizer: it makes its own cases (see the mains) and runs that operator's two
// routines on them, 0 = no report.
#include <math.h>

#include "host_common.h"

static int max_steps_of(float length, float ds) { return (int)(4.0f * length / ds); }   // drrt_api.hip cable_begin

EXPORT size_t cable_host_lds_bytes(int rres, int nprof, int ngrad) { return cable_lds_bytes(rres, nprof, ngrad); }

// xt, vt: (n,3); dist2, opl, rec_steps, steps (the march's iterations): n each; esc: n, 0 = the ray ran out of steps
EXPORT int cable_opl_host_trace(const float* rif, int rres, float radius, float length, size_t n, const float* pos,
                                const float* vel, const float* target, float ds, float* xt, float* vt, float* dist2,
                                float* opl, uint32_t* rec_steps, uint32_t* steps, uint8_t* esc) {
  const Cyl C = make_cyl(rif, rres, radius, length);
  const int max_steps = max_steps_of(length, ds);
  for (size_t i = 0; i < n; ++i) {
    const RayOut r = cable_trace_opl_ray(C, ds, max_steps, pos + 3 * i, vel + 3 * i, target + 3 * i, opl[i], rec_steps[i]);
    for (int k = 0; k < 3; ++k) { xt[3 * i + k] = r.xt[k]; vt[3 * i + k] = r.vt[k]; }
    dist2[i] = r.dist2; steps[i] = r.steps; esc[i] = r.esc ? 1 : 0;
  }
  return 0;
}

// dx, dv, dopl: nullable (zeros).  grad: double[rres], zeroed here.  dpos, dvel: (n,3); rsteps (reverse iterations),
// failed: n each.
EXPORT int cable_opl_host_backtrace(const float* rif, int rres, float radius, float length, size_t n, const float* pos,
                                    const float* xt, const float* vt, const uint32_t* rec_steps, const float* dx,
                                    const float* dv, const float* dopl, float ds, double* grad, float* dpos, float* dvel,
                                    uint32_t* rsteps, uint8_t* failed) {
  const Cyl C = make_cyl(rif, rres, radius, length);
  const int max_steps = max_steps_of(length, ds);
  for (int k = 0; k < rres; ++k) grad[k] = 0.0;
  auto sink = [grad](int i0, int i1, float a0, float a1) { grad[i0] += a0; grad[i1] += a1; };
  return backtrace_rays(n, dx, dv, dpos, dvel, rsteps, failed, [&](size_t i, const float* gx, const float* gv) {
    return cable_opl_backtrace_ray(C, ds, max_steps, pos + 3 * i, xt + 3 * i, vt + 3 * i, rec_steps[i], gx, gv,
                                   dopl ? dopl[i] : 0.f, sink);
  });
}

// As cable_opl_host_trace, with `field` (rres samples) and tau for opl
EXPORT int cable_field_host_trace(const float* rif, const float* field, int rres, float radius, float length, size_t n,
                                  const float* pos, const float* vel, const float* target, float ds, float* xt, float* vt,
                                  float* dist2, float* tau, uint32_t* rec_steps, uint32_t* steps, uint8_t* esc) {
  const Cyl C = make_cyl(rif, rres, radius, length);
  const int max_steps = max_steps_of(length, ds);
  for (size_t i = 0; i < n; ++i) {
    const RayOut r = cable_trace_field_ray(C, field, ds, max_steps, pos + 3 * i, vel + 3 * i, target + 3 * i, tau[i],
                                           rec_steps[i]);
    for (int k = 0; k < 3; ++k) { xt[3 * i + k] = r.xt[k]; vt[3 * i + k] = r.vt[k]; }
    dist2[i] = r.dist2; steps[i] = r.steps; esc[i] = r.esc ? 1 : 0;
  }
  return 0;
}

// As cable_opl_host_backtrace, with dtau for dopl and grad_field: double[rres], zeroed here
EXPORT int cable_field_host_backtrace(const float* rif, const float* field, int rres, float radius, float length, size_t n,
                                      const float* pos, const float* xt, const float* vt, const uint32_t* rec_steps,
                                      const float* dx, const float* dv, const float* dtau, float ds, double* grad,
                                      double* grad_field, float* dpos, float* dvel, uint32_t* rsteps, uint8_t* failed) {
  const Cyl C = make_cyl(rif, rres, radius, length);
  const int max_steps = max_steps_of(length, ds);
  for (int k = 0; k < rres; ++k) grad[k] = grad_field[k] = 0.0;
  auto sink = [grad](int i0, int i1, float a0, float a1) { grad[i0] += a0; grad[i1] += a1; };
  auto fsink = [grad_field](int i0, int i1, float a0, float a1) { grad_field[i0] += a0; grad_field[i1] += a1; };
  return backtrace_rays(n, dx, dv, dpos, dvel, rsteps, failed, [&](size_t i, const float* gx, const float* gv) {
    return cable_field_backtrace_ray(C, field, ds, max_steps, pos + 3 * i, xt + 3 * i, vt + 3 * i, rec_steps[i], gx, gv,
                                     dtau ? dtau[i] : 0.f, sink, fsink);
  });
}

#if defined(CABLE_OPL_MAIN) || defined(CABLE_FIELD_MAIN)
// Two profiles (2 samples; 33 samples with a NaN and an Inf entry; the field main: in each of its two profiles), rays from
// a fixed generator with NaN / Inf planted in positions, velocities, targets and seeds, the forward's own rec_steps and
// the two poisoned ones (max_steps + 1, 0xFFFFFFFF) on every fourth ray each.  A poisoned ray must come back failed with
// zero gradients and no iterations.
static uint32_t lcg(uint32_t& s) { s = s * 1664525u + 1013904223u; return s >> 8; }
static float uni(uint32_t& s) { return (float)lcg(s) / 16777216.0f; }

static const size_t kRays = 256;
static const float kRadius = 0.7f, kLength = 1.5f;

struct Rays {
  std::vector<float> pos, vel, tg, dx, dv, dint;            // dint: the seed on the integral
  std::vector<float> xt, vt, d2, integral, dpos, dvel;
  std::vector<uint32_t> rec, st, rs;
  std::vector<uint8_t> esc, fl;
};

static Rays make_rays(uint32_t s) {
  const float specials[4] = {NAN, INFINITY, -INFINITY, 0.f};
  const size_t n = kRays;
  Rays r{std::vector<float>(3 * n), std::vector<float>(3 * n), std::vector<float>(3 * n), std::vector<float>(3 * n),
         std::vector<float>(3 * n), std::vector<float>(n), std::vector<float>(3 * n), std::vector<float>(3 * n),
         std::vector<float>(n), std::vector<float>(n), std::vector<float>(3 * n), std::vector<float>(3 * n),
         std::vector<uint32_t>(n), std::vector<uint32_t>(n), std::vector<uint32_t>(n), std::vector<uint8_t>(n),
         std::vector<uint8_t>(n)};
  for (size_t i = 0; i < n; ++i) {
    for (int k = 0; k < 3; ++k) {
      r.pos[3 * i + k] = kRadius + (k == 1 ? 0.f : 0.8f * kRadius * (uni(s) - 0.5f));
      r.vel[3 * i + k] = k == 1 ? 1.f : 0.2f * (uni(s) - 0.5f);
      r.tg[3 * i + k] = r.pos[3 * i + k] + (k == 1 ? 3.f * kLength * uni(s) : 0.f);
      r.dx[3 * i + k] = uni(s) - 0.5f; r.dv[3 * i + k] = uni(s) - 0.5f;
    }
    r.dint[i] = uni(s) - 0.5f;
    if (i % 8 == 1) {                     // one special in one of the six arrays
      float* arrays[6] = {r.pos.data(), r.vel.data(), r.tg.data(), r.dx.data(), r.dv.data(), nullptr};
      const unsigned a = lcg(s) % 6u;
      const float v = specials[lcg(s) % 4u];
      if (arrays[a]) arrays[a][3 * i + lcg(s) % 3u] = v; else r.dint[i] = v;
    }
  }
  return r;
}

// the forward's counts are sane; then every fourth ray gets each of the two poisoned ones
static bool poison(Rays& r, uint32_t max_steps) {
  for (size_t i = 0; i < kRays; ++i) {
    if (r.rec[i] > r.st[i] || r.st[i] > max_steps) { printf("forward: bad counts on ray %zu\n", i); return false; }
    if (i % 4 == 2) r.rec[i] = max_steps + 1u;
    if (i % 4 == 3) r.rec[i] = 0xFFFFFFFFu;
  }
  return true;
}

static bool check_pass(const Rays& r, size_t& poisoned, unsigned long long& sum) {
  for (size_t i = 0; i < kRays; ++i) {
    const bool bad = i % 4 >= 2;
    if (bad != (r.fl[i] != 0)) { printf("ray %zu: failed = %d\n", i, r.fl[i]); return false; }
    if (bad) {
      ++poisoned;
      if (r.rs[i] != 0) { printf("ray %zu: a poisoned count made iterations\n", i); return false; }
      for (int k = 0; k < 3; ++k)
        if (r.dpos[3 * i + k] != 0.f || r.dvel[3 * i + k] != 0.f) { printf("ray %zu: gradient not zero\n", i); return false; }
    } else if (r.rs[i] != r.rec[i]) {
      printf("ray %zu: %u reverse iterations for j = %u\n", i, r.rs[i], r.rec[i]);
      return false;
    }
    sum += r.rs[i];
  }
  return true;
}

int main() {
  unsigned long long sum = 0;
  size_t poisoned = 0;
  for (int which = 0; which < 2; ++which) {
    const int rres = which ? 33 : 2;
    const float ds = which ? 0.011f : 0.012f;
    const size_t n = kRays;
    std::vector<float> prof(rres), field(rres);
    for (int k = 0; k < rres; ++k) {
      prof[k] = 1.5f - 0.2f * (float)k / (float)(rres - 1);
      field[k] = 0.5f + 0.3f * sinf(1.7f * (float)k);
    }
    if (which) { prof[7] = NAN; prof[20] = INFINITY; field[5] = INFINITY; field[21] = NAN; }
    std::vector<double> grad(rres), gfield(rres);
#ifdef CABLE_OPL_MAIN
    Rays r = make_rays(12345u + which);
    cable_opl_host_trace(prof.data(), rres, kRadius, kLength, n, r.pos.data(), r.vel.data(), r.tg.data(), ds, r.xt.data(),
                         r.vt.data(), r.d2.data(), r.integral.data(), r.rec.data(), r.st.data(), r.esc.data());
    if (!poison(r, (uint32_t)max_steps_of(kLength, ds))) return 1;
    for (int pass = 0; pass < 3; ++pass) {                  // all seeds; dopl alone; (dx, dv) alone
      cable_opl_host_backtrace(prof.data(), rres, kRadius, kLength, n, r.pos.data(), r.xt.data(), r.vt.data(), r.rec.data(),
                               pass == 1 ? nullptr : r.dx.data(), pass == 1 ? nullptr : r.dv.data(),
                               pass == 2 ? nullptr : r.dint.data(), ds, grad.data(), r.dpos.data(), r.dvel.data(),
                               r.rs.data(), r.fl.data());
      if (!check_pass(r, poisoned, sum)) return 1;
    }
#else
    Rays r = make_rays(54321u + which);
    cable_field_host_trace(prof.data(), field.data(), rres, kRadius, kLength, n, r.pos.data(), r.vel.data(), r.tg.data(), ds,
                           r.xt.data(), r.vt.data(), r.d2.data(), r.integral.data(), r.rec.data(), r.st.data(),
                           r.esc.data());
    if (!poison(r, (uint32_t)max_steps_of(kLength, ds))) return 1;
    for (int pass = 0; pass < 4; ++pass) {                  // all seeds; dtau alone; (dx, dv) alone; field = the profile
      const float* f = pass == 3 ? prof.data() : field.data();
      cable_field_host_backtrace(prof.data(), f, rres, kRadius, kLength, n, r.pos.data(), r.xt.data(), r.vt.data(),
                                 r.rec.data(), pass == 1 ? nullptr : r.dx.data(), pass == 1 ? nullptr : r.dv.data(),
                                 pass == 2 ? nullptr : r.dint.data(), ds, grad.data(), gfield.data(), r.dpos.data(),
                                 r.dvel.data(), r.rs.data(), r.fl.data());
      if (!check_pass(r, poisoned, sum)) return 1;
    }
#endif
  }
  return finished("%zu poisoned rays refused, %llu reverse iterations", poisoned, sum);
}
#endif
