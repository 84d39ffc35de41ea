// cable_field_rays.hip -- TEST INFRASTRUCTURE ONLY (never built or loaded by the package).
//
// The host build of the two routines of the fibre march with the line integral of a second radial profile
// (cable_trace_field_ray, cable_field_backtrace_ray of adjointnonlinearraytracing_amd/csrc/drrt_device.h), looped as
// drrt_cable_field.hip launches them.  Compiled by tests/cable_field_host.py with the line of tests/hostcheck_lib.py
// (`hipcc --cuda-host-only -O2 -ffp-contract=off -mfma`): the CPU tier compares it with float64 autograd
// (tests/cable_field_ad.py), the GPU tier compares the kernels with it.  Both profile gradients are summed in double here
// (the kernels sum f64 LDS atomics and fp32 global atomics in another order anyway).
//
// With -DCABLE_FIELD_MAIN it is a stand-alone program (its own main, nothing preloaded) for a build under AddressSanitizer +
// UndefinedBehaviorSanitizer: it makes its own cases (see main) and runs both routines on them, 0 = no report.
#include <math.h>
#include <stdint.h>
#include <stddef.h>
#include <stdio.h>

#include <vector>

#include "../../adjointnonlinearraytracing_amd/csrc/drrt_device.h"

using namespace drrt;

#define EXPORT extern "C" __attribute__((visibility("default")))

static int max_steps_of(float length, float ds) { return (int)(4.0f * length / ds); }   // drrt_api.hip cable_begin

// xt, vt: (n,3); dist2, tau, rec_steps, steps (the march's iterations): n each; esc: n, 0 = the ray ran out of steps
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

// dx, dv, dtau: nullable (zeros).  grad, grad_field: double[rres] each, zeroed here.  dpos, dvel: (n,3); rsteps (reverse
// iterations), failed: n each.
EXPORT int cable_field_host_backtrace(const float* rif, const float* field, int rres, float radius, float length, size_t n,
                                      const float* pos, const float* xt, const float* vt, const uint32_t* rec_steps,
                                      const float* dx, const float* dv, const float* dtau, float ds, double* grad,
                                      double* grad_field, float* dpos, float* dvel, uint32_t* rsteps, uint8_t* failed) {
  const Cyl C = make_cyl(rif, rres, radius, length);
  const int max_steps = max_steps_of(length, ds);
  for (int k = 0; k < rres; ++k) grad[k] = grad_field[k] = 0.0;
  auto sink = [grad](int i0, int i1, float a0, float a1) { grad[i0] += a0; grad[i1] += a1; };
  auto fsink = [grad_field](int i0, int i1, float a0, float a1) { grad_field[i0] += a0; grad_field[i1] += a1; };
  const float zero[3] = {0.f, 0.f, 0.f};
  for (size_t i = 0; i < n; ++i) {
    const RayGrad g = cable_field_backtrace_ray(C, field, ds, max_steps, pos + 3 * i, xt + 3 * i, vt + 3 * i, rec_steps[i],
                                                dx ? dx + 3 * i : zero, dv ? dv + 3 * i : zero, dtau ? dtau[i] : 0.f, sink,
                                                fsink);
    for (int k = 0; k < 3; ++k) { dpos[3 * i + k] = g.dp[k]; dvel[3 * i + k] = g.dv[k]; }
    rsteps[i] = g.steps; failed[i] = g.failed ? 1 : 0;
  }
  return 0;
}

#ifdef CABLE_FIELD_MAIN
// Two profile pairs (2 samples; 33 samples with a NaN and an Inf entry in each profile), rays from a fixed generator with
// NaN / Inf planted in positions, velocities, targets and seeds, the forward's own rec_steps and the two poisoned ones
// (max_steps + 1, 0xFFFFFFFF) on every fourth ray each.  A poisoned ray must come back failed with zero gradients and no
// iterations.
static uint32_t lcg(uint32_t& s) { s = s * 1664525u + 1013904223u; return s >> 8; }
static float uni(uint32_t& s) { return (float)lcg(s) / 16777216.0f; }

int main() {
  const float specials[4] = {NAN, INFINITY, -INFINITY, 0.f};
  unsigned long long sum = 0;
  size_t poisoned = 0;
  for (int which = 0; which < 2; ++which) {
    const int rres = which ? 33 : 2;
    const float radius = 0.7f, length = 1.5f, ds = which ? 0.011f : 0.012f;
    std::vector<float> prof(rres), field(rres);
    for (int k = 0; k < rres; ++k) {
      prof[k] = 1.5f - 0.2f * (float)k / (float)(rres - 1);
      field[k] = 0.5f + 0.3f * sinf(1.7f * (float)k);
    }
    if (which) { prof[7] = NAN; prof[20] = INFINITY; field[5] = INFINITY; field[21] = NAN; }
    const size_t n = 256;
    uint32_t s = 54321u + which;
    std::vector<float> pos(3 * n), vel(3 * n), tg(3 * n), dx(3 * n), dv(3 * n), dtau(n);
    for (size_t i = 0; i < n; ++i) {
      for (int k = 0; k < 3; ++k) {
        pos[3 * i + k] = radius + (k == 1 ? 0.f : 0.8f * radius * (uni(s) - 0.5f));
        vel[3 * i + k] = k == 1 ? 1.f : 0.2f * (uni(s) - 0.5f);
        tg[3 * i + k] = pos[3 * i + k] + (k == 1 ? 3.f * length * uni(s) : 0.f);
        dx[3 * i + k] = uni(s) - 0.5f; dv[3 * i + k] = uni(s) - 0.5f;
      }
      dtau[i] = uni(s) - 0.5f;
      if (i % 8 == 1) {                     // one special in one of the six arrays
        float* arrays[6] = {pos.data(), vel.data(), tg.data(), dx.data(), dv.data(), nullptr};
        const unsigned a = lcg(s) % 6u;
        const float v = specials[lcg(s) % 4u];
        if (arrays[a]) arrays[a][3 * i + lcg(s) % 3u] = v; else dtau[i] = v;
      }
    }
    std::vector<float> xt(3 * n), vt(3 * n), d2(n), tau(n), dpos(3 * n), dvel(3 * n);
    std::vector<uint32_t> rec(n), st(n), rs(n);
    std::vector<uint8_t> esc(n), fl(n);
    std::vector<double> grad(rres), gfield(rres);
    cable_field_host_trace(prof.data(), field.data(), rres, radius, length, n, pos.data(), vel.data(), tg.data(), ds,
                           xt.data(), vt.data(), d2.data(), tau.data(), rec.data(), st.data(), esc.data());
    const uint32_t max_steps = (uint32_t)max_steps_of(length, ds);
    for (size_t i = 0; i < n; ++i) {
      if (rec[i] > st[i] || st[i] > max_steps) { printf("forward: bad counts on ray %zu\n", i); return 1; }
      if (i % 4 == 2) rec[i] = max_steps + 1u;
      if (i % 4 == 3) rec[i] = 0xFFFFFFFFu;
    }
    for (int pass = 0; pass < 4; ++pass) {                  // all seeds; dtau alone; (dx, dv) alone; field = the profile
      const float* f = pass == 3 ? prof.data() : field.data();
      cable_field_host_backtrace(prof.data(), f, rres, radius, length, n, pos.data(), xt.data(), vt.data(), rec.data(),
                                 pass == 1 ? nullptr : dx.data(), pass == 1 ? nullptr : dv.data(),
                                 pass == 2 ? nullptr : dtau.data(), ds, grad.data(), gfield.data(), dpos.data(), dvel.data(),
                                 rs.data(), fl.data());
      for (size_t i = 0; i < n; ++i) {
        const bool bad = i % 4 >= 2;
        if (bad != (fl[i] != 0)) { printf("ray %zu: failed = %d\n", i, fl[i]); return 1; }
        if (bad) {
          ++poisoned;
          if (rs[i] != 0) { printf("ray %zu: a poisoned count made iterations\n", i); return 1; }
          for (int k = 0; k < 3; ++k)
            if (dpos[3 * i + k] != 0.f || dvel[3 * i + k] != 0.f) { printf("ray %zu: gradient not zero\n", i); return 1; }
        } else if (rs[i] != rec[i]) { printf("ray %zu: %u reverse iterations for j = %u\n", i, rs[i], rec[i]); return 1; }
        sum += rs[i];
      }
    }
  }
  printf("%zu poisoned rays refused, %llu reverse iterations\nsanitizer run finished without reports\n", poisoned, sum);
  return 0;
}
#endif
