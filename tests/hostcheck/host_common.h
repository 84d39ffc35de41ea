// host_common.h -- TEST INFRASTRUCTURE ONLY (never built or loaded by the package).
//
// What the host builds of the per-ray routines (integral_rays.hip, target_rays.hip, cable_integral_rays.hip) share: the
// Vol and step bound of a call, the taps and the double-summing sinks of a grid, the one forward and the one reverse loop
// over the rays, and, for the stand-alone sanitizer programs, the reader of a case file, the three-pass loop and the
// closing line.  An operator adds the one call in the middle of each loop.
#pragma once
#include <stdarg.h>
#include <stdint.h>
#include <stddef.h>
#include <stdio.h>

#include <vector>

#include "../../adjointnonlinearraytracing_amd/csrc/drrt_device.h"

using namespace drrt;

#define EXPORT extern "C" __attribute__((visibility("default")))

static inline Vol vol(const float* rif, const int* res, float h) {
  Vol V;
  V.data = rif; V.W = res[0]; V.H = res[1]; V.D = res[2];
  vol_finish(V, h);
  return V;
}
static inline int max_steps_of(const int* res, float h, float ds) {      // the forward's bound (drrt_api.hip steps_fwd)
  const int mx = res[0] > res[1] ? (res[0] > res[2] ? res[0] : res[2]) : (res[1] > res[2] ? res[1] : res[2]);
  return (int)(4.0f * h * (float)mx / ds);
}
static inline void add_corners(double* grad, const Cell& c, const Corners& w) {
  double* g = grad + c.base;
  g[0] += w.c000;            g[c.ox] += w.c100;
  g[c.oy] += w.c010;         g[c.oy + c.ox] += w.c110;
  g[c.oz] += w.c001;         g[c.oz + c.ox] += w.c101;
  g[c.oz + c.oy] += w.c011;  g[c.oz + c.oy + c.ox] += w.c111;
}

// ---- a grid's taps and sinks ---------------------------------------------------------------------------------------------
struct GridTaps {                                                        // taps(c) of one grid
  const float* data;
  Taps operator()(const Cell& c) const { return fetch(data, c); }
};

// The sinks sum in double, in the order they are called.  `parts`: 0 = the whole contribution, 1 = its value weights
// alone, 2 = its gradient splat alone; a ValueSink's contributions have no splat, so 2 leaves its grid zero.
struct SplatSink {                                                       // sink(c, val, gx, gy, gz) of dL/dn
  double* grad; int parts;
  void operator()(const Cell& c, float val, float gx, float gy, float gz) const {
    if (parts == 1) gx = gy = gz = 0.f;
    if (parts == 2) val = 0.f;
    add_corners(grad, c, splat_weights(c.wx, c.wy, c.wz, val, gx, gy, gz));
  }
};
struct ValueSink {                                                       // sink(c, val) of a further grid
  double* grad; int parts;
  void operator()(const Cell& c, float val) const {
    if (parts != 2) add_corners(grad, c, value_weights(c.wx, c.wy, c.wz, val));
  }
};
template <typename Sink>
static Sink zeroed(double* grad, size_t count, int parts = 0) {          // the sink of a grid, which it zeroes
  for (size_t k = 0; k < count; ++k) grad[k] = 0.0;
  return Sink{grad, parts};
}

// ---- the loops over the rays -------------------------------------------------------------------------------------------
// Forward: ray(i, p, v) -> RayOut.  xt, vt: (n,3); steps: n; *n_failed as in drrt_stats.
template <typename RayFn>
static int trace_rays(size_t n, const float* pos, const float* vel, float* xt, float* vt, uint32_t* steps,
                      long long* n_failed, RayFn&& ray) {
  long long nf = 0;
  for (size_t i = 0; i < n; ++i) {
    const RayOut r = ray(i, pos + 3 * i, vel + 3 * i);
    for (int k = 0; k < 3; ++k) { xt[3 * i + k] = r.xt[k]; vt[3 * i + k] = r.vt[k]; }
    steps[i] = r.steps;
    nf += r.act ? 1 : 0;
  }
  *n_failed = nf;
  return 0;
}

// Reverse: ray(i, dx, dv) -> RayGrad, rays in ascending order; dx, dv: nullable (the callable sees zeros).  dpos, dvel:
// (n,3); rsteps (reverse iterations), failed: n each.
template <typename RayFn>
static int backtrace_rays(size_t n, const float* dx, const float* dv, float* dpos, float* dvel, uint32_t* rsteps,
                          uint8_t* failed, RayFn&& ray) {
  const float zero[3] = {0.f, 0.f, 0.f};
  for (size_t i = 0; i < n; ++i) {
    const RayGrad r = ray(i, dx ? dx + 3 * i : zero, dv ? dv + 3 * i : zero);
    for (int k = 0; k < 3; ++k) { dpos[3 * i + k] = r.dp[k]; dvel[3 * i + k] = r.dv[k]; }
    rsteps[i] = r.steps; failed[i] = r.failed ? 1 : 0;
  }
  return 0;
}

// ---- the stand-alone programs ------------------------------------------------------------------------------------------
// A case file on a grid: `ints` int32 (W, H, D, n, then the operator's own, each >= 1); float32 h, ds; then float32 arrays,
// read in the file's order with floats(count).  A bad header or a short read leaves ok false.
struct CaseFile {
  FILE* f = nullptr;
  bool ok = false;
  int hd[8] = {};
  float h = 0.f, ds = 0.f;
  size_t nvox = 0, n = 0;

  CaseFile(int argc, char** argv, int ints = 4) {
    float sc[2];
    if (argc < 2 || !(f = fopen(argv[1], "rb"))) return;
    if (fread(hd, sizeof(int), ints, f) != (size_t)ints || fread(sc, sizeof(float), 2, f) != 2) return;
    if (hd[0] < 1 || hd[1] < 1 || hd[2] < 1 || hd[3] < 0) return;
    for (int k = 4; k < ints; ++k) if (hd[k] < 1) return;
    h = sc[0]; ds = sc[1];
    nvox = (size_t)hd[0] * hd[1] * hd[2]; n = (size_t)hd[3];
    ok = true;
  }
  ~CaseFile() { if (f) fclose(f); }
  CaseFile(const CaseFile&) = delete;
  CaseFile& operator=(const CaseFile&) = delete;

  std::vector<float> floats(size_t count) {
    std::vector<float> a(ok ? count : 0);
    ok = ok && fread(a.data(), sizeof(float), count, f) == count;
    return a;
  }
};

// What the program of an operator of trace_rays / backtrace_rays keeps per ray, and its checksum.
struct RayRun {
  std::vector<float> xt, vt, dpos, dvel;
  std::vector<uint32_t> st, rs;
  std::vector<uint8_t> fl;
  long long nf = 0;
  unsigned long long sum = 0;
  explicit RayRun(size_t n) : xt(3 * n), vt(3 * n), dpos(3 * n), dvel(3 * n), st(n), rs(n), fl(n) {}

  // back(pass), pass = 0, 1, 2: the operator's adjoint into dpos, dvel, rs, fl, another choice of null seeds, flag and
  // parts on each pass
  template <typename BackFn>
  void three_passes(BackFn&& back) {
    for (int pass = 0; pass < 3; ++pass) {
      back(pass);
      for (size_t i = 0; i < rs.size(); ++i) sum += rs[i] + fl[i];
    }
    for (size_t i = 0; i < st.size(); ++i) sum += st[i];
  }
};

// "<the program's own line>\nsanitizer run finished without reports\n"; -> 0, the exit status of a clean run
__attribute__((format(printf, 1, 2))) static inline int finished(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vprintf(fmt, ap);
  va_end(ap);
  printf("\nsanitizer run finished without reports\n");
  return 0;
}
