// integral_rays.hip -- TEST INFRASTRUCTURE ONLY (never built or loaded by the package).
//
// The host build of the routines of the grid integral family -- optical path length (trace_opl_ray, opl_backtrace_ray),
// line integral of a second field (trace_field_ray, field_backtrace_ray), emission with self-absorption (exp_neg,
// trace_emission_ray, emission_backtrace_ray), line integral of a vector field (trace_vector_ray, vector_backtrace_ray) and
// ray paths without and with the velocity series (trace_path_ray, path_backtrace_ray: path_host_*; trace_phase_ray,
// phase_backtrace_ray: phase_host_*) of adjointnonlinearraytracing_amd/csrc/drrt_device.h -- looped as drrt_integral.hip
// launches them: every export names its taps and sinks and the one call per ray, the loops are
// host_common.h's.  Compiled by tests/integral_host.py with the line of tests/hostcheck_lib.py (`hipcc --cuda-host-only -O2
// -ffp-contract=off -mfma`): the CPU tier compares it with float64 autograd (tests/opl_ad.py, field_ad.py, emission_ad.py,
// vector_ad.py, path_ad.py), the GPU tier compares the kernels with it.  Every grid gradient is summed in double here (the
// kernels sum fp32 atomics in another order anyway), and the two parts of a contribution to dL/dn -- the value weights and
// the gradient splat that DRRT_FLAG_CORRECTED_H scales -- can be had separately (`parts`); a contribution to a further grid
// (dL/dfield, dL/de, dL/da, a plane of dL/du) has value weights only, so `parts` = 2 leaves those grids zero.
//
// With -DOPL_MAIN, -DFIELD_MAIN, -DEMISSION_MAIN, -DVECTOR_MAIN, -DPATH_MAIN or -DPHASE_MAIN it is a stand-alone program
// (its own main, nothing preloaded) for a build under AddressSanitizer + UndefinedBehaviorSanitizer: argv[1] names a file with one case of
// that operator (see its main), all its routines run on it, 0 = no report.
#include "host_common.h"

// What every export derives from (rif, res, h, ds[, corrected_h]).
struct Call {
  Vol V; int max_steps; float grad_scale; size_t nvox; GridTaps taps;
  Call(const float* rif, const int* res, float h, float ds, int corrected_h = 0)
      : V(vol(rif, res, h)), max_steps(max_steps_of(res, h, ds)), grad_scale(corrected_h ? V.inv_h : 1.0f),
        nvox((size_t)res[0] * res[1] * res[2]), taps{rif} {}
};

// ---- optical path length ---------------------------------------------------------------------------------------------
// xt, vt: (n,3); opl, steps: n; *n_failed as in drrt_stats
EXPORT int opl_host_trace(const float* rif, const int* res, size_t n, const float* pos, const float* vel, float h, float ds,
                          float* xt, float* vt, float* opl, uint32_t* steps, long long* n_failed) {
  const Call c(rif, res, h, ds);
  return trace_rays(n, pos, vel, xt, vt, steps, n_failed, [&](size_t i, const float* p, const float* v) {
    return trace_opl_ray(c.V, ds, c.max_steps, p, v, c.taps, opl[i]);
  });
}

// dx, dv, dopl: nullable (zeros).  grad: double[nvox], zeroed here.  parts: 0 = the whole contribution, 1 = its value
// weights alone, 2 = its gradient splat alone.  dpos, dvel: (n,3); rsteps (reverse iterations), failed: n each.
EXPORT int opl_host_backtrace(const float* rif, const int* res, size_t n, const float* pos, const float* vel,
                              const float* xt, const float* vt, const uint32_t* fsteps, const float* dx, const float* dv,
                              const float* dopl, float h, float ds, int corrected_h, int parts, double* grad, float* dpos,
                              float* dvel, uint32_t* rsteps, uint8_t* failed) {
  const Call c(rif, res, h, ds, corrected_h);
  const SplatSink sink = zeroed<SplatSink>(grad, c.nvox, parts);
  return backtrace_rays(n, dx, dv, dpos, dvel, rsteps, failed, [&](size_t i, const float* gx, const float* gv) {
    return opl_backtrace_ray(c.V, ds, c.grad_scale, c.max_steps, fsteps[i], pos + 3 * i, vel + 3 * i, xt + 3 * i,
                             vt + 3 * i, gx, gv, dopl ? dopl[i] : 0.f, c.taps, sink);
  });
}

#ifdef OPL_MAIN
// The case file: int32 W, H, D, n; float32 h, ds; then float32 arrays rif[W*H*D], pos, vel, dx, dv (n*3 each), dopl[n].
int main(int argc, char** argv) {
  CaseFile c(argc, argv);
  const size_t n = c.n;
  const std::vector<float> rif = c.floats(c.nvox), pos = c.floats(3 * n), vel = c.floats(3 * n), dx = c.floats(3 * n),
                           dv = c.floats(3 * n), dopl = c.floats(n);
  if (!c.ok) return 2;
  RayRun o(n);
  std::vector<float> opl(n);
  std::vector<double> grad(c.nvox);
  opl_host_trace(rif.data(), c.hd, n, pos.data(), vel.data(), c.h, c.ds, o.xt.data(), o.vt.data(), opl.data(), o.st.data(),
                 &o.nf);
  o.three_passes([&](int pass) {                          // all seeds, flag on; no seeds on the rays, flag off, one part
    opl_host_backtrace(rif.data(), c.hd, n, pos.data(), vel.data(), o.xt.data(), o.vt.data(), o.st.data(),
                       pass == 1 ? nullptr : dx.data(), pass == 1 ? nullptr : dv.data(), pass == 2 ? nullptr : dopl.data(),
                       c.h, c.ds, pass != 1, pass, grad.data(), o.dpos.data(), o.dvel.data(), o.rs.data(), o.fl.data());
  });
  return finished("%zu rays, %lld failed, checksum %llu", n, o.nf, o.sum);
}
#endif

// ---- line integral of a second field -----------------------------------------------------------------------------------
// xt, vt: (n,3); tau, steps: n; *n_failed as in drrt_stats
EXPORT int field_host_trace(const float* rif, const float* field, const int* res, size_t n, const float* pos,
                            const float* vel, float h, float ds, float* xt, float* vt, float* tau, uint32_t* steps,
                            long long* n_failed) {
  const Call c(rif, res, h, ds);
  const GridTaps ftaps{field};
  return trace_rays(n, pos, vel, xt, vt, steps, n_failed, [&](size_t i, const float* p, const float* v) {
    return trace_field_ray(c.V, ds, c.max_steps, p, v, c.taps, ftaps, tau[i]);
  });
}

// dx, dv, dtau: nullable (zeros).  grad, grad_field: double[nvox], zeroed here.  parts: 0 = the whole contribution, 1 = its
// value weights alone, 2 = its gradient splat alone.  dpos, dvel: (n,3); rsteps (reverse iterations), failed: n each.
EXPORT int field_host_backtrace(const float* rif, const float* field, const int* res, size_t n, const float* pos,
                                const float* vel, const float* xt, const float* vt, const uint32_t* fsteps, const float* dx,
                                const float* dv, const float* dtau, float h, float ds, int corrected_h, int parts,
                                double* grad, double* grad_field, float* dpos, float* dvel, uint32_t* rsteps,
                                uint8_t* failed) {
  const Call c(rif, res, h, ds, corrected_h);
  const GridTaps ftaps{field};
  const SplatSink sink = zeroed<SplatSink>(grad, c.nvox, parts);
  const ValueSink fsink = zeroed<ValueSink>(grad_field, c.nvox, parts);
  return backtrace_rays(n, dx, dv, dpos, dvel, rsteps, failed, [&](size_t i, const float* gx, const float* gv) {
    return field_backtrace_ray(c.V, ds, c.grad_scale, c.max_steps, fsteps[i], pos + 3 * i, vel + 3 * i, xt + 3 * i,
                               vt + 3 * i, gx, gv, dtau ? dtau[i] : 0.f, c.taps, ftaps, sink, fsink);
  });
}

#ifdef FIELD_MAIN
// The case file: int32 W, H, D, n; float32 h, ds; then float32 arrays rif[W*H*D], field[W*H*D], pos, vel, dx, dv (n*3 each),
// dtau[n].
int main(int argc, char** argv) {
  CaseFile c(argc, argv);
  const size_t n = c.n;
  const std::vector<float> rif = c.floats(c.nvox), field = c.floats(c.nvox), pos = c.floats(3 * n), vel = c.floats(3 * n),
                           dx = c.floats(3 * n), dv = c.floats(3 * n), dtau = c.floats(n);
  if (!c.ok) return 2;
  RayRun o(n);
  std::vector<float> tau(n);
  std::vector<double> grad(c.nvox), gfield(c.nvox);
  field_host_trace(rif.data(), field.data(), c.hd, n, pos.data(), vel.data(), c.h, c.ds, o.xt.data(), o.vt.data(),
                   tau.data(), o.st.data(), &o.nf);
  o.three_passes([&](int pass) {                          // all seeds, flag on; no seeds on the rays, flag off, one part
    field_host_backtrace(rif.data(), field.data(), c.hd, n, pos.data(), vel.data(), o.xt.data(), o.vt.data(), o.st.data(),
                         pass == 1 ? nullptr : dx.data(), pass == 1 ? nullptr : dv.data(),
                         pass == 2 ? nullptr : dtau.data(), c.h, c.ds, pass != 1, pass, grad.data(), gfield.data(),
                         o.dpos.data(), o.dvel.data(), o.rs.data(), o.fl.data());
  });
  return finished("%zu rays, %lld failed, checksum %llu", n, o.nf, o.sum);
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
  const Call c(rif, res, h, ds);
  const GridTaps etaps{emis}, ataps{absb};
  return trace_rays(n, pos, vel, xt, vt, steps, n_failed, [&](size_t i, const float* p, const float* v) {
    return trace_emission_ray(c.V, ds, c.max_steps, p, v, c.taps, etaps, ataps, rad[i], tau[i]);
  });
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
  const Call c(rif, res, h, ds, corrected_h);
  const GridTaps etaps{emis}, ataps{absb};
  const SplatSink sink = zeroed<SplatSink>(grad, c.nvox, parts);
  const ValueSink esink = zeroed<ValueSink>(grad_e, c.nvox, parts), asink = zeroed<ValueSink>(grad_a, c.nvox, parts);
  return backtrace_rays(n, dx, dv, dpos, dvel, rsteps, failed, [&](size_t i, const float* gx, const float* gv) {
    return emission_backtrace_ray(c.V, ds, c.grad_scale, c.max_steps, fsteps[i], pos + 3 * i, vel + 3 * i, xt + 3 * i,
                                  vt + 3 * i, tau[i], gx, gv, drad ? drad[i] : 0.f, dtau ? dtau[i] : 0.f, c.taps, etaps,
                                  ataps, sink, esink, asink);
  });
}

#ifdef EMISSION_MAIN
// The case file: int32 W, H, D, n; float32 h, ds; then float32 arrays rif[W*H*D], emission[W*H*D], absorption[W*H*D], pos,
// vel, dx, dv (n*3 each), drad[n], dtau[n].
int main(int argc, char** argv) {
  CaseFile c(argc, argv);
  const size_t n = c.n;
  const std::vector<float> rif = c.floats(c.nvox), emis = c.floats(c.nvox), absb = c.floats(c.nvox), pos = c.floats(3 * n),
                           vel = c.floats(3 * n), dx = c.floats(3 * n), dv = c.floats(3 * n), drad = c.floats(n),
                           dtau = c.floats(n);
  if (!c.ok) return 2;
  RayRun o(n);
  std::vector<float> rad(n), tau(n), ex(n);
  std::vector<double> grad(c.nvox), ge(c.nvox), ga(c.nvox);
  emission_host_exp_neg(dtau.data(), n, ex.data());        // the seeds on tau carry NaN, +-Inf, +-3e38 and denormals
  const float edge[8] = {0.f, -0.f, 87.f, -87.f, 88.f, -88.f, 1e-40f, -1e-40f};
  float eout[8];
  emission_host_exp_neg(edge, 8, eout);
  emission_host_trace(rif.data(), emis.data(), absb.data(), c.hd, n, pos.data(), vel.data(), c.h, c.ds, o.xt.data(),
                      o.vt.data(), rad.data(), tau.data(), o.st.data(), &o.nf);
  o.three_passes([&](int pass) {                          // all seeds, flag on; no seeds on the rays, flag off, one part
    emission_host_backtrace(rif.data(), emis.data(), absb.data(), c.hd, n, pos.data(), vel.data(), o.xt.data(),
                            o.vt.data(), o.st.data(), tau.data(), pass == 1 ? nullptr : dx.data(),
                            pass == 1 ? nullptr : dv.data(), drad.data(), pass == 2 ? nullptr : dtau.data(), c.h, c.ds,
                            pass != 1, pass, grad.data(), ge.data(), ga.data(), o.dpos.data(), o.dvel.data(), o.rs.data(),
                            o.fl.data());
  });
  return finished("%zu rays, %lld failed, checksum %llu, exp_neg(0) %.9g", n, o.nf, o.sum, (double)eout[0]);
}
#endif

// ---- line integral of a vector field -----------------------------------------------------------------------------------
// vfield: 3 nvox floats, plane k at + k nvox.  xt, vt: (n,3); circ, steps: n; *n_failed as in drrt_stats
EXPORT int vector_host_trace(const float* rif, const float* vfield, const int* res, size_t n, const float* pos,
                             const float* vel, float h, float ds, float* xt, float* vt, float* circ, uint32_t* steps,
                             long long* n_failed) {
  const Call c(rif, res, h, ds);
  auto vtaps = [&](const Cell& cell, int k) -> Taps { return fetch(vfield + (size_t)k * c.nvox, cell); };
  return trace_rays(n, pos, vel, xt, vt, steps, n_failed, [&](size_t i, const float* p, const float* v) {
    return trace_vector_ray(c.V, ds, c.max_steps, p, v, c.taps, vtaps, circ[i]);
  });
}

// dx, dv, dcirc: nullable (zeros).  grad: double[nvox], grad_vfield: double[3 nvox], zeroed here.  parts: 0 = the whole
// contribution, 1 = its value weights alone, 2 = its gradient splat alone.  dpos, dvel: (n,3); rsteps (reverse iterations),
// failed: n each.
EXPORT int vector_host_backtrace(const float* rif, const float* vfield, const int* res, size_t n, const float* pos,
                                 const float* vel, const float* xt, const float* vt, const uint32_t* fsteps,
                                 const float* dx, const float* dv, const float* dcirc, float h, float ds, int corrected_h,
                                 int parts, double* grad, double* grad_vfield, float* dpos, float* dvel, uint32_t* rsteps,
                                 uint8_t* failed) {
  const Call c(rif, res, h, ds, corrected_h);
  auto vtaps = [&](const Cell& cell, int k) -> Taps { return fetch(vfield + (size_t)k * c.nvox, cell); };
  const SplatSink sink = zeroed<SplatSink>(grad, c.nvox, parts);
  const ValueSink planes = zeroed<ValueSink>(grad_vfield, 3 * c.nvox, parts);
  auto vsink = [&](int k, const Cell& cell, float val) { ValueSink{planes.grad + (size_t)k * c.nvox, parts}(cell, val); };
  return backtrace_rays(n, dx, dv, dpos, dvel, rsteps, failed, [&](size_t i, const float* gx, const float* gv) {
    return vector_backtrace_ray(c.V, ds, c.grad_scale, c.max_steps, fsteps[i], pos + 3 * i, vel + 3 * i, xt + 3 * i,
                                vt + 3 * i, gx, gv, dcirc ? dcirc[i] : 0.f, c.taps, vtaps, sink, vsink);
  });
}

#ifdef VECTOR_MAIN
// The case file: int32 W, H, D, n; float32 h, ds; then float32 arrays rif[W*H*D], vfield[3*W*H*D], pos, vel, dx, dv (n*3
// each), dcirc[n].
int main(int argc, char** argv) {
  CaseFile c(argc, argv);
  const size_t n = c.n;
  const std::vector<float> rif = c.floats(c.nvox), vfield = c.floats(3 * c.nvox), pos = c.floats(3 * n),
                           vel = c.floats(3 * n), dx = c.floats(3 * n), dv = c.floats(3 * n), dcirc = c.floats(n);
  if (!c.ok) return 2;
  RayRun o(n);
  std::vector<float> circ(n);
  std::vector<double> grad(c.nvox), gv(3 * c.nvox);
  vector_host_trace(rif.data(), vfield.data(), c.hd, n, pos.data(), vel.data(), c.h, c.ds, o.xt.data(), o.vt.data(),
                    circ.data(), o.st.data(), &o.nf);
  o.three_passes([&](int pass) {                          // all seeds, flag on; no seeds on the rays, flag off, one part
    vector_host_backtrace(rif.data(), vfield.data(), c.hd, n, pos.data(), vel.data(), o.xt.data(), o.vt.data(), o.st.data(),
                          pass == 1 ? nullptr : dx.data(), pass == 1 ? nullptr : dv.data(),
                          pass == 2 ? nullptr : dcirc.data(), c.h, c.ds, pass != 1, pass, grad.data(), gv.data(),
                          o.dpos.data(), o.dvel.data(), o.rs.data(), o.fl.data());
  });
  return finished("%zu rays, %lld failed, checksum %llu", n, o.nf, o.sum);
}
#endif

// ---- ray paths ---------------------------------------------------------------------------------------------------------
// One body under path_host_* (VEL false: trace_path_ray / path_backtrace_ray, the header's calls without the velocity
// series) and phase_host_* (VEL true: trace_phase_ray / phase_backtrace_ray, vpath beside path and dvpath beside dpath).
template <bool VEL>
static int path_trace(const float* rif, const int* res, size_t n, const float* pos, const float* vel, float h, float ds,
                      int stride, int samples, float* xt, float* vt, float* path, float* vpath, int32_t* count,
                      uint32_t* steps, long long* n_failed) {
  if (stride < 1 || samples < 1) return 1;
  const Call c(rif, res, h, ds);
  return trace_rays(n, pos, vel, xt, vt, steps, n_failed, [&](size_t i, const float* p, const float* v) {
    auto put = [&](float* series, unsigned j, float x, float y, float z) {
      float* q = series + ((size_t)j * n + i) * 3;
      q[0] = x; q[1] = y; q[2] = z;
    };
    auto store = [&](unsigned j, float x, float y, float z) { put(path, j, x, y, z); };
    auto both = [&](unsigned j, float x, float y, float z, float vx, float vy, float vz) {
      put(path, j, x, y, z);
      put(vpath, j, vx, vy, vz);
    };
    const unsigned S = (unsigned)stride, M = (unsigned)samples;
    unsigned cnt = 0;
    const RayOut r = VEL ? trace_phase_ray(c.V, ds, c.max_steps, p, v, S, M, c.taps, both, cnt)
                         : trace_path_ray(c.V, ds, c.max_steps, p, v, S, M, c.taps, store, cnt);
    count[i] = (int32_t)cnt;
    return r;
  });
}

template <bool VEL>
static int path_backtrace(const float* rif, const int* res, size_t n, const float* pos, const float* vel, const float* xt,
                          const float* vt, const uint32_t* fsteps, const float* dx, const float* dv, const float* dpath,
                          const float* dvpath, float h, float ds, int stride, int samples, int corrected_h, double* grad,
                          float* dpos, float* dvel, uint32_t* rsteps, uint8_t* failed) {
  if (stride < 1 || samples < 1) return 1;
  const Call c(rif, res, h, ds, corrected_h);
  const SplatSink sink = zeroed<SplatSink>(grad, c.nvox);
  const float zero[3] = {0.f, 0.f, 0.f};
  return backtrace_rays(n, dx, dv, dpos, dvel, rsteps, failed, [&](size_t i, const float* gx, const float* gv) {
    auto read = [&](const float* series, unsigned j, float* g) {       // -> whether there is such a seed; zeros if not
      const float* q = series ? series + ((size_t)j * n + i) * 3 : zero;
      g[0] = q[0]; g[1] = q[1]; g[2] = q[2];
      return series != nullptr;
    };
    auto seed = [&](unsigned j, float* g) { read(dpath, j, g); };
    auto vseed = [&](unsigned j, float* g) { return read(dvpath, j, g); };
    const float *p0 = pos + 3 * i, *v0 = vel + 3 * i, *xe = xt + 3 * i, *ve = vt + 3 * i;
    const unsigned S = (unsigned)stride, M = (unsigned)samples;
    return VEL ? phase_backtrace_ray(c.V, ds, c.grad_scale, c.max_steps, fsteps[i], p0, v0, xe, ve, gx, gv, S, M, seed, vseed,
                                     c.taps, sink)
               : path_backtrace_ray(c.V, ds, c.grad_scale, c.max_steps, fsteps[i], p0, v0, xe, ve, gx, gv, S, M, seed, c.taps,
                                    sink);
  });
}

// stride, samples >= 1.  xt, vt: (n,3); path, vpath: (samples, n, 3); count, steps: n; *n_failed as in drrt_stats
EXPORT int path_host_trace(const float* rif, const int* res, size_t n, const float* pos, const float* vel, float h, float ds,
                           int stride, int samples, float* xt, float* vt, float* path, int32_t* count, uint32_t* steps,
                           long long* n_failed) {
  return path_trace<false>(rif, res, n, pos, vel, h, ds, stride, samples, xt, vt, path, nullptr, count, steps, n_failed);
}
EXPORT int phase_host_trace(const float* rif, const int* res, size_t n, const float* pos, const float* vel, float h, float ds,
                            int stride, int samples, float* xt, float* vt, float* path, float* vpath, int32_t* count,
                            uint32_t* steps, long long* n_failed) {
  return path_trace<true>(rif, res, n, pos, vel, h, ds, stride, samples, xt, vt, path, vpath, count, steps, n_failed);
}

// dx, dv, dpath, dvpath: nullable (zeros; a null dvpath is no seed at all).  grad: double[nvox], zeroed here.  dpos, dvel:
// (n,3); rsteps (reverse iterations), failed: n each.
EXPORT int path_host_backtrace(const float* rif, const int* res, size_t n, const float* pos, const float* vel,
                               const float* xt, const float* vt, const uint32_t* fsteps, const float* dx, const float* dv,
                               const float* dpath, float h, float ds, int stride, int samples, int corrected_h, double* grad,
                               float* dpos, float* dvel, uint32_t* rsteps, uint8_t* failed) {
  return path_backtrace<false>(rif, res, n, pos, vel, xt, vt, fsteps, dx, dv, dpath, nullptr, h, ds, stride, samples,
                               corrected_h, grad, dpos, dvel, rsteps, failed);
}
EXPORT int phase_host_backtrace(const float* rif, const int* res, size_t n, const float* pos, const float* vel,
                                const float* xt, const float* vt, const uint32_t* fsteps, const float* dx, const float* dv,
                                const float* dpath, const float* dvpath, float h, float ds, int stride, int samples,
                                int corrected_h, double* grad, float* dpos, float* dvel, uint32_t* rsteps, uint8_t* failed) {
  return path_backtrace<true>(rif, res, n, pos, vel, xt, vt, fsteps, dx, dv, dpath, dvpath, h, ds, stride, samples,
                              corrected_h, grad, dpos, dvel, rsteps, failed);
}

#if defined(PATH_MAIN) || defined(PHASE_MAIN)
// The case file: int32 W, H, D, n, stride, samples; float32 h, ds; then float32 arrays rif[W*H*D], pos, vel, dx, dv (n*3
// each), dpath[samples*n*3] and, with -DPHASE_MAIN, dvpath[samples*n*3].  n = 0 is a case.
int main(int argc, char** argv) {
#ifdef PHASE_MAIN
  constexpr bool VEL = true;
#else
  constexpr bool VEL = false;
#endif
  CaseFile c(argc, argv, 6);
  const size_t n = c.n, m = (size_t)c.hd[5];
  const std::vector<float> rif = c.floats(c.nvox), pos = c.floats(3 * n), vel = c.floats(3 * n), dx = c.floats(3 * n),
                           dv = c.floats(3 * n), dpath = c.floats(m * n * 3), dvpath = c.floats(VEL ? m * n * 3 : 0);
  if (!c.ok) return 2;
  RayRun o(n);
  std::vector<float> path(m * n * 3), vpath(VEL ? m * n * 3 : 0);
  std::vector<int32_t> cnt(n);
  std::vector<double> grad(c.nvox);
  if (path_trace<VEL>(rif.data(), c.hd, n, pos.data(), vel.data(), c.h, c.ds, c.hd[4], c.hd[5], o.xt.data(), o.vt.data(),
                      path.data(), vpath.data(), cnt.data(), o.st.data(), &o.nf)) return 2;
  // all seeds, flag on; no seeds on the rays (PHASE_MAIN: nor on path), flag off; no dpath (PHASE_MAIN: no dvpath)
  o.three_passes([&](int pass) {
    path_backtrace<VEL>(rif.data(), c.hd, n, pos.data(), vel.data(), o.xt.data(), o.vt.data(), o.st.data(),
                        pass == 1 ? nullptr : dx.data(), pass == 1 ? nullptr : dv.data(),
                        pass == (VEL ? 1 : 2) ? nullptr : dpath.data(), pass == 2 ? nullptr : dvpath.data(), c.h, c.ds,
                        c.hd[4], c.hd[5], pass != 1, grad.data(), o.dpos.data(), o.dvel.data(), o.rs.data(), o.fl.data());
  });
  for (size_t i = 0; i < n; ++i) o.sum += (unsigned)cnt[i];
  return finished("%zu rays, %lld failed, checksum %llu", n, o.nf, o.sum);
}
#endif
