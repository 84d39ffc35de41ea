// drrt_emission.hip -- gfx950 kernels of emission with self-absorption along the bent ray: drrt_trace_emission_f32 (trace,
// plus rad = sum T_k ds n_k e_k with T_k = exp_neg(tau_k) the transmittance in front of sample k, and tau = sum ds n_k a_k,
// e_k / a_k the emission / absorption fields at the cell and weights of n_k) and drrt_backtrace_emission_f32 (its adjoint:
// dL/dn, dL/de, dL/da, dL/dpos and dL/dvel from seeds on (xt, vt, rad, tau) in ONE reverse march).  Not in the reference.
// Per-ray arithmetic: exp_neg / trace_emission_ray / emission_backtrace_ray of drrt_device.h, which
// tests/hostcheck/emission_rays.hip runs on the host; shared pieces: drrt_march.h.
//
// One ray per lane, everything in registers, as drrt_field.hip: the taps of n go through OplTaps (pair copy or plain grid),
// those of the two fields through one FieldTaps each (plain gathers of the field itself, kept while the lane stays in a
// strictly interior cell).
//
// The adjoint scatters into each grid with HeldCorners (one global fp32 atomic per tap and per run of samples in one
// cell), one instance per grid.  The kernel is instantiated per subset of the three grids scattered, so that a call asking
// for one grid carries only that grid's eight corner sums.  No LDS window, as for the optical path length.
#include "drrt_march.h"

namespace drrt {

template <bool PAIR>
__global__ void __launch_bounds__(kBlock) k_trace_emission(EmissionTraceArgs a) {
  const Vol& V = a.vol;
  const size_t t = (size_t)xcd_block(blockIdx.x, gridDim.x, a.xcd_order ? kXcdRuns16 : kXcdOff) * kBlock + threadIdx.x;
  const TapRows R = tap_rows<PAIR>(V);
  unsigned steps = 0, failed = 0;
  size_t i;
  if (ray_index(a.perm, t, a.n, i)) {
    const Ray3 p = ld3(a.pos, i), u = ld3(a.vel, i);
    const float p0[3] = {p.x, p.y, p.z}, v0[3] = {u.x, u.y, u.z};
    OplTaps<PAIR> taps(V, R);
    FieldTaps etaps(a.emission), ataps(a.absorption);
    float rad, tau;
    const RayOut r = trace_emission_ray(V, a.ds, a.max_steps, p0, v0, taps, etaps, ataps, rad, tau);
    steps = r.steps; failed = r.act ? 1u : 0u;
    st3(a.xt, i, r.xt[0], r.xt[1], r.xt[2]);
    st3(a.vt, i, r.vt[0], r.vt[1], r.vt[2]);
    a.rad[i] = rad;
    a.tau[i] = tau;
    a.steps_out[i] = r.steps;
  }
  block_stats(a.stats, steps, failed);
}

// GRID / EMIS / ABSB: dL/dn / dL/de / dL/da is scattered (a.grad / a.grad_emission / a.grad_absorption is not null)
template <bool PAIR, bool GRID, bool EMIS, bool ABSB>
__global__ void __launch_bounds__(kBlock) k_backtrace_emission(EmissionBackArgs a) {
  const Vol& V = a.vol;
  const size_t t = (size_t)xcd_block(blockIdx.x, gridDim.x, a.xcd_order ? kXcdRuns16 : kXcdOff) * kBlock + threadIdx.x;
  const TapRows R = tap_rows<PAIR>(V);
  unsigned steps = 0, failed = 0;
  size_t i;
  if (ray_index(a.perm, t, a.n, i)) {
    const Ray3 zero{0.f, 0.f, 0.f};
    const Ray3 p = ld3(a.pos, i), u = ld3(a.vel, i), xe = ld3(a.xt, i), ve = ld3(a.vt, i);
    const Ray3 gx = a.dx ? ld3(a.dx, i) : zero, gv = a.dv ? ld3(a.dv, i) : zero;
    const float p0[3] = {p.x, p.y, p.z}, v0[3] = {u.x, u.y, u.z}, xt[3] = {xe.x, xe.y, xe.z}, vt[3] = {ve.x, ve.y, ve.z};
    const float dx[3] = {gx.x, gx.y, gx.z}, dv[3] = {gv.x, gv.y, gv.z};
    const float drad = a.drad ? a.drad[i] : 0.f, dtau = a.dtau ? a.dtau[i] : 0.f;
    OplTaps<PAIR> taps(V, R);
    FieldTaps etaps(a.emission), ataps(a.absorption);
    HeldCorners acc(a.grad), eacc(a.grad_emission), aacc(a.grad_absorption);
    const RayGrad g = emission_backtrace_ray(V, a.ds, a.grad_scale, a.max_steps, a.fsteps[i], p0, v0, xt, vt, a.tau[i], dx, dv,
      drad, dtau, taps, etaps, ataps,
      [&](const Cell& c, float val, float sx, float sy, float sz) {
        if (GRID) acc.add(c, splat_weights(c.wx, c.wy, c.wz, val, sx, sy, sz));
      },
      [&](const Cell& c, float val) {
        if (EMIS) eacc.add(c, value_weights(c.wx, c.wy, c.wz, val));
      },
      [&](const Cell& c, float val) {
        if (ABSB) aacc.add(c, value_weights(c.wx, c.wy, c.wz, val));
      });
    if (GRID) acc.flush();
    if (EMIS) eacc.flush();
    if (ABSB) aacc.flush();
    steps = g.steps; failed = g.failed ? 1u : 0u;
    if (a.dpos) {
      st3(a.dpos, i, g.dp[0], g.dp[1], g.dp[2]);
      st3(a.dvel, i, g.dv[0], g.dv[1], g.dv[2]);
    }
  }
  block_stats(a.stats, steps, failed);
}

void launch_trace_emission(const EmissionTraceArgs& a, hipStream_t s) {
  const dim3 g(grid_for(a.n)), b(kBlock);
  if (a.vol.pair != nullptr) hipLaunchKernelGGL(k_trace_emission<true>, g, b, 0, s, a);
  else                       hipLaunchKernelGGL(k_trace_emission<false>, g, b, 0, s, a);
}

template <bool PAIR, bool GRID, bool EMIS>
static void launch_backtrace_emission_a(const EmissionBackArgs& a, hipStream_t s) {
  const dim3 g(grid_for(a.n)), b(kBlock);
  if (a.grad_absorption != nullptr) hipLaunchKernelGGL((k_backtrace_emission<PAIR, GRID, EMIS, true>), g, b, 0, s, a);
  else                              hipLaunchKernelGGL((k_backtrace_emission<PAIR, GRID, EMIS, false>), g, b, 0, s, a);
}

template <bool PAIR>
static void launch_backtrace_emission_p(const EmissionBackArgs& a, hipStream_t s) {
  const bool grid = a.grad != nullptr, emis = a.grad_emission != nullptr;
  if (grid && emis) launch_backtrace_emission_a<PAIR, true, true>(a, s);
  else if (grid)    launch_backtrace_emission_a<PAIR, true, false>(a, s);
  else if (emis)    launch_backtrace_emission_a<PAIR, false, true>(a, s);
  else              launch_backtrace_emission_a<PAIR, false, false>(a, s);
}

void launch_backtrace_emission(const EmissionBackArgs& a, hipStream_t s) {
  if (a.vol.pair != nullptr) launch_backtrace_emission_p<true>(a, s);
  else                       launch_backtrace_emission_p<false>(a, s);
}

}  // namespace drrt
