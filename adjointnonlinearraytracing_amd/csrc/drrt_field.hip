// drrt_field.hip -- gfx950 kernels of the line integral of a second field along the bent ray: drrt_trace_field_f32 (trace,
// plus tau = sum ds n_k a_k over the samples the march takes anyway, a_k the field at the cell and weights of n_k) and
// drrt_backtrace_field_f32 (its adjoint: dL/dn, dL/dfield, dL/dpos and dL/dvel from seeds on (xt, vt, tau) in ONE reverse
// march).  Not in the reference.  Per-ray arithmetic: trace_field_ray / field_backtrace_ray of drrt_device.h, which
// tests/hostcheck/field_rays.hip runs on the host; shared pieces: drrt_march.h.
//
// One ray per lane, everything in registers, as drrt_opl.hip: the taps of n go through OplTaps (pair copy or plain grid),
// those of the field are plain gathers of the field itself -- there is no pair copy of it -- and both are kept while the
// lane stays in a strictly interior cell.
//
// The adjoint scatters into each grid with HeldCorners (one global fp32 atomic per tap and per run of samples in one
// cell), one instance per grid.  The kernel is instantiated per set of grids scattered, so that a call asking for one grid
// does not carry the other's eight corner sums.  No LDS window, as for the optical path length.
// FieldTaps lives in drrt_march.h: drrt_emission.hip uses it too.
#include "drrt_march.h"

namespace drrt {

template <bool PAIR>
__global__ void __launch_bounds__(kBlock) k_trace_field(FieldTraceArgs a) {
  const Vol& V = a.vol;
  const size_t t = (size_t)xcd_block(blockIdx.x, gridDim.x, a.xcd_order ? kXcdRuns16 : kXcdOff) * kBlock + threadIdx.x;
  const TapRows R = tap_rows<PAIR>(V);
  unsigned steps = 0, failed = 0;
  size_t i;
  if (ray_index(a.perm, t, a.n, i)) {
    const Ray3 p = ld3(a.pos, i), u = ld3(a.vel, i);
    const float p0[3] = {p.x, p.y, p.z}, v0[3] = {u.x, u.y, u.z};
    OplTaps<PAIR> taps(V, R);
    FieldTaps ftaps(a.field);
    float tau;
    const RayOut r = trace_field_ray(V, a.ds, a.max_steps, p0, v0, taps, ftaps, tau);
    steps = r.steps; failed = r.act ? 1u : 0u;
    st3(a.xt, i, r.xt[0], r.xt[1], r.xt[2]);
    st3(a.vt, i, r.vt[0], r.vt[1], r.vt[2]);
    a.tau[i] = tau;
    a.steps_out[i] = r.steps;
  }
  block_stats(a.stats, steps, failed);
}

// GRID / FIELD: dL/dn / dL/dfield is scattered (a.grad / a.grad_field is not null)
template <bool PAIR, bool GRID, bool FIELD>
__global__ void __launch_bounds__(kBlock) k_backtrace_field(FieldBackArgs a) {
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
    const float dtau = a.dtau ? a.dtau[i] : 0.f;
    OplTaps<PAIR> taps(V, R);
    FieldTaps ftaps(a.field);
    HeldCorners acc(a.grad), facc(a.grad_field);
    const RayGrad g = field_backtrace_ray(V, a.ds, a.grad_scale, a.max_steps, a.fsteps[i], p0, v0, xt, vt, dx, dv, dtau, taps,
      ftaps,
      [&](const Cell& c, float val, float sx, float sy, float sz) {
        if (GRID) acc.add(c, splat_weights(c.wx, c.wy, c.wz, val, sx, sy, sz));
      },
      [&](const Cell& c, float val) {
        if (FIELD) facc.add(c, value_weights(c.wx, c.wy, c.wz, val));
      });
    if (GRID) acc.flush();
    if (FIELD) facc.flush();
    steps = g.steps; failed = g.failed ? 1u : 0u;
    if (a.dpos) {
      st3(a.dpos, i, g.dp[0], g.dp[1], g.dp[2]);
      st3(a.dvel, i, g.dv[0], g.dv[1], g.dv[2]);
    }
  }
  block_stats(a.stats, steps, failed);
}

void launch_trace_field(const FieldTraceArgs& a, hipStream_t s) {
  const dim3 g(grid_for(a.n)), b(kBlock);
  if (a.vol.pair != nullptr) hipLaunchKernelGGL(k_trace_field<true>, g, b, 0, s, a);
  else                       hipLaunchKernelGGL(k_trace_field<false>, g, b, 0, s, a);
}

template <bool PAIR>
static void launch_backtrace_field_p(const FieldBackArgs& a, hipStream_t s) {
  const dim3 g(grid_for(a.n)), b(kBlock);
  const bool grid = a.grad != nullptr, field = a.grad_field != nullptr;
  if (grid && field) hipLaunchKernelGGL((k_backtrace_field<PAIR, true, true>), g, b, 0, s, a);
  else if (grid)     hipLaunchKernelGGL((k_backtrace_field<PAIR, true, false>), g, b, 0, s, a);
  else if (field)    hipLaunchKernelGGL((k_backtrace_field<PAIR, false, true>), g, b, 0, s, a);
  else               hipLaunchKernelGGL((k_backtrace_field<PAIR, false, false>), g, b, 0, s, a);
}

void launch_backtrace_field(const FieldBackArgs& a, hipStream_t s) {
  if (a.vol.pair != nullptr) launch_backtrace_field_p<true>(a, s);
  else                       launch_backtrace_field_p<false>(a, s);
}

}  // namespace drrt
