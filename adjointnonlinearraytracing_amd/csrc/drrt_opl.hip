// drrt_opl.hip -- gfx950 kernels of the optical path length: drrt_trace_opl_f32 (trace, plus opl = sum ds n_k^2 over the
// samples the march takes anyway) and drrt_backtrace_opl_f32 (its adjoint: dL/dn, dL/dpos and dL/dvel from seeds on
// (xt, vt, opl) in ONE reverse march).  Not in the reference.  Per-ray arithmetic: trace_opl_ray / opl_backtrace_ray of
// drrt_device.h, which tests/hostcheck/opl_rays.hip runs on the host; shared pieces: drrt_march.h.
//
// One ray per lane, everything in registers, as drrt_adjoint_rays.hip: a lane keeps the taps of a strictly interior cell
// while it stays in it; boundary cells are fetched with their clamps (fetch of drrt_device.h).
//
// The adjoint scatters with one global fp32 atomic per tap, like k_backtrace_direct, with one refinement: a lane keeps the
// eight corner sums of its cell in registers while consecutive samples fall in the same cell, and flushes them when the
// cell changes and after its last iteration (with ds = h / 2 that roughly halves the atomics).  There is NO LDS window: the
// ring kernel's fixed-point window is scaled for backtrace's contributions and a per-step source term does not fit its
// overflow budget, so this kernel pays the memory-side atomic rate where many rays cross the same voxels.
#include "drrt_march.h"

namespace drrt {

// the taps of cell c for the lane: gathered through R, kept while the lane stays in a strictly interior cell
template <bool PAIR>
struct OplTaps {
  const Vol& V;
  const TapRows& R;
  unsigned off = 0;          // byte offset (tap_offset) of the interior cell whose taps the lane holds
  bool held = false;
  f4 q0 = f4{0.f, 0.f, 0.f, 0.f}, q1 = f4{0.f, 0.f, 0.f, 0.f};
  __device__ __forceinline__ OplTaps(const Vol& v, const TapRows& r) : V(v), R(r) {}
  __device__ __forceinline__ Taps operator()(const Cell& c) {
    if (!c.interior) { held = false; return fetch(V.data, c); }
    const unsigned noff = tap_offset<PAIR>(c.base);
    if (!(held & (noff == off))) { gather_rows<PAIR>(R, noff, q0, q1); off = noff; held = true; }
    return taps_of<PAIR>(q0, q1);
  }
};

template <bool PAIR>
__global__ void __launch_bounds__(kBlock) k_trace_opl(OplTraceArgs a) {
  const Vol& V = a.vol;
  const size_t t = (size_t)xcd_block(blockIdx.x, gridDim.x, a.xcd_order ? kXcdRuns16 : kXcdOff) * kBlock + threadIdx.x;
  const TapRows R = tap_rows<PAIR>(V);
  unsigned steps = 0, failed = 0;
  size_t i;
  if (ray_index(a.perm, t, a.n, i)) {
    const Ray3 p = ld3(a.pos, i), u = ld3(a.vel, i);
    const float p0[3] = {p.x, p.y, p.z}, v0[3] = {u.x, u.y, u.z};
    OplTaps<PAIR> taps(V, R);
    float opl;
    const RayOut r = trace_opl_ray(V, a.ds, a.max_steps, p0, v0, taps, opl);
    steps = r.steps; failed = r.act ? 1u : 0u;
    st3(a.xt, i, r.xt[0], r.xt[1], r.xt[2]);
    st3(a.vt, i, r.vt[0], r.vt[1], r.vt[2]);
    a.opl[i] = opl;
    a.steps_out[i] = r.steps;
  }
  block_stats(a.stats, steps, failed);
}

// The eight corner sums of the cell the lane is in.  Two cells with the same corner 000 and the same (clamp) offsets have
// the same eight addresses, so that is the test for "the same cell".
struct HeldCorners {
  float* grad;
  int base = -1, ox = 0, oy = 0, oz = 0;     // base < 0: nothing held
  Corners s;
  __device__ __forceinline__ explicit HeldCorners(float* g) : grad(g) {}
  __device__ __forceinline__ void flush() {
    if (base < 0) return;
    float* g = grad + base;
    atomic_add_f32(g, s.c000);                atomic_add_f32(g + ox, s.c100);
    atomic_add_f32(g + oy, s.c010);           atomic_add_f32(g + oy + ox, s.c110);
    atomic_add_f32(g + oz, s.c001);           atomic_add_f32(g + oz + ox, s.c101);
    atomic_add_f32(g + oz + oy, s.c011);      atomic_add_f32(g + oz + oy + ox, s.c111);
    base = -1;
  }
  __device__ __forceinline__ void add(const Cell& c, const Corners& w) {
    if ((c.base == base) & (c.ox == ox) & (c.oy == oy) & (c.oz == oz)) {
      s.c000 += w.c000; s.c100 += w.c100; s.c010 += w.c010; s.c110 += w.c110;
      s.c001 += w.c001; s.c101 += w.c101; s.c011 += w.c011; s.c111 += w.c111;
      return;
    }
    flush();
    s = w; base = c.base; ox = c.ox; oy = c.oy; oz = c.oz;
  }
};

template <bool PAIR>
__global__ void __launch_bounds__(kBlock) k_backtrace_opl(OplBackArgs a) {
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
    const float dopl = a.dopl ? a.dopl[i] : 0.f;
    OplTaps<PAIR> taps(V, R);
    HeldCorners acc(a.grad);
    const bool scatter = a.grad != nullptr;
    const RayGrad g = opl_backtrace_ray(V, a.ds, a.grad_scale, a.max_steps, a.fsteps[i], p0, v0, xt, vt, dx, dv, dopl, taps,
      [&](const Cell& c, float val, float sx, float sy, float sz) {
        if (scatter) acc.add(c, splat_weights(c.wx, c.wy, c.wz, val, sx, sy, sz));
      });
    acc.flush();
    steps = g.steps; failed = g.failed ? 1u : 0u;
    if (a.dpos) {
      st3(a.dpos, i, g.dp[0], g.dp[1], g.dp[2]);
      st3(a.dvel, i, g.dv[0], g.dv[1], g.dv[2]);
    }
  }
  block_stats(a.stats, steps, failed);
}

void launch_trace_opl(const OplTraceArgs& a, hipStream_t s) {
  const dim3 g(grid_for(a.n)), b(kBlock);
  if (a.vol.pair != nullptr) hipLaunchKernelGGL(k_trace_opl<true>, g, b, 0, s, a);
  else                       hipLaunchKernelGGL(k_trace_opl<false>, g, b, 0, s, a);
}

void launch_backtrace_opl(const OplBackArgs& a, hipStream_t s) {
  const dim3 g(grid_for(a.n)), b(kBlock);
  if (a.vol.pair != nullptr) hipLaunchKernelGGL(k_backtrace_opl<true>, g, b, 0, s, a);
  else                       hipLaunchKernelGGL(k_backtrace_opl<false>, g, b, 0, s, a);
}

}  // namespace drrt
