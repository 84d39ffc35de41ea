// drrt_integral.hip -- gfx950 kernels of the integral operators: trace with a line integral over the samples the march takes
// anyway, and the adjoint that returns every gradient from seeds on all outputs in ONE reverse march.  Not in the reference.
//   drrt_trace_opl_f32 / drrt_backtrace_opl_f32            opl = sum ds n_k^2; dL/dn, dL/dpos, dL/dvel from seeds on
//                                                          (xt, vt, opl)
//   drrt_trace_field_f32 / drrt_backtrace_field_f32        tau = sum ds n_k a_k, a_k a second field at the cell and weights
//                                                          of n_k; dL/dn, dL/dfield and the ray gradients from (xt, vt, tau)
//   drrt_trace_emission_f32 / drrt_backtrace_emission_f32  rad = sum T_k ds n_k e_k with T_k = exp_neg(tau_k) the
//                                                          transmittance in front of sample k, and tau = sum ds n_k a_k;
//                                                          dL/dn, dL/de, dL/da and the ray gradients from (xt, vt, rad, tau)
//   drrt_trace_vector_f32 / drrt_backtrace_vector_f32      circ = sum ds u_k . v_{k+1}, u_k a vector field (three planes) at
//                                                          the cell and weights of n_k, v_{k+1} the velocity behind the
//                                                          step; dL/dn, the three planes of dL/du and the ray gradients
//                                                          from (xt, vt, circ)
//   drrt_trace_path_f32 / drrt_backtrace_path_f32          path = every stride-th marching position, padded with xt: the
//                                                          first operator whose per-ray output is a series; dL/dn and the
//                                                          ray gradients from (xt, vt, path)
//   drrt_trace_phase_f32 / drrt_backtrace_phase_f32        the path entries with vpath beside path: the marching velocity
//                                                          at every sample, padded with vt, so that (path[j], vpath[j]) is
//                                                          the march's state; dL/dn and the ray gradients from
//                                                          (xt, vt, path, vpath).  The same routine and lane bodies as the
//                                                          path entries, which are these with the velocity series absent
// Per-ray arithmetic: trace_integral_ray / integral_backtrace_ray of drrt_device.h with each operator's integrand and term
// (trace_opl_ray ... phase_backtrace_ray), which tests/hostcheck/integral_rays.hip runs on the host; shared pieces:
// drrt_march.h.
//
// One ray per lane, everything in registers, as drrt_ray_adjoints.hip: the taps of n go through HeldTaps (pair copy or plain
// grid), those of a further field through one FieldTaps each (plain gathers of the field itself -- there is no pair copy
// of it); both are kept while the lane stays in a strictly interior cell, and boundary cells are fetched with their clamps
// (fetch of drrt_device.h).
//
// The adjoints scatter with one global fp32 atomic per tap, like k_backtrace_direct, with one refinement: per grid a lane
// keeps the eight corner sums of its cell in registers (HeldCorners) while consecutive samples fall in the same cell, and
// flushes them when the cell changes and after its last iteration (with ds = h / 2 that roughly halves the atomics).  The
// field and emission adjoints are instantiated per subset of the grids scattered, so that a call asking for one grid
// carries only that grid's corner sums.  There is NO LDS window: the ring kernel's fixed-point window is scaled for
// backtrace's contributions and a per-step source term does not fit its overflow budget, so these kernels pay the
// memory-side atomic rate where many rays cross the same voxels.
#include "drrt_march.h"

namespace drrt {

// What the forward kernels share: the lane's ray, its march and its stores.  `march(i, p0, v0, taps)` -> RayOut runs the
// operator's routine on ray i, `store(i)` writes the operator's own per-ray outputs.
template <bool PAIR, typename Args, typename March, typename Store>
__device__ __forceinline__ void trace_lanes(const Args& a, March&& march, Store&& store) {
  const Vol& V = a.vol;
  const size_t t = (size_t)xcd_block(blockIdx.x, gridDim.x, a.xcd_order ? kXcdRuns16 : kXcdOff) * kBlock + threadIdx.x;
  const TapRows R = tap_rows<PAIR>(V);
  unsigned steps = 0, failed = 0;
  size_t i;
  if (ray_index(a.perm, t, a.n, i)) {
    const Ray3 p = ld3(a.pos, i), u = ld3(a.vel, i);
    const float p0[3] = {p.x, p.y, p.z}, v0[3] = {u.x, u.y, u.z};
    HeldTaps<PAIR> taps(V, R);
    const RayOut r = march(i, p0, v0, taps);
    steps = r.steps; failed = r.act ? 1u : 0u;
    st3(a.xt, i, r.xt[0], r.xt[1], r.xt[2]);
    st3(a.vt, i, r.vt[0], r.vt[1], r.vt[2]);
    store(i);
    a.steps_out[i] = r.steps;
  }
  block_stats(a.stats, steps, failed);
}

// What the adjoint kernels share: the lane's forward ray and seeds (null seeds read as zeros), its reverse march, and the
// store of the ray gradients (when asked for).  `march(i, r, taps)` -> RayGrad runs the operator's routine with its own
// seeds and sinks.
struct AdjRay { float p0[3], v0[3], xt[3], vt[3], dx[3], dv[3]; unsigned K; };

template <bool PAIR, typename Args, typename March>
__device__ __forceinline__ void backtrace_lanes(const Args& a, March&& march) {
  const Vol& V = a.vol;
  const size_t t = (size_t)xcd_block(blockIdx.x, gridDim.x, a.xcd_order ? kXcdRuns16 : kXcdOff) * kBlock + threadIdx.x;
  const TapRows R = tap_rows<PAIR>(V);
  unsigned steps = 0, failed = 0;
  size_t i;
  if (ray_index(a.perm, t, a.n, i)) {
    const Ray3 zero{0.f, 0.f, 0.f};
    const Ray3 p = ld3(a.pos, i), u = ld3(a.vel, i), xe = ld3(a.xt, i), ve = ld3(a.vt, i);
    const Ray3 gx = a.dx ? ld3(a.dx, i) : zero, gv = a.dv ? ld3(a.dv, i) : zero;
    const AdjRay r{{p.x, p.y, p.z}, {u.x, u.y, u.z}, {xe.x, xe.y, xe.z}, {ve.x, ve.y, ve.z}, {gx.x, gx.y, gx.z},
                   {gv.x, gv.y, gv.z}, a.fsteps[i]};
    HeldTaps<PAIR> taps(V, R);
    const RayGrad g = march(i, r, taps);
    steps = g.steps; failed = g.failed ? 1u : 0u;
    if (a.dpos) {
      st3(a.dpos, i, g.dp[0], g.dp[1], g.dp[2]);
      st3(a.dvel, i, g.dv[0], g.dv[1], g.dv[2]);
    }
  }
  block_stats(a.stats, steps, failed);
}

// the sinks of the reverse march: a contribution to dL/dn (value and gradient splat) / to a further grid (value weights)
template <bool ON>
struct SplatSink {
  HeldCorners& acc;
  __device__ __forceinline__ void operator()(const Cell& c, float val, float sx, float sy, float sz) {
    if (ON) acc.add(c, splat_weights(c.wx, c.wy, c.wz, val, sx, sy, sz));
  }
};
template <bool ON>
struct ValueSink {
  HeldCorners& acc;
  __device__ __forceinline__ void operator()(const Cell& c, float val) {
    if (ON) acc.add(c, value_weights(c.wx, c.wy, c.wz, val));
  }
};

// ---- optical path length ---------------------------------------------------------------------------------------------
template <bool PAIR>
__global__ void __launch_bounds__(kBlock) k_trace_opl(OplTraceArgs a) {
  float opl;
  trace_lanes<PAIR>(a,
    [&](size_t, const float* p0, const float* v0, HeldTaps<PAIR>& taps) {
      return trace_opl_ray(a.vol, a.ds, a.max_steps, p0, v0, taps, opl);
    },
    [&](size_t i) { a.opl[i] = opl; });
}

template <bool PAIR>
__global__ void __launch_bounds__(kBlock) k_backtrace_opl(OplBackArgs a) {
  backtrace_lanes<PAIR>(a, [&](size_t i, const AdjRay& r, HeldTaps<PAIR>& taps) {
    const float dopl = a.dopl ? a.dopl[i] : 0.f;
    HeldCorners acc(a.grad);
    const bool scatter = a.grad != nullptr;
    const RayGrad g = opl_backtrace_ray(a.vol, a.ds, a.grad_scale, a.max_steps, r.K, r.p0, r.v0, r.xt, r.vt, r.dx, r.dv, dopl,
      taps, [&](const Cell& c, float val, float sx, float sy, float sz) {
        if (scatter) acc.add(c, splat_weights(c.wx, c.wy, c.wz, val, sx, sy, sz));
      });
    acc.flush();
    return g;
  });
}

// ---- line integral of a second field -----------------------------------------------------------------------------------
template <bool PAIR>
__global__ void __launch_bounds__(kBlock) k_trace_field(FieldTraceArgs a) {
  float tau;
  trace_lanes<PAIR>(a,
    [&](size_t, const float* p0, const float* v0, HeldTaps<PAIR>& taps) {
      FieldTaps ftaps(a.field);
      return trace_field_ray(a.vol, a.ds, a.max_steps, p0, v0, taps, ftaps, tau);
    },
    [&](size_t i) { a.tau[i] = tau; });
}

// GRID / FIELD: dL/dn / dL/dfield is scattered (a.grad / a.grad_field is not null)
template <bool PAIR, bool GRID, bool FIELD>
__global__ void __launch_bounds__(kBlock) k_backtrace_field(FieldBackArgs a) {
  backtrace_lanes<PAIR>(a, [&](size_t i, const AdjRay& r, HeldTaps<PAIR>& taps) {
    const float dtau = a.dtau ? a.dtau[i] : 0.f;
    FieldTaps ftaps(a.field);
    HeldCorners acc(a.grad), facc(a.grad_field);
    SplatSink<GRID> sink{acc};
    ValueSink<FIELD> fsink{facc};
    const RayGrad g = field_backtrace_ray(a.vol, a.ds, a.grad_scale, a.max_steps, r.K, r.p0, r.v0, r.xt, r.vt, r.dx, r.dv,
                                          dtau, taps, ftaps, sink, fsink);
    if (GRID) acc.flush();
    if (FIELD) facc.flush();
    return g;
  });
}

// ---- emission with self-absorption -----------------------------------------------------------------------------------
template <bool PAIR>
__global__ void __launch_bounds__(kBlock) k_trace_emission(EmissionTraceArgs a) {
  float rad, tau;
  trace_lanes<PAIR>(a,
    [&](size_t, const float* p0, const float* v0, HeldTaps<PAIR>& taps) {
      FieldTaps etaps(a.emission), ataps(a.absorption);
      return trace_emission_ray(a.vol, a.ds, a.max_steps, p0, v0, taps, etaps, ataps, rad, tau);
    },
    [&](size_t i) { a.rad[i] = rad; a.tau[i] = tau; });
}

// GRID / EMIS / ABSB: dL/dn / dL/de / dL/da is scattered (a.grad / a.grad_emission / a.grad_absorption is not null)
template <bool PAIR, bool GRID, bool EMIS, bool ABSB>
__global__ void __launch_bounds__(kBlock) k_backtrace_emission(EmissionBackArgs a) {
  backtrace_lanes<PAIR>(a, [&](size_t i, const AdjRay& r, HeldTaps<PAIR>& taps) {
    const float drad = a.drad ? a.drad[i] : 0.f, dtau = a.dtau ? a.dtau[i] : 0.f;
    FieldTaps etaps(a.emission), ataps(a.absorption);
    HeldCorners acc(a.grad), eacc(a.grad_emission), aacc(a.grad_absorption);
    SplatSink<GRID> sink{acc};
    ValueSink<EMIS> esink{eacc};
    ValueSink<ABSB> asink{aacc};
    const RayGrad g = emission_backtrace_ray(a.vol, a.ds, a.grad_scale, a.max_steps, r.K, r.p0, r.v0, r.xt, r.vt, a.tau[i],
                                             r.dx, r.dv, drad, dtau, taps, etaps, ataps, sink, esink, asink);
    if (GRID) acc.flush();
    if (EMIS) eacc.flush();
    if (ABSB) aacc.flush();
    return g;
  });
}

// ---- line integral of a vector field -----------------------------------------------------------------------------------
// the taps of the three component planes: one FieldTaps each, plane k at + k nvox
struct VectorTaps {
  FieldTaps x, y, z;
  __device__ __forceinline__ VectorTaps(const float* u, size_t nvox) : x(u), y(u + nvox), z(u + 2 * nvox) {}
  __device__ __forceinline__ Taps operator()(const Cell& c, int k) { return k == 0 ? x(c) : k == 1 ? y(c) : z(c); }
};
__device__ __forceinline__ size_t plane_size(const Vol& V) { return (size_t)V.sz * (size_t)V.D; }

template <bool PAIR>
__global__ void __launch_bounds__(kBlock) k_trace_vector(VectorTraceArgs a) {
  float circ;
  trace_lanes<PAIR>(a,
    [&](size_t, const float* p0, const float* v0, HeldTaps<PAIR>& taps) {
      VectorTaps vtaps(a.vfield, plane_size(a.vol));
      return trace_vector_ray(a.vol, a.ds, a.max_steps, p0, v0, taps, vtaps, circ);
    },
    [&](size_t i) { a.circ[i] = circ; });
}

// GRID / VFIELD: dL/dn / the three planes of dL/du are scattered (a.grad / a.grad_vfield is not null)
template <bool PAIR, bool GRID, bool VFIELD>
__global__ void __launch_bounds__(kBlock) k_backtrace_vector(VectorBackArgs a) {
  backtrace_lanes<PAIR>(a, [&](size_t i, const AdjRay& r, HeldTaps<PAIR>& taps) {
    const float dcirc = a.dcirc ? a.dcirc[i] : 0.f;
    const size_t nvox = plane_size(a.vol);
    VectorTaps vtaps(a.vfield, nvox);
    HeldCorners acc(a.grad), xacc(a.grad_vfield), yacc(a.grad_vfield + nvox), zacc(a.grad_vfield + 2 * nvox);
    SplatSink<GRID> sink{acc};
    auto vsink = [&](int k, const Cell& c, float val) {
      if (VFIELD) (k == 0 ? xacc : k == 1 ? yacc : zacc).add(c, value_weights(c.wx, c.wy, c.wz, val));
    };
    const RayGrad g = vector_backtrace_ray(a.vol, a.ds, a.grad_scale, a.max_steps, r.K, r.p0, r.v0, r.xt, r.vt, r.dx, r.dv,
                                           dcirc, taps, vtaps, sink, vsink);
    if (GRID) acc.flush();
    if (VFIELD) { xacc.flush(); yacc.flush(); zacc.flush(); }
    return g;
  });
}

// ---- ray paths -----------------------------------------------------------------------------------------------------------
// path is (samples, n, 3), sample-major: entry j of ray i at (j n + i) 3, so that in caller order a wave's 64 stores of one
// sample are one contiguous run of 768 bytes.  Under a visit order (perm) they are 64 scattered 12-byte stores on 1 / stride
// of the iterations; they are not staged (DESIGN.md 6 has what that costs).  vpath is laid out and stored like path, one
// store behind it: in caller order a wave writes one contiguous run of 768 bytes per sample and series.
// VEL: the call carries the velocity series (the phase entries: a.vpath / a.dvpath exist); without it the velocities handed
// to the store are dropped and NoVSeed seeds none, and the compiler removes the series completely.
template <bool VEL, typename Args, typename TapFn>
__device__ __forceinline__ RayOut trace_path_lane(const Args& a, size_t i, const float* p0, const float* v0, TapFn& taps,
                                                  unsigned& count) {
  auto store = [&](unsigned j, float x, float y, float z, float vx, float vy, float vz) {
    const size_t e = (size_t)j * a.n + i;
    st3(a.path, e, x, y, z);
    if constexpr (VEL) st3(a.vpath, e, vx, vy, vz);
  };
  return trace_phase_ray(a.vol, a.ds, a.max_steps, p0, v0, a.stride, a.samples, taps, store, count);
}

// GRID: dL/dn is scattered (a.grad is not null)
template <bool GRID, bool VEL, typename Args, typename TapFn>
__device__ __forceinline__ RayGrad backtrace_path_lane(const Args& a, size_t i, const AdjRay& r, TapFn& taps) {
  auto seed = [&](unsigned j, float* g) {
    const Ray3 zero{0.f, 0.f, 0.f};
    const Ray3 d = a.dpath ? ld3(a.dpath, (size_t)j * a.n + i) : zero;
    g[0] = d.x; g[1] = d.y; g[2] = d.z;
  };
  auto vseed = [&] {
    if constexpr (VEL) {
      return [&a, i](unsigned j, float* g) {
        if (!a.dvpath) return false;
        const Ray3 d = ld3(a.dvpath, (size_t)j * a.n + i);
        g[0] = d.x; g[1] = d.y; g[2] = d.z;
        return true;
      };
    } else {
      return NoVSeed{};
    }
  }();
  HeldCorners acc(a.grad);
  SplatSink<GRID> sink{acc};
  const RayGrad g = phase_backtrace_ray(a.vol, a.ds, a.grad_scale, a.max_steps, r.K, r.p0, r.v0, r.xt, r.vt, r.dx, r.dv,
                                        a.stride, a.samples, seed, vseed, taps, sink);
  if (GRID) acc.flush();
  return g;
}

template <bool PAIR>
__global__ void __launch_bounds__(kBlock) k_trace_path(PathTraceArgs a) {
  unsigned count;
  trace_lanes<PAIR>(a,
    [&](size_t i, const float* p0, const float* v0, HeldTaps<PAIR>& taps) {
      return trace_path_lane<false>(a, i, p0, v0, taps, count);
    },
    [&](size_t i) { a.count[i] = (int)count; });
}
template <bool PAIR>
__global__ void __launch_bounds__(kBlock) k_trace_phase(PhaseTraceArgs a) {
  unsigned count;
  trace_lanes<PAIR>(a,
    [&](size_t i, const float* p0, const float* v0, HeldTaps<PAIR>& taps) {
      return trace_path_lane<true>(a, i, p0, v0, taps, count);
    },
    [&](size_t i) { a.count[i] = (int)count; });
}
template <bool PAIR, bool GRID>
__global__ void __launch_bounds__(kBlock) k_backtrace_path(PathBackArgs a) {
  backtrace_lanes<PAIR>(a, [&](size_t i, const AdjRay& r, HeldTaps<PAIR>& taps) {
    return backtrace_path_lane<GRID, false>(a, i, r, taps);
  });
}
template <bool PAIR, bool GRID>
__global__ void __launch_bounds__(kBlock) k_backtrace_phase(PhaseBackArgs a) {
  backtrace_lanes<PAIR>(a, [&](size_t i, const AdjRay& r, HeldTaps<PAIR>& taps) {
    return backtrace_path_lane<GRID, true>(a, i, r, taps);
  });
}

// ---- launchers ---------------------------------------------------------------------------------------------------------
// which instantiation of a kernel a call gets: with_bools (drrt_march.h)
#define LAUNCH_INTEGRAL(kernel, a, s) hipLaunchKernelGGL(kernel, dim3(grid_for((a).n)), dim3(kBlock), 0, s, a)

void launch_trace_opl(const OplTraceArgs& a, hipStream_t s) {
  with_bools([&](auto pair) { LAUNCH_INTEGRAL(k_trace_opl<decltype(pair)::value>, a, s); }, a.vol.pair != nullptr);
}
void launch_backtrace_opl(const OplBackArgs& a, hipStream_t s) {
  with_bools([&](auto pair) { LAUNCH_INTEGRAL(k_backtrace_opl<decltype(pair)::value>, a, s); }, a.vol.pair != nullptr);
}
void launch_trace_field(const FieldTraceArgs& a, hipStream_t s) {
  with_bools([&](auto pair) { LAUNCH_INTEGRAL(k_trace_field<decltype(pair)::value>, a, s); }, a.vol.pair != nullptr);
}
void launch_backtrace_field(const FieldBackArgs& a, hipStream_t s) {
  with_bools([&](auto pair, auto grid, auto field) {
    LAUNCH_INTEGRAL((k_backtrace_field<decltype(pair)::value, decltype(grid)::value, decltype(field)::value>), a, s);
  }, a.vol.pair != nullptr, a.grad != nullptr, a.grad_field != nullptr);
}
void launch_trace_emission(const EmissionTraceArgs& a, hipStream_t s) {
  with_bools([&](auto pair) { LAUNCH_INTEGRAL(k_trace_emission<decltype(pair)::value>, a, s); }, a.vol.pair != nullptr);
}
void launch_backtrace_emission(const EmissionBackArgs& a, hipStream_t s) {
  with_bools([&](auto pair, auto grid, auto emis, auto absb) {
    LAUNCH_INTEGRAL((k_backtrace_emission<decltype(pair)::value, decltype(grid)::value, decltype(emis)::value,
                                          decltype(absb)::value>), a, s);
  }, a.vol.pair != nullptr, a.grad != nullptr, a.grad_emission != nullptr, a.grad_absorption != nullptr);
}
void launch_trace_vector(const VectorTraceArgs& a, hipStream_t s) {
  with_bools([&](auto pair) { LAUNCH_INTEGRAL(k_trace_vector<decltype(pair)::value>, a, s); }, a.vol.pair != nullptr);
}
void launch_backtrace_vector(const VectorBackArgs& a, hipStream_t s) {
  with_bools([&](auto pair, auto grid, auto vfield) {
    LAUNCH_INTEGRAL((k_backtrace_vector<decltype(pair)::value, decltype(grid)::value, decltype(vfield)::value>), a, s);
  }, a.vol.pair != nullptr, a.grad != nullptr, a.grad_vfield != nullptr);
}
void launch_trace_path(const PathTraceArgs& a, hipStream_t s) {
  with_bools([&](auto pair) { LAUNCH_INTEGRAL(k_trace_path<decltype(pair)::value>, a, s); }, a.vol.pair != nullptr);
}
void launch_backtrace_path(const PathBackArgs& a, hipStream_t s) {
  with_bools([&](auto pair, auto grid) {
    LAUNCH_INTEGRAL((k_backtrace_path<decltype(pair)::value, decltype(grid)::value>), a, s);
  }, a.vol.pair != nullptr, a.grad != nullptr);
}
void launch_trace_phase(const PhaseTraceArgs& a, hipStream_t s) {
  with_bools([&](auto pair) { LAUNCH_INTEGRAL(k_trace_phase<decltype(pair)::value>, a, s); }, a.vol.pair != nullptr);
}
void launch_backtrace_phase(const PhaseBackArgs& a, hipStream_t s) {
  with_bools([&](auto pair, auto grid) {
    LAUNCH_INTEGRAL((k_backtrace_phase<decltype(pair)::value, decltype(grid)::value>), a, s);
  }, a.vol.pair != nullptr, a.grad != nullptr);
}

}  // namespace drrt
