// drrt_device.h -- per-ray building blocks of the gfx950 eikonal ray-march kernels.
//
// What the reference computes (file:line = /root/reference/...):
//   volume::eval_grad  src/volume.cpp:101-181   trilinear n(p) and grad n(p)
//   volume::eval_hess  src/volume.cpp:40-99     mixed second partials (zero diagonal)
//   volume::splat      src/volume.cpp:182-244   adjoint of eval_grad w.r.t. the voxels
//   volume::inbounds / escaped  src/volume.cpp:246-271
//   cylinder_volume::*  src/cylinder_volume.cpp:26-170
//   one forward / adjoint march iteration: src/tracer.cpp:68-86, :420-435
//
// How it is computed here: the 8 taps are fetched once per ray-step and n, grad n and the
// three mixed partials all come from ONE factored lerp tree (differences first, ~27 flops
// instead of the ~150 of the expanded weight products; differences-first also avoids the
// cancellation of the reference's (sum of 4 products) - (sum of 4 products) form); the 16
// scatter_adds of volume::splat are fused into 8 corner contributions.
//
// ARITHMETIC CONTRACT ("factored fp32 spec"): every expression below is an explicit sequence of
// IEEE-754 binary32 operations (+, -, *, fmaf, floorf, sqrtf, /, conversions); the library is
// built with -ffp-contract=off so the compiler adds no fusion of its own.  The CPU oracle's
// `factored` arithmetic mode (oracle/drrt_oracle_impl.h) restates the same sequence in plain C,
// which makes forward trajectories and exit steps comparable BIT FOR BIT between the GPU and the
// oracle (only the order of the adjoint's atomic sums differs).  Functions that need nothing
// device-specific are __host__ __device__ so that tests/hostcheck can run this very code on the
// CPU; the package itself never does (no CPU compute path).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define DRRT_HD __host__ __device__ __forceinline__

namespace drrt {

constexpr int kWave = 64;

struct Vol {
  const float* data;
  int W, H, D;          // res[0], res[1], res[2]  (x, y, z extents; x is memory-contiguous)
  int sy, sz;           // element strides of y and z: W, W*H
  float inv_h;          // 1.0f/h   (reference: rcp(h_), src/volume.cpp:128)
  float inv_h2;         // inv_h*inv_h
  float bx, by, bz;     // (float)(res-1)*h : bounds of inbounds/escaped (src/volume.cpp:252-254)
  unsigned lx, ly, lz;  // res-3 (0 when res < 4): a floor index i with 1 <= i <= res-3 is "strictly interior"
  const float* pair;    // optional (device only): the "pair copy" of the grid, 2 floats per voxel i: {n[i], n[i+sy]}
                        // (clamped at the far y face), built per call by k_build_pair; null = not in use
  float q_min, q_step, q_inv_step;   // 16-bit ray-state positions ("q16", include/drrt_hip.h): p = q_min + code * q_step
};

// ---- 16-bit ray state ("q16"): 6 bytes per 3-vector, like IEEE half, but with the precision where a march needs it ----
// position  unsigned 16-bit code over [-E/16, E + E/16], E = the largest box extent: step = 1.125 E / 65535 (h/228 on a
//           256^3 grid, against h/8 for an IEEE half near 1.0); positions outside the range saturate
// direction signed 16-bit fixed point, step 2^-14 (range [-2, 2): |v| = n stays below 2 for any index below 2)
// seeds     (dx, dv of the adjoint) stay IEEE half: they need relative, not absolute, precision
constexpr float kQ16VelStep = 1.0f / 16384.0f;
DRRT_HD float q16_pos_dec(const Vol& V, uint16_t c) { return fmaf((float)c, V.q_step, V.q_min); }
DRRT_HD uint16_t q16_pos_enc(const Vol& V, float x) {
  float t = (x - V.q_min) * V.q_inv_step;
  t = t > 0.f ? t : 0.f;                       // also NaN -> 0
  t = t < 65535.f ? t : 65535.f;
  return (uint16_t)(int)rintf(t);
}
DRRT_HD float q16_vel_dec(int16_t c) { return (float)c * kQ16VelStep; }
DRRT_HD int16_t q16_vel_enc(float v) {
  float t = v * 16384.0f;
  t = t > -32768.f ? t : -32768.f;             // also NaN -> -32768
  t = t < 32767.f ? t : 32767.f;
  return (int16_t)(int)rintf(t);
}

DRRT_HD void vol_finish(Vol& V, float h) {   // derived fields; data, W, H, D must be set
  V.sy = V.W; V.sz = V.W * V.H; V.pair = nullptr;
  V.inv_h = 1.0f / h; V.inv_h2 = V.inv_h * V.inv_h;
  V.bx = (float)(V.W - 1) * h; V.by = (float)(V.H - 1) * h; V.bz = (float)(V.D - 1) * h;
  V.lx = V.W >= 4 ? (unsigned)(V.W - 3) : 0u; V.ly = V.H >= 4 ? (unsigned)(V.H - 3) : 0u;
  V.lz = V.D >= 4 ? (unsigned)(V.D - 3) : 0u;
  const float ext = fmaxf(V.bx, fmaxf(V.by, V.bz));
  V.q_min = -ext * 0.0625f; V.q_step = (ext * 1.125f) / 65535.0f; V.q_inv_step = 65535.0f / (ext * 1.125f);
}

struct Cell {
  int base;             // flat index of corner 000
  int ix, iy, iz;       // (clamped) integer coordinates of corner 000
  int ox, oy, oz;       // element offsets to the +x, +y, +z neighbours (0 where clamped)
  float wx, wy, wz;     // fractional weights w0 = pm - floor(pm)  (unclamped, Q11)
  bool interior;        // every floor index in [1, res-3]: no clamp acts, the 8 taps are distinct, and
                        // the point is a whole cell away from every face, so whatever the rounding of
                        // p*inv_h: inbounds(p) is true and escaped(p, .) is false
};

DRRT_HD int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// a*b + c for non-negative operands below 2^24 (grid coordinates and strides): v_mad_u32_u24 is a
// full-rate VALU op, the generic 32-bit integer multiply is quarter rate
DRRT_HD int mad24(int a, int b, int c) {
#if defined(__HIP_DEVICE_COMPILE__)
  return (int)(__umul24((unsigned)a, (unsigned)b) + (unsigned)c);
#else
  return a * b + c;
#endif
}

// float -> int with the saturating behaviour of v_cvt_i32_f32 (NaN -> 0), also on the host
DRRT_HD int f2i_sat(float f) {
#if defined(__HIP_DEVICE_COMPILE__)
  return (int)f;
#else
  if (!(f == f)) return 0;
  if (f >= 2147483648.0f) return 2147483647;
  if (f <= -2147483648.0f) return (-2147483647 - 1);
  return (int)f;
#endif
}

// src/volume.cpp:128-141: pm = p*rcp(h); pos = floor2int(pm); w0 = pm - pos; clamp indices.
DRRT_HD Cell locate(const Vol& V, float px, float py, float pz) {
  Cell c;
  float fx = px * V.inv_h, fy = py * V.inv_h, fz = pz * V.inv_h;
  float flx = floorf(fx), fly = floorf(fy), flz = floorf(fz);
  c.wx = fx - flx; c.wy = fy - fly; c.wz = fz - flz;
  int ix = f2i_sat(flx), iy = f2i_sat(fly), iz = f2i_sat(flz);
  c.interior = (((unsigned)ix - 1u) < V.lx) & (((unsigned)iy - 1u) < V.ly) & (((unsigned)iz - 1u) < V.lz);   // wraps, no UB
  if (c.interior) {                      // fast path: the clamps below are no-ops here
    c.base = mad24(iz, V.sz, mad24(iy, V.sy, ix));
    c.ix = ix; c.iy = iy; c.iz = iz;
    c.ox = 1; c.oy = V.sy; c.oz = V.sz;
    return c;
  }
  // clamp(i + 1, 0, res - 1) written so that a saturated index (huge or non-finite coordinate) cannot overflow
  int x0 = clampi(ix, 0, V.W - 1), x1 = clampi(ix, -1, V.W - 2) + 1;
  int y0 = clampi(iy, 0, V.H - 1), y1 = clampi(iy, -1, V.H - 2) + 1;
  int z0 = clampi(iz, 0, V.D - 1), z1 = clampi(iz, -1, V.D - 2) + 1;
  c.base = mad24(z0, V.sz, mad24(y0, V.sy, x0));
  c.ix = x0; c.iy = y0; c.iz = z0;
  c.ox = x1 - x0; c.oy = (y1 != y0) ? V.sy : 0; c.oz = (z1 != z0) ? V.sz : 0;
  return c;
}

// The 8 taps of a cell, held as the four (x0, x0+1) PAIRS they are fetched as -- each pair is one register pair
// that an 8-byte load fills directly, so a lane can keep its taps across steps (fetch_reuse) without copies:
//   a = (v000, v100)  at (y0, z0)      b = (v010, v110)  at (y1, z0)
//   e = (v001, v101)  at (y0, z1)      f = (v011, v111)  at (y1, z1)
typedef float f2 __attribute__((ext_vector_type(2)));
struct Taps { f2 a, b, e, f; };

DRRT_HD Taps taps_zero() { Taps t; t.a = t.b = t.e = t.f = f2{0.f, 0.f}; return t; }

// One (x0, x0+1) pair: ONE 8-byte load on the device (global_load_dwordx2 needs only 4-byte alignment).
DRRT_HD f2 ld_pair(const float* p) {
#if defined(__HIP_DEVICE_COMPILE__)
  typedef float __attribute__((ext_vector_type(2), aligned(4))) f2u;
  const f2u a = *reinterpret_cast<const f2u*>(p);
  return f2{a.x, a.y};
#else
  return f2{p[0], p[1]};
#endif
}

DRRT_HD Taps fetch(const float* __restrict__ d, const Cell& c) {
  Taps t;
#if defined(__HIP_DEVICE_COMPILE__)
  __builtin_assume(c.base >= 0 && c.base < (1 << 29));   // make_vol() rejects grids of 2^29 voxels or more
#endif
  const float* p = d + (unsigned)c.base;
  // The x-neighbour is the next float in memory: fetch each (x0, x0+1) pair with ONE 8-byte load.  The texture
  // addresser handles a wave's gather at a few lanes per clock, so 4 pair loads instead of 8 dword loads halve
  // the dominant cost of the march.  Cells clamped in x (ox == 0, only on the far x face) must not read p[1]:
  // that could run past the end of the grid allocation.
  if (c.ox == 1) {
    t.a = ld_pair(p); t.b = ld_pair(p + c.oy); t.e = ld_pair(p + c.oz); t.f = ld_pair(p + c.oz + c.oy);
    return t;
  }
  t.a = f2{p[0], p[c.ox]};                t.b = f2{p[c.oy], p[c.oy + c.ox]};
  t.e = f2{p[c.oz], p[c.oz + c.ox]};      t.f = f2{p[c.oz + c.oy], p[c.oz + c.oy + c.ox]};
  return t;
}

// The march's gather is bound by the texture addresser, and its cost is per gather INSTRUCTION: ~30-37 cycles of the
// CU's addresser for a divergent 64-lane load, the same with one active lane as with 64, and only ~15 % more for 16
// bytes per lane than for 8 (tools/chain_bench.hip, tools/gather_bench.hip).  With the pair copy of the grid --
// P[i] = {n[i], n[i+sy]}, the y-neighbour interleaved -- ONE 16-byte load at (x0, y0, z) returns the four taps of a
// z-face, {n(x0,y0), n(x0,y1), n(x0+1,y0), n(x0+1,y1)}, so a strictly interior cell is two loads instead of four
// (and the copy is 2x the grid, against 4x for a full (x,y) quad per voxel).  Same floats -> bit-identical results.
typedef float f4 __attribute__((ext_vector_type(4)));
DRRT_HD Taps taps_from_pair(f4 q0, f4 q1) {      // q0 = face z0, q1 = face z1 of the pair copy
  Taps t;
  t.a = f2{q0.x, q0.z}; t.b = f2{q0.y, q0.w};
  t.e = f2{q1.x, q1.z}; t.f = f2{q1.y, q1.w};
  return t;
}
#if defined(__HIPCC__)
__device__ __forceinline__ f4 ld_quad8(const float* p) {      // 16 bytes at 8-byte alignment: one global_load_dwordx4
  typedef float __attribute__((ext_vector_type(4), aligned(8))) f4u;
  const f4u a = *reinterpret_cast<const f4u*>(p);
  return f4{a.x, a.y, a.z, a.w};
}
#endif
DRRT_HD Taps fetch_vol(const Vol& V, const Cell& c) {
#if defined(__HIP_DEVICE_COMPILE__)
  if (V.pair != nullptr && c.interior) {
    __builtin_assume(c.base >= 0 && c.base < (1 << 29));
    const float* p = V.pair + 2u * (unsigned)c.base;
    return taps_from_pair(ld_quad8(p), ld_quad8(p + 2u * (unsigned)V.sz));
  }
#endif
  return fetch(V.data, c);
}

// ---- tap reuse ------------------------------------------------------------------------------------
// With ds = h/step_res a ray samples the same cell ~step_res times in a row, and the cell it moves on to
// shares a face -- 4 of the 8 taps -- with the one it leaves.  The march's limiter is the texture addresser,
// whose cost is per lane-address (above), so the taps a lane already holds are kept in registers:
//   REUSE 1  same cell as the previous step: no load at all;
//   REUSE 2  additionally, a move across ONE y- or z-face keeps the two (x0, x0+1) pairs of the shared face and
//            loads only the two pairs of the new far face (an x-move would still need four pair loads: the
//            pairs straddle it).
// Only strictly interior cells are cached (regular strides, 8 distinct taps).  The floats are the ones a full
// fetch would return, so results are bit-identical (tests: hostcheck on the CPU, GPU parity vs the oracle).
struct TapCache { Taps t; int base; };     // base < 0: nothing cached

template <int REUSE>
DRRT_HD void fetch_reuse(const Vol& V, const Cell& c, TapCache& tc) {
  if (REUSE == 0 || V.pair != nullptr) { tc.t = fetch_vol(V, c); return; }
  if (!c.interior) { tc.t = fetch(V.data, c); tc.base = -1; return; }
  if (c.base == tc.base) return;
  Taps& t = tc.t;
#if defined(__HIP_DEVICE_COMPILE__)
  __builtin_assume(c.base >= 0 && c.base < (1 << 29));
#endif
  const float* p = V.data + (unsigned)c.base;
  if (REUSE >= 2 && tc.base >= 0) {
    const int d = c.base - tc.base;
    if (d == V.sy)  { t.a = t.b; t.e = t.f; t.b = ld_pair(p + V.sy); t.f = ld_pair(p + V.sz + V.sy); tc.base = c.base; return; }   // +y
    if (d == -V.sy) { t.b = t.a; t.f = t.e; t.a = ld_pair(p);        t.e = ld_pair(p + V.sz);        tc.base = c.base; return; }   // -y
    if (d == V.sz)  { t.a = t.e; t.b = t.f; t.e = ld_pair(p + V.sz); t.f = ld_pair(p + V.sz + V.sy); tc.base = c.base; return; }   // +z
    if (d == -V.sz) { t.e = t.a; t.f = t.b; t.a = ld_pair(p);        t.b = ld_pair(p + V.sy);        tc.base = c.base; return; }   // -z
  }
  t.a = ld_pair(p); t.b = ld_pair(p + V.sy); t.e = ld_pair(p + V.sz); t.f = ld_pair(p + V.sz + V.sy);
  tc.base = c.base;
}

// n and RAW gradient / mixed partials (not yet multiplied by 1/h, 1/h^2).
struct Sample { float n, gx, gy, gz, hxy, hxz, hyz; };

template <bool WITH_HESS>
DRRT_HD Sample interp(const Taps& t, float wx, float wy, float wz) {
  Sample s;
  // x-differences at the four (y,z) edges
  float d00 = t.a.y - t.a.x, d10 = t.b.y - t.b.x, d01 = t.e.y - t.e.x, d11 = t.f.y - t.f.x;
  // x-lerped values
  float c00 = fmaf(wx, d00, t.a.x), c10 = fmaf(wx, d10, t.b.x);
  float c01 = fmaf(wx, d01, t.e.x), c11 = fmaf(wx, d11, t.f.x);
  float e0 = c10 - c00, e1 = c11 - c01;                  // d/dy at z0, z1
  float l0 = fmaf(wy, e0, c00), l1 = fmaf(wy, e1, c01);  // (x,y)-lerped at z0, z1
  float dz = l1 - l0;
  s.gz = dz;
  s.n  = fmaf(wz, dz, l0);
  float eyz = e1 - e0;
  s.gy = fmaf(wz, eyz, e0);
  float dxy0 = d10 - d00, dxy1 = d11 - d01;              // d2/dxdy at z0, z1
  float gx0 = fmaf(wy, dxy0, d00), gx1 = fmaf(wy, dxy1, d01);
  float gxz = gx1 - gx0;
  s.gx = fmaf(wz, gxz, gx0);
  if (WITH_HESS) {
    s.hxy = fmaf(wz, dxy1 - dxy0, dxy0);                 // src/volume.cpp:79-81
    s.hxz = gxz;                                         // src/volume.cpp:82-84
    s.hyz = eyz;                                         // src/volume.cpp:85-87
  } else {
    s.hxy = s.hxz = s.hyz = 0.f;
  }
  return s;
}

// src/volume.cpp:246-256
DRRT_HD bool inbounds(const Vol& V, float px, float py, float pz) {
  return (px >= 0.f) & (py >= 0.f) & (pz >= 0.f) & (px < V.bx) & (py < V.by) & (pz < V.bz);
}
// src/volume.cpp:258-271
DRRT_HD bool escaped(const Vol& V, float px, float py, float pz, float vx, float vy, float vz) {
  bool ex = ((px < 0.f) & (vx < 0.f)) | ((px >= V.bx) & (vx > 0.f));
  bool ey = ((py < 0.f) & (vy < 0.f)) | ((py >= V.by) & (vy > 0.f));
  bool ez = ((pz < 0.f) & (vz < 0.f)) | ((pz >= V.bz) & (vz > 0.f));
  return ex | ey | ez;
}

DRRT_HD float dot3(float ax, float ay, float az, float bx, float by, float bz) {
  return fmaf(az, bz, fmaf(ay, by, ax * bx));
}

// Fused volume::splat (src/volume.cpp:217-243): contribution of (val, grad) to the 8 corners.
//   corner(a,b,c) = val*X_a*Y_b*Z_c  +  gx*(+-)Y_b*Z_c + gy*(+-)X_a*Z_c + gz*(+-)X_a*Y_b
// with X_0 = 1-wx, X_1 = wx, sign = - for index 0, + for index 1.
struct Corners { float c000, c100, c010, c110, c001, c101, c011, c111; };

DRRT_HD Corners splat_weights(float wx, float wy, float wz, float val, float gx, float gy, float gz) {
  float x1 = wx, x0 = 1.f - wx, y1 = wy, y0 = 1.f - wy, z1 = wz, z0 = 1.f - wz;
  float a0 = fmaf(val, x0, -gx), a1 = fmaf(val, x1, gx);          // val*X_a -+ gx
  float yz00 = y0 * z0, yz10 = y1 * z0, yz01 = y0 * z1, yz11 = y1 * z1;
  float gyz0 = gy * z0, gyz1 = gy * z1, gzy0 = gz * y0, gzy1 = gz * y1;
  float b00 = -gyz0 - gzy0, b10 = gyz0 - gzy1, b01 = gzy0 - gyz1, b11 = gyz1 + gzy1;
  Corners c;
  c.c000 = fmaf(yz00, a0, x0 * b00);  c.c100 = fmaf(yz00, a1, x1 * b00);
  c.c010 = fmaf(yz10, a0, x0 * b10);  c.c110 = fmaf(yz10, a1, x1 * b10);
  c.c001 = fmaf(yz01, a0, x0 * b01);  c.c101 = fmaf(yz01, a1, x1 * b01);
  c.c011 = fmaf(yz11, a0, x0 * b11);  c.c111 = fmaf(yz11, a1, x1 * b11);
  return c;
}

// The same 8 corner contributions as x-PAIRS (c_0bc, c_1bc), computed with packed fp32 operations (v_pk_mul_f32 /
// v_pk_fma_f32: two IEEE operations per instruction, the SAME operations in the same order as splat_weights, so the
// values are bit-identical): 13 packed + 7 scalar instructions instead of 42 scalar ones.
struct CornerPairs { f2 c00, c10, c01, c11; };    // (y0,z0) (y1,z0) (y0,z1) (y1,z1), each (x0, x1)

DRRT_HD f2 fma2(f2 a, f2 b, f2 c) { return __builtin_elementwise_fma(a, b, c); }

DRRT_HD CornerPairs splat_weights_pk(float wx, float wy, float wz, float val, float gx, float gy, float gz) {
  const float y0 = 1.f - wy, z0 = 1.f - wz;
  const f2 X = f2{1.f - wx, wx}, Y = f2{y0, wy};
  const f2 A = fma2(f2{val, val}, X, f2{-gx, gx});                       // val*X_a -+ gx
  const f2 yzl = Y * z0, yzh = Y * wz;                                   // (yz00, yz10), (yz01, yz11)
  const f2 gyz = f2{z0, wz} * gy, gzy = Y * gz;                          // (gyz0, gyz1), (gzy0, gzy1)
  const float b00 = -gyz.x - gzy.x, b10 = gyz.x - gzy.y, b01 = gzy.x - gyz.y, b11 = gyz.y + gzy.y;
  CornerPairs c;
  c.c00 = fma2(f2{yzl.x, yzl.x}, A, X * b00);
  c.c10 = fma2(f2{yzl.y, yzl.y}, A, X * b10);
  c.c01 = fma2(f2{yzh.x, yzh.x}, A, X * b01);
  c.c11 = fma2(f2{yzh.y, yzh.y}, A, X * b11);
  return c;
}

// ---------------------------------------------------------------------------------------------
// one forward march iteration (src/tracer.cpp:68-86; plane :144-145; sdf :287-288)
// MODE 0 = trace, 1 = trace_plane, 2 = trace_sdf, 3 = trace_target (closest-approach tracking)
// ---------------------------------------------------------------------------------------------
struct FwdState {
  float x, y, z, vx, vy, vz;         // marching state
  float xtx, xty, xtz, vtx, vty, vtz;  // recorded exit / closest-approach state
  float aux0, aux1, aux2, aux3, aux4, aux5;  // MODE 1: plane origin+normal; MODE 3: target (aux0..2), best dist2 (aux3)
  bool inside, esc;
};

DRRT_HD void fwd_init(const Vol& V, FwdState& s) {
  s.xtx = s.x; s.xty = s.y; s.xtz = s.z; s.vtx = s.vx; s.vty = s.vy; s.vtz = s.vz;   // :56-57
  s.inside = inbounds(V, s.x, s.y, s.z);                                              // :61
  s.esc = false;                                                                      // :62
}

// The start of every forward march and of every replay of one: the ray (p, v), the mode's aux slots -- MODE 1: (a, b) = the
// plane's origin and direction; MODE 3: a = the target, and the record's dist2 starts at |p - a|^2 (src/tracer.cpp:200);
// otherwise zeros, a and b unused -- fwd_init, and the cell of p.
template <int MODE>
DRRT_HD void fwd_begin(const Vol& V, const float p[3], const float v[3], const float* a, const float* b, FwdState& s, Cell& c) {
  s.x = p[0]; s.y = p[1]; s.z = p[2]; s.vx = v[0]; s.vy = v[1]; s.vz = v[2];
  s.aux0 = s.aux1 = s.aux2 = s.aux3 = s.aux4 = s.aux5 = 0.f;
  if (MODE == 1) {
    s.aux0 = a[0]; s.aux1 = a[1]; s.aux2 = a[2];
    s.aux3 = b[0]; s.aux4 = b[1]; s.aux5 = b[2];
  }
  if (MODE == 3) {
    s.aux0 = a[0]; s.aux1 = a[1]; s.aux2 = a[2];
    const float ex = s.x - a[0], ey = s.y - a[1], ez = s.z - a[2];
    s.aux3 = dot3(ex, ey, ez, ex, ey, ez);
  }
  fwd_init(V, s);
  c = locate(V, s.x, s.y, s.z);
}

// One forward iteration.  In: `c` = cell of the current position (always located, used only when the
// ray is inside), `t` = the 8 taps there (valid when s.inside).  Out: `c` = cell of the NEW position,
// reused by the next iteration -- and when that cell is strictly interior the box tests are skipped
// (inbounds is true and escaped is false there by construction, see Cell::interior).
template <int MODE>
DRRT_HD void fwd_step_c(const Vol& V, const float* __restrict__ sdf, float ds, FwdState& s, Cell& c, const Taps& t) {
  float n = 0.f, gx = 0.f, gy = 0.f, gz = 0.f;
  if (s.inside) {                                                           // masked gather (Q4)
    Sample q = interp<false>(t, c.wx, c.wy, c.wz);
    n = q.n; gx = q.gx * V.inv_h; gy = q.gy * V.inv_h; gz = q.gz * V.inv_h;
  }
  const float dsn = ds * n;
  s.vx = fmaf(dsn, gx, s.vx); s.vy = fmaf(dsn, gy, s.vy); s.vz = fmaf(dsn, gz, s.vz);   // :70
  s.x = fmaf(ds, s.vx, s.x); s.y = fmaf(ds, s.vy, s.y); s.z = fmaf(ds, s.vz, s.z);      // :71
  c = locate(V, s.x, s.y, s.z);
  bool cur_inside, esc_now = false;
  if (MODE == 2) {                                                          // :287-288
    float d = 0.f;
    if (s.inside) d = interp<false>(fetch(sdf, c), c.wx, c.wy, c.wz).n;
    cur_inside = d < 0.f;
    if (!c.interior) esc_now = escaped(V, s.x, s.y, s.z, s.vx, s.vy, s.vz);
  } else {
    cur_inside = true;
    if (!c.interior) {
      cur_inside = inbounds(V, s.x, s.y, s.z);                              // :73
      esc_now = escaped(V, s.x, s.y, s.z, s.vx, s.vy, s.vz);                // :76
    }
    if (MODE == 1) {                                                        // :144-145
      float d = dot3(s.x - s.aux0, s.y - s.aux1, s.z - s.aux2, s.aux3, s.aux4, s.aux5);
      cur_inside = cur_inside & !(d > 0.f);
    }
  }
  const bool cross = s.inside & !cur_inside;                                // :74
  s.esc = s.esc | cross | esc_now;                                          // :75-76
  if (MODE == 3) {                                                          // :216-227
    float ex = s.x - s.aux0, ey = s.y - s.aux1, ez = s.z - s.aux2;
    float cur = dot3(ex, ey, ez, ex, ey, ez);
    if (cur < s.aux3) { s.xtx = s.x; s.xty = s.y; s.xtz = s.z; s.vtx = s.vx; s.vty = s.vy; s.vtz = s.vz; s.aux3 = cur; }
  } else if (cross) {                                                       // :79-80
    s.xtx = s.x; s.xty = s.y; s.xtz = s.z; s.vtx = s.vx; s.vty = s.vy; s.vtz = s.vz;
  }
  s.inside = cur_inside;                                                    // :86
}

// trace_plane, for a ray that has just been flagged escaped: can it produce ANOTHER exit record later?
// The reference keeps marching escaped rays while its global loop runs (src/tracer.cpp:130-160) and records
// EVERY inside -> outside transition, so a ray that can come back into {in bounds, not past the plane} may
// overwrite its exit record later.  An escaped ray flies straight (its gathers are masked), hence it can
// NOT come back when it is outside the box moving away (volume::escaped), or past the plane and not
// approaching it.  Anything else -- in practice only a ray that STARTS past the plane and heads back
// through it -- is flagged and re-marched over the global loop count by ray_full<1>.
DRRT_HD bool plane_again(const Vol& V, const FwdState& s) {
  const float d = dot3(s.x - s.aux0, s.y - s.aux1, s.z - s.aux2, s.aux3, s.aux4, s.aux5);
  const float dv = dot3(s.vx, s.vy, s.vz, s.aux3, s.aux4, s.aux5);
  const bool gone = escaped(V, s.x, s.y, s.z, s.vx, s.vy, s.vz) | ((d > 0.f) & (dv >= 0.f));
  return !gone;
}

template <int MODE>
DRRT_HD void fwd_step(const Vol& V, const float* __restrict__ sdf, float ds, FwdState& s, Cell& c) {
  Taps t = taps_zero();
  if (s.inside) t = fetch_vol(V, c);
  fwd_step_c<MODE>(V, sdf, ds, s, c, t);
}

// The same with the taps the lane already holds kept across steps (fetch_reuse).  A ray that is not inside does
// not sample (Q4) and fwd_step_c ignores the taps then, so the cache is simply left alone.
template <int MODE, int REUSE>
DRRT_HD void fwd_step_r(const Vol& V, const float* __restrict__ sdf, float ds, FwdState& s, Cell& c, TapCache& tc) {
  if (s.inside) fetch_reuse<REUSE>(V, c, tc);
  fwd_step_c<MODE>(V, sdf, ds, s, c, tc.t);
}

// ---------------------------------------------------------------------------------------------
// one adjoint march iteration (src/tracer.cpp:420-435; sdf :488-497).  Returns true when the ray
// is still active after the step, in which case (c, w) is its contribution to dL/dn: add the
// 8 corner values `w` at the 8 taps of cell `c`.
// ---------------------------------------------------------------------------------------------
struct AdjState {
  float x, y, z, vx, vy, vz;
  float lx, ly, lz, mx, my, mz;      // lambda (dL/dx), mu (dL/dv)
  bool active, outside;
};

DRRT_HD void adj_init(const Vol& V, float ds, float dxx, float dxy, float dxz,
                      float dvx, float dvy, float dvz, AdjState& s) {
  s.lx = dxx; s.ly = dxy; s.lz = dxz;                                                   // :409
  s.mx = fmaf(ds, dxx, dvx); s.my = fmaf(ds, dxy, dvy); s.mz = fmaf(ds, dxz, dvz);      // :410
  s.active = !escaped(V, s.x, s.y, s.z, -s.vx, -s.vy, -s.vz);                           // :413-414
  s.outside = false;
}

// One adjoint iteration is split in two halves so that the windowed kernel can issue the NEXT sample's gather
// between them (software pipelining, k_backtrace_flat / k_backtrace_ring); adj_step below is the plain sequence.
struct AdjSample { float n, gx, gy, gz, hxy, hxz, hyz; };   // n, grad n (scaled by 1/h), mixed partials (raw)

// First half (src/tracer.cpp:421-425; sdf :488-497): sample the cell `c` the ray has just stepped into (taps `t`),
// update v, decide whether the ray is still active.  Everything on the march's critical path is here.
// MODE 1: `st` are the 8 sdf taps of the cell when the caller has gathered them ahead (`have_st`), else they are fetched here.
template <int MODE>   // 0 = backtrace, 1 = backtrace_sdf
DRRT_HD bool adj_sample_st(const Vol& V, const float* __restrict__ sdf, float ds, AdjState& s, const Cell& c, const Taps& t,
                           AdjSample& m, const Taps& st, bool have_st) {
  const Sample q = interp<true>(t, c.wx, c.wy, c.wz);                                  // :421-422
  m.n = q.n; m.gx = q.gx * V.inv_h; m.gy = q.gy * V.inv_h; m.gz = q.gz * V.inv_h;
  m.hxy = q.hxy; m.hxz = q.hxz; m.hyz = q.hyz;
  const float mdsn = -ds * m.n;
  s.vx = fmaf(mdsn, m.gx, s.vx); s.vy = fmaf(mdsn, m.gy, s.vy); s.vz = fmaf(mdsn, m.gz, s.vz); // :423
  bool active = true;
  if (!c.interior) active = !escaped(V, s.x, s.y, s.z, -s.vx, -s.vy, -s.vz);            // :425
  if (MODE == 1) {                                                                      // :488-497
    bool now_out = interp<false>(have_st ? st : fetch(sdf, c), c.wx, c.wy, c.wz).n >= 0.f;
    active = active & !((!s.outside) & now_out);
    s.outside = now_out;
  }
  s.active = active;
  return active;
}
template <int MODE>
DRRT_HD bool adj_sample(const Vol& V, const float* __restrict__ sdf, float ds, AdjState& s, const Cell& c, const Taps& t,
                        AdjSample& m) {
  return adj_sample_st<MODE>(V, sdf, ds, s, c, t, m, t, false);
}

// The lambda / mu recurrences of one adjoint iteration (:434-435), dn = mu . grad n: the exact transpose of the forward
// step's Jacobian (d(n grad n)/dx = grad n grad n^T + n H, H the mixed partials, Q10).
DRRT_HD void adj_recur(const Vol& V, float ds, AdjState& s, const AdjSample& m, float dn) {
  const float n = m.n, gx = m.gx, gy = m.gy, gz = m.gz;
  // la += ds*(dn*grad n + n*H*mu), H = mixed partials / h^2, zero diagonal (:434, Q10)
  const float hxy = m.hxy * V.inv_h2, hxz = m.hxz * V.inv_h2, hyz = m.hyz * V.inv_h2;
  const float hmx = fmaf(hxz, s.mz, hxy * s.my);
  const float hmy = fmaf(hyz, s.mz, hxy * s.mx);
  const float hmz = fmaf(hyz, s.my, hxz * s.mx);
  s.lx = fmaf(ds, fmaf(dn, gx, n * hmx), s.lx);
  s.ly = fmaf(ds, fmaf(dn, gy, n * hmy), s.ly);
  s.lz = fmaf(ds, fmaf(dn, gz, n * hmz), s.lz);
  s.mx = fmaf(ds, s.lx, s.mx); s.my = fmaf(ds, s.ly, s.my); s.mz = fmaf(ds, s.lz, s.mz);   // :435
}

// Second half (:430-435), for a ray that is still active: its contribution `w` to dL/dn at the 8 taps of `c`, then
// the lambda / mu recurrences.  Nothing here feeds the next sample's position.
DRRT_HD void adj_contrib(const Vol& V, float ds, float grad_scale, AdjState& s, const Cell& c, const AdjSample& m,
                         Corners& w) {
  const float n = m.n, gx = m.gx, gy = m.gy, gz = m.gz;
  const float dn = dot3(s.mx, s.my, s.mz, gx, gy, gz);                                  // :430
  const float nds = (n * ds) * grad_scale;
  w = splat_weights(c.wx, c.wy, c.wz, dn * ds, nds * s.mx, nds * s.my, nds * s.mz);     // :431-432
  adj_recur(V, ds, s, m, dn);
}

template <int MODE>   // 0 = backtrace, 1 = backtrace_sdf
DRRT_HD bool adj_step(const Vol& V, const float* __restrict__ sdf, float ds, float grad_scale,
                      AdjState& s, Cell& c, Corners& w) {
  s.x = fmaf(-ds, s.vx, s.x); s.y = fmaf(-ds, s.vy, s.y); s.z = fmaf(-ds, s.vz, s.z);   // :420
  c = locate(V, s.x, s.y, s.z);
  AdjSample m;
  if (!adj_sample<MODE>(V, sdf, ds, s, c, fetch_vol(V, c), m)) return false;            // :426-428
  adj_contrib(V, ds, grad_scale, s, c, m, w);
  return true;
}

// ---- cylinder (radial profile) volume, src/cylinder_volume.cpp ---------------------------------
struct Cyl {
  const float* data;    // may point to LDS
  int rres;
  float radius, length;
  float h, inv_h;       // h = radius/(rres-1) (:42), inv_h = 1/h
  float r2;             // radius*radius
};

DRRT_HD Cyl make_cyl(const float* data, int rres, float radius, float length) {
  Cyl C; C.data = data; C.rres = rres; C.radius = radius; C.length = length;
  C.h = radius / (float)(rres - 1); C.inv_h = 1.f / C.h; C.r2 = radius * radius;
  return C;
}

struct CylCell { int i0, i1; float w0, r, rhx, rhz; bool tiny; };

DRRT_HD CylCell cyl_locate(const Cyl& C, float px, float pz) {
  CylCell c;
  float xs = px - C.radius, zs = pz - C.radius;                 // :37-38 (y component zeroed)
  c.r = sqrtf(fmaf(xs, xs, zs * zs));                           // :41
  float rm = c.r * C.inv_h;                                     // :44 (r / h)
  int ir = f2i_sat(floorf(rm));
  c.i0 = clampi(ir, 0, C.rres - 1);                             // :45
  c.i1 = clampi(c.i0 + 1, 0, C.rres - 1);                       // :46
  c.w0 = rm - (float)c.i0;                                      // :48 (uses the CLAMPED idx0)
  c.tiny = c.r < 1e-6f;                                         // :15, :56
  float inv_r = c.tiny ? 0.f : 1.f / c.r;
  c.rhx = xs * inv_r; c.rhz = zs * inv_r;                       // normalize(xs), zeroed when tiny
  return c;
}

// src/cylinder_volume.cpp:150-156
DRRT_HD bool cyl_inbounds(const Cyl& C, float px, float py, float pz) {
  float xs = px - C.radius, zs = pz - C.radius;
  return (fmaf(xs, xs, zs * zs) < C.r2) & (py < C.length) & (py >= 0.f);
}
// src/cylinder_volume.cpp:158-170
DRRT_HD bool cyl_escaped(const Cyl& C, float px, float py, float pz, float vx, float vy, float vz) {
  float xs = px - C.radius, zs = pz - C.radius;
  bool esc_len = ((py < 0.f) & (vy < 0.f)) | ((py > C.length) & (vy > 0.f));
  bool out_r = fmaf(xs, xs, zs * zs) >= C.r2;
  bool esc_r = fmaf(xs, vx, zs * vz) > 0.f;
  return (out_r & esc_r) | esc_len;
}

// one forward cable iteration (src/tracer.cpp:351-373); target/best in aux0..3 like MODE 3
DRRT_HD void cable_fwd_step(const Cyl& C, float ds, FwdState& s) {
  CylCell c = cyl_locate(C, s.x, s.z);                                  // :351 (unmasked gather)
  float v0 = C.data[c.i0], v1 = C.data[c.i1];
  float f = fmaf(v1, c.w0, v0 * (1.f - c.w0));                          // :53
  float rx = (v1 - v0) * C.inv_h;                                       // :54
  float dsn = ds * f;
  s.vx = fmaf(dsn, rx * c.rhx, s.vx); s.vz = fmaf(dsn, rx * c.rhz, s.vz);   // :353 (grad_y = 0)
  s.x = fmaf(ds, s.vx, s.x); s.y = fmaf(ds, s.vy, s.y); s.z = fmaf(ds, s.vz, s.z);   // :354
  float ex = s.x - s.aux0, ey = s.y - s.aux1, ez = s.z - s.aux2;
  float cur = dot3(ex, ey, ez, ex, ey, ez);                             // :356
  bool cur_inside = cyl_inbounds(C, s.x, s.y, s.z);
  bool cross = s.inside & !cur_inside;
  s.esc = s.esc | cross | cyl_escaped(C, s.x, s.y, s.z, s.vx, s.vy, s.vz);   // :361-362
  if (cur < s.aux3) { s.xtx = s.x; s.xty = s.y; s.xtz = s.z; s.vtx = s.vx; s.vty = s.vy; s.vtz = s.vz; s.aux3 = cur; } // :365-367
  s.inside = cur_inside;
}

// What one reverse cable iteration samples at (s.x, s.z): n, n' and grad n = n' rhat (y component 0).  Steps v back
// (:550) and leaves x alone.  Shared by the dL/dn adjoint and the ray-state adjoint.
struct CylAdjSample { CylCell c; float n, rx, gx, gz; };

DRRT_HD CylAdjSample cable_adj_sample(const Cyl& C, float ds, AdjState& s) {
  CylAdjSample m;
  m.c = cyl_locate(C, s.x, s.z);
  float v0 = C.data[m.c.i0], v1 = C.data[m.c.i1];
  m.n = fmaf(v1, m.c.w0, v0 * (1.f - m.c.w0));                          // :53
  m.rx = (v1 - v0) * C.inv_h;                                           // :54 / :88
  m.gx = m.rx * m.c.rhx; m.gz = m.rx * m.c.rhz;                         // grad n (y comp 0)
  float mdsn = -ds * m.n;
  s.vx = fmaf(mdsn, m.gx, s.vx); s.vz = fmaf(mdsn, m.gz, s.vz);         // :550
  return m;
}

// The lambda / mu recurrences of one reverse cable iteration (:561-562), dn = mu . grad n taken before them.  The sample
// is passed by value: by reference the compiler orders two multiplies of k_backtrace_cable the other way round.
DRRT_HD void cable_adj_recur(float ds, AdjState& s, CylAdjSample m, float dn) {
  const CylCell& c = m.c;
  // Hessian (:88-108): (I - rhat rhat^T)_{xz} * (n'/r), zero when r < eps
  float sH = c.tiny ? 0.f : m.rx / c.r;
  float h00 = (1.f - c.rhx * c.rhx) * sH, h02 = -(c.rhx * c.rhz) * sH, h22 = (1.f - c.rhz * c.rhz) * sH;
  float hmx = fmaf(h02, s.mz, h00 * s.mx), hmz = fmaf(h22, s.mz, h02 * s.mx);
  s.lx = fmaf(ds, fmaf(dn, m.gx, m.n * hmx), s.lx);                     // :561 (y row of H is 0)
  s.lz = fmaf(ds, fmaf(dn, m.gz, m.n * hmz), s.lz);
  s.mx = fmaf(ds, s.lx, s.mx); s.my = fmaf(ds, s.ly, s.my); s.mz = fmaf(ds, s.lz, s.mz);   // :562
}

// one adjoint cable iteration (src/tracer.cpp:547-562); contribution: a0 at i0, a1 at i1
DRRT_HD bool cable_adj_step(const Cyl& C, float ds, AdjState& s, int& i0, int& i1, float& a0, float& a1) {
  s.x = fmaf(-ds, s.vx, s.x); s.y = fmaf(-ds, s.vy, s.y); s.z = fmaf(-ds, s.vz, s.z);     // :547
  const CylAdjSample m = cable_adj_sample(C, ds, s);
  const CylCell& c = m.c;
  float w0 = c.w0, w1 = 1.f - c.w0;
  s.active = !cyl_escaped(C, s.x, s.y, s.z, -s.vx, -s.vy, -s.vz);       // :552
  if (!s.active) return false;
  float dn = fmaf(s.mz, m.gz, s.mx * m.gx);                             // :557
  // cylinder_volume::splat (:113-148): value taps val*w, gradient taps -+(grad.rhat)/h
  float val = dn * ds;
  float gv = (m.n * ds) * fmaf(s.mz, c.rhz, s.mx * c.rhx);              // dot(dnx*ds, rhat); 0 if tiny
  float gvh = gv * C.inv_h;
  i0 = c.i0; i1 = c.i1;
  a0 = fmaf(val, w1, -gvh); a1 = fmaf(val, w0, gvh);
  cable_adj_recur(ds, s, m, dn);
  return true;
}

// ---------------------------------------------------------------------------------------------
// whole-ray drivers shared by the kernels (one ray per lane) and by tests/hostcheck
// ---------------------------------------------------------------------------------------------
struct RayOut { float xt[3], vt[3]; float dist2; bool esc, act, again; unsigned steps; };

// trace / trace_plane / trace_sdf for ONE ray, per-ray termination (see drrt_march.h header)
constexpr int kTapReuse = 1;      // product default of the forward marches (see fetch_reuse): measured on MI355X, 256^3 /
                                  // 1M rays: no reuse 1.47 ms, same-cell 1.31 ms, + shared-face 1.68 ms (its branches cost
                                  // more issue slots than the two pair loads they save)

template <int MODE, int REUSE = kTapReuse>
DRRT_HD RayOut trace_ray(const Vol& V, const float* __restrict__ sdf, float ds, int max_steps,
                         const float p[3], const float v[3], const float* pln_o, const float* pln_d) {
  FwdState s;
  Cell c;
  fwd_begin<MODE>(V, p, v, pln_o, pln_d, s, c);
  bool act = true;
  if (MODE == 2) act = interp<false>(fetch(sdf, c), c.wx, c.wy, c.wz).n < 0.f;   // src/tracer.cpp:276-277
  unsigned steps = 0;
  TapCache tc;
  tc.base = -1;
  tc.t = taps_zero();
  for (int it = 0; it < max_steps; ++it) {
    fwd_step_r<MODE, REUSE>(V, sdf, ds, s, c, tc);
    ++steps;
    if (s.esc) break;                                                     // per-ray form of :82
  }
  act = act & !s.esc;                                                     // :77
  if (MODE != 2 && !s.esc) { s.xtx = s.x; s.xty = s.y; s.xtz = s.z; }     // :95 (vt stays, Q6)
  RayOut o;
  o.xt[0] = s.xtx; o.xt[1] = s.xty; o.xt[2] = s.xtz; o.vt[0] = s.vtx; o.vt[1] = s.vty; o.vt[2] = s.vtz;
  o.dist2 = 0.f; o.esc = s.esc; o.act = act; o.steps = steps; o.again = false;
  if (MODE == 1 && s.esc) o.again = plane_again(V, s);
  if (MODE == 2 && s.esc && s.inside) {
    // trace_sdf: the ray left the BOX (volume::escaped) while the clamped sdf sample still reads negative.  The
    // reference keeps marching it -- still "inside", still refracted by clamped samples -- and records the
    // moment the sdf turns non-negative, if its global loop lasts that long (:283-304).  Flag for ray_full<2>.
    // (Once the sdf sample is non-negative the later ones are masked to 0, so a ray can cross only once.)
    o.again = true;
  }
  return o;
}

// trace_plane / trace_sdf for ONE ray over exactly `total` iterations of the reference's global loop, no
// early termination (src/tracer.cpp:130-160, :283-304 as written): for the rays trace_ray flags with `again`.
template <int MODE>
DRRT_HD RayOut ray_full(const Vol& V, const float* __restrict__ sdf, float ds, unsigned total, const float p[3],
                        const float v[3], const float* pln_o, const float* pln_d) {
  FwdState s;
  Cell c;
  fwd_begin<MODE>(V, p, v, pln_o, pln_d, s, c);
  for (unsigned it = 0; it < total; ++it) fwd_step<MODE>(V, sdf, ds, s, c);
  if (MODE != 2 && !s.esc) { s.xtx = s.x; s.xty = s.y; s.xtz = s.z; }
  RayOut o;
  o.xt[0] = s.xtx; o.xt[1] = s.xty; o.xt[2] = s.xtz; o.vt[0] = s.vtx; o.vt[1] = s.vty; o.vt[2] = s.vtz;
  o.dist2 = 0.f; o.esc = s.esc; o.act = !s.esc; o.steps = total; o.again = false;
  return o;
}

// trace_target phase A for ONE ray: march until escaped, track the closest approach;
// `cont` receives the marching state (x, v) for phase B.
template <int REUSE = kTapReuse>
DRRT_HD RayOut target_ray_a(const Vol& V, float ds, int max_steps, const float p[3], const float v[3],
                            const float tg[3], float cont[6]) {
  FwdState s;
  Cell c;
  fwd_begin<3>(V, p, v, tg, nullptr, s, c);
  unsigned steps = 0;
  TapCache tc;
  tc.base = -1;
  tc.t = taps_zero();
  for (int it = 0; it < max_steps; ++it) {
    fwd_step_r<3, REUSE>(V, nullptr, ds, s, c, tc);
    ++steps;
    if (s.esc) break;
  }
  RayOut o;
  o.xt[0] = s.xtx; o.xt[1] = s.xty; o.xt[2] = s.xtz; o.vt[0] = s.vtx; o.vt[1] = s.vty; o.vt[2] = s.vtz;
  o.dist2 = s.aux3; o.esc = s.esc; o.act = !s.esc; o.steps = steps;
  cont[0] = s.x; cont[1] = s.y; cont[2] = s.z; cont[3] = s.vx; cont[4] = s.vy; cont[5] = s.vz;
  return o;
}

// trace_target phase B for ONE ray: an escaped ray flies straight (its gathers are masked) for
// the remaining `total - done` iterations of the reference's global loop (:225-227 is not gated
// by `escaped`).  Returns true when the closest-approach record was improved.
DRRT_HD bool target_ray_b(float ds, unsigned done, unsigned total, const float cont[6], const float tg[3],
                          float& best, float xt[3], float vt[3]) {
  float x = cont[0], y = cont[1], z = cont[2];
  const float vx = cont[3], vy = cont[4], vz = cont[5];
  bool upd = false;
  for (unsigned k = done; k < total; ++k) {
    x = fmaf(ds, vx, x); y = fmaf(ds, vy, y); z = fmaf(ds, vz, z);
    float ex = x - tg[0], ey = y - tg[1], ez = z - tg[2];
    float cur = dot3(ex, ey, ez, ex, ey, ez);
    if (cur < best) { best = cur; xt[0] = x; xt[1] = y; xt[2] = z; upd = true; }
  }
  if (upd) { vt[0] = vx; vt[1] = vy; vt[2] = vz; }
  return upd;
}

// backtrace / backtrace_sdf for ONE ray; `sink(cell, corners)` receives every contribution.
template <int MODE, typename Sink>
DRRT_HD unsigned backtrace_ray(const Vol& V, const float* __restrict__ sdf, float ds, float grad_scale,
                               int max_steps, const float xt[3], const float vt[3], const float dx[3],
                               const float dv[3], Sink&& sink) {
  AdjState s;
  s.x = xt[0]; s.y = xt[1]; s.z = xt[2]; s.vx = vt[0]; s.vy = vt[1]; s.vz = vt[2];
  adj_init(V, ds, dx[0], dx[1], dx[2], dv[0], dv[1], dv[2], s);
  if (MODE == 1 && s.active) {                                            // src/tracer.cpp:476-477
    Cell c = locate(V, s.x, s.y, s.z);
    s.outside = interp<false>(fetch(sdf, c), c.wx, c.wy, c.wz).n >= 0.f;
  }
  unsigned steps = 0;
  for (int it = 0; it < max_steps && s.active; ++it) {
    Cell c; Corners w;
    if (!adj_step<MODE>(V, sdf, ds, grad_scale, s, c, w)) break;
    ++steps;
    sink(c, w);
  }
  return steps;
}

// ---- the integral operators: one forward loop, one reverse march -----------------------------------------------------
// trace_opl, trace_field, trace_emission and trace_vector are trace with a line integral over the samples the march takes anyway; their
// adjoints, and the ray-state adjoint of trace, are one reverse march.  Both skeletons are written once here; an operator
// supplies an integrand (forward) and a term (reverse), defined with its mathematics further down.
struct RayGrad { float dp[3], dv[3]; unsigned steps; bool failed; };

// The forward loop for ONE ray.  The state update is fwd_step_c<0> itself on the taps `taps(c)` returns, looped as
// trace_ray<0> loops it, so (xt, vt, steps) are trace_ray<0>'s bit for bit; the sample is evaluated once more for n_k (the
// compiler merges the two).  `q(c, inside, n)` is called once per iteration, before the step, with the mask of
// fwd_step_c's sample (Q4) and n = n_k under it, 0.f while the ray is not inside (free flight outside the box adds
// nothing).  The integrand samples its own fields at the cell and weights of c, under the same mask, and owns its
// accumulators, which start at 0.f and are updated in iteration order.  A failed ray leaves in them what it accumulated.
// `q.step(s)` is called once per iteration behind the step, with the state it left: s.v is v_{k+1}, the velocity that
// carried the ray from x_k to x_{k+1} (an integrand whose summand needs the ray's direction closes its iteration there).
template <typename TapFn, typename Integrand>
DRRT_HD RayOut trace_integral_ray(const Vol& V, float ds, int max_steps, const float p[3], const float v[3], TapFn&& taps,
                                  Integrand&& q) {
  FwdState s;
  Cell c;
  fwd_begin<0>(V, p, v, nullptr, nullptr, s, c);
  unsigned steps = 0;
  for (int it = 0; it < max_steps; ++it) {
    Taps t = taps_zero();
    float n = 0.f;
    if (s.inside) {                                                       // the masked sample of fwd_step_c (Q4)
      t = taps(c);
      n = interp<false>(t, c.wx, c.wy, c.wz).n;
    }
    q(c, s.inside, n);
    fwd_step_c<0>(V, nullptr, ds, s, c, t);
    q.step(s);
    ++steps;
    if (s.esc) break;                                                     // per-ray form of :82
  }
  if (!s.esc) { s.xtx = s.x; s.xty = s.y; s.xtz = s.z; }                  // :95 (vt stays, Q6)
  RayOut o;
  o.xt[0] = s.xtx; o.xt[1] = s.xty; o.xt[2] = s.xtz; o.vt[0] = s.vtx; o.vt[1] = s.vty; o.vt[2] = s.vtz;
  o.dist2 = 0.f; o.esc = s.esc; o.act = !s.esc; o.steps = steps; o.again = false;
  return o;
}

// ---- the seeded reverse run: what every reverse march of the grid shares ------------------------------------------------
// A reverse march undoes the forward iterations hi-1 .. lo of a ray from the state (x_hi, v_hi) and the seeds (gx, gv) on
// it.  rev_seed seeds it like adj_init: lambda = gx (dL/dx), mu = gv + ds gx, and q = gv.  q is dL/dv_k; mu runs one
// iteration ahead of it, as adj_recur leaves it (q is mu before its last update), so after the iteration that arrives at
// x_k lambda = dL/dx_k and q = dL/dv_k: rev_store's (dpos, dvel).  The iterations come in runs of equal `inside` mask of
// the forward (Q4: it samples n only while the ray is inside):
//   sampled run   rev_sampled: hi - lo reverse iterations of adj_sample<0> / adj_recur with neither the backward-escape
//                 test nor the adjoint's own step bound.  The last of them (`entry`) samples at (ex, ey, ez), the run's
//                 first position as the forward's replay took it, instead of its reconstruction x_{lo+1} - ds v_{lo+1}: a
//                 ray that starts on a face (where grad n jumps) would otherwise be sampled a rounding error outside it.
//   free flight   rev_flight: m iterations outside leave lambda unchanged and add m ds lambda to mu and q.  The caller
//                 sets the position the next sampled run starts from.
// `taps(c)` returns the 8 taps of cell c (the caller chooses how they are fetched; the floats are the grid's).
// What an operator adds to a sampled run is its `term`, called in this order in every reverse iteration, m the sample
// (n_k, grad n_k):
//   term.enter(V, c, s)                    behind locate and before the sample: c is the cell of x_k and s.v still holds
//                                          v_{k+1}, the velocity that carried the ray out of x_k; a term whose summand has
//                                          the ray's direction in it seeds mu (dL/dv_{k+1}) here, so that dn and the
//                                          contribution to dL/dn below see the seed
//   dn = term.dn(V, c, m, mu . grad n_k)   the factor of ds grad n_k that adj_recur adds to lambda: d L / d n_k over ds
//   sink(c, val, gx, gy, gz)               the contribution to dL/dn, formed like adj_contrib's with mu BEFORE adj_recur
//                                          updates it: val = dn ds, g = (n_k ds grad_scale) mu; the caller adds
//                                          splat_weights(c.wx, c.wy, c.wz, val, gx, gy, gz) at the 8 taps of c
//   term.pull(V, c, m, s, entry)           the term's own pulls on lambda (the gradients of its fields at the sample
//                                          position, a direct seed on x_k) and its contributions to its own grids, BEFORE
//                                          adj_recur, whose closing mu += ds lambda must see the pulls
//   adj_recur(V, ds, s, m, dn)
//   term.after()                           the term's running scalars
// With grad_scale = 1 / h (DRRT_FLAG_CORRECTED_H) the sum of the contributions is the exact discrete derivative; the 1/h
// scales only the splat into the grid (Q3) and does not enter the ray gradients.
struct NoTerm {                              // trace itself: nothing is integrated
  DRRT_HD void enter(const Vol&, const Cell&, AdjState&) {}
  DRRT_HD float dn(const Vol&, const Cell&, const AdjSample&, float mg) { return mg; }
  DRRT_HD void pull(const Vol&, const Cell&, const AdjSample&, AdjState&, bool) {}
  DRRT_HD void after() {}
};
struct NoSink {                              // a ray-state adjoint: no contribution to dL/dn is formed
  DRRT_HD void operator()(const Cell&, float, float, float, float) {}
};
struct NoVSeed {                             // a ray path without the velocity series: statically no seed on vpath
  DRRT_HD bool operator()(unsigned, float*) const { return false; }
};

struct RevMarch { AdjState s; float qx, qy, qz; };

DRRT_HD void rev_seed(RevMarch& r, float ds, const float x[3], const float v[3], const float gx[3], const float gv[3]) {
  AdjState& s = r.s;
  s.x = x[0]; s.y = x[1]; s.z = x[2]; s.vx = v[0]; s.vy = v[1]; s.vz = v[2];
  s.lx = gx[0]; s.ly = gx[1]; s.lz = gx[2];                                               // adj_init, :409
  s.mx = fmaf(ds, gx[0], gv[0]); s.my = fmaf(ds, gx[1], gv[1]); s.mz = fmaf(ds, gx[2], gv[2]);   // :410
  s.active = true; s.outside = false;
  r.qx = gv[0]; r.qy = gv[1]; r.qz = gv[2];
}

template <typename TapFn, typename Sink, typename Term>
DRRT_HD void rev_sampled(const Vol& V, float ds, float grad_scale, RevMarch& r, unsigned hi, unsigned lo, float ex, float ey,
                         float ez, TapFn&& taps, Sink&& sink, Term&& term) {
  AdjState& s = r.s;
  for (unsigned k = hi; k > lo; --k) {
    s.x = fmaf(-ds, s.vx, s.x); s.y = fmaf(-ds, s.vy, s.y); s.z = fmaf(-ds, s.vz, s.z);   // :420
    if (k == lo + 1u) { s.x = ex; s.y = ey; s.z = ez; }                  // the run's first sample, as the forward took it
    const Cell c = locate(V, s.x, s.y, s.z);
    term.enter(V, c, s);
    AdjSample m;
    (void)adj_sample<0>(V, nullptr, ds, s, c, taps(c), m);                // v_{k-1}; the escape test is not used
    const float dn = term.dn(V, c, m, dot3(s.mx, s.my, s.mz, m.gx, m.gy, m.gz));         // :430
    const float nds = (m.n * ds) * grad_scale;
    sink(c, dn * ds, nds * s.mx, nds * s.my, nds * s.mz);
    r.qx = s.mx; r.qy = s.my; r.qz = s.mz;
    term.pull(V, c, m, s, k == lo + 1u);
    adj_recur(V, ds, s, m, dn);
    term.after();
  }
}

DRRT_HD void rev_flight(RevMarch& r, unsigned m, float ds) {
  AdjState& s = r.s;
  const float ads = (float)m * ds;
  r.qx = fmaf(ads, s.lx, r.qx); r.qy = fmaf(ads, s.ly, r.qy); r.qz = fmaf(ads, s.lz, r.qz);
  s.mx = fmaf(ads, s.lx, s.mx); s.my = fmaf(ads, s.ly, s.my); s.mz = fmaf(ads, s.lz, s.mz);
}

DRRT_HD void rev_store(const RevMarch& r, float dp[3], float dv[3]) {
  dp[0] = r.s.lx; dp[1] = r.s.ly; dp[2] = r.s.lz;
  dv[0] = r.qx; dv[1] = r.qy; dv[2] = r.qz;
}

// The reverse march for ONE ray: dL/dpos, dL/dvel from the seeds (dx, dv) on the exit ray (xt, vt), given the forward's
// inputs (p0, v0) and its iteration count K, and the contributions to dL/dn.  A ray that starts outside flies straight for
// e iterations first (x_e = x0 + e ds v0) and is refracted by the samples at x_e .. x_{K-1}: the masks are F^e T^(K-e).
//   * K >= max_steps (the forward's Q5 bound): the ray failed (vt is the stale v0, Q6) -> zero gradient, failed = true,
//     no contribution.  A ray that exits on exactly the last allowed iteration looks the same and is treated the same.
//   * the prefix is replayed from (p0, v0) with the forward's own operations; no in-box sample among x_0 .. x_{K-1}:
//     the ray never entered, (xt, vt) = (p0, v0), every integral is 0, the gradient is the identity (dx, dv) and there is
//     no contribution.
//   * otherwise the sampled run K-1 .. e from (xt, vt), then the free flight of the prefix -- for e = 0 too: 0 ds lambda is
//     NaN for an infinite lambda.
template <typename TapFn, typename Sink, typename Term>
DRRT_HD RayGrad integral_backtrace_ray(const Vol& V, float ds, float grad_scale, int max_steps, unsigned K,
                                       const float p0[3], const float v0[3], const float xt[3], const float vt[3],
                                       const float dx[3], const float dv[3], TapFn&& taps, Sink&& sink, Term&& term) {
  RayGrad g;
  g.steps = 0; g.failed = false;
  if (max_steps <= 0 || K >= (unsigned)max_steps) {
    g.dp[0] = g.dp[1] = g.dp[2] = g.dv[0] = g.dv[1] = g.dv[2] = 0.f;
    g.failed = true;
    return g;
  }
  // free-flight prefix: the forward's x = fmaf(ds, v, x) with v = v0 until the first in-box sample
  float px = p0[0], py = p0[1], pz = p0[2];
  unsigned e = 0;
  while (e < K && !inbounds(V, px, py, pz)) {
    px = fmaf(ds, v0[0], px); py = fmaf(ds, v0[1], py); pz = fmaf(ds, v0[2], pz);
    ++e;
  }
  if (e == K) {                                                           // never sampled inside: xt = p0, vt = v0
    g.dp[0] = dx[0]; g.dp[1] = dx[1]; g.dp[2] = dx[2]; g.dv[0] = dv[0]; g.dv[1] = dv[1]; g.dv[2] = dv[2];
    return g;
  }
  RevMarch r;
  rev_seed(r, ds, xt, vt, dx, dv);
  rev_sampled(V, ds, grad_scale, r, K, e, px, py, pz, taps, sink, term);
  rev_flight(r, e, ds);
  rev_store(r, g.dp, g.dv);
  g.steps = K - e;
  return g;
}

// Ray-state adjoint of trace for ONE ray (drrt_last_steps gives K): the reverse march with no term.  No contribution to
// dL/dn is formed.
template <typename TapFn>
DRRT_HD RayGrad backtrace_ray_state(const Vol& V, float ds, int max_steps, unsigned K, const float p0[3],
                                    const float v0[3], const float xt[3], const float vt[3], const float dx[3],
                                    const float dv[3], TapFn&& taps) {
  return integral_backtrace_ray(V, ds, 1.f, max_steps, K, p0, v0, xt, vt, dx, dv, taps, NoSink{}, NoTerm{});
}

// ---- optical path length -------------------------------------------------------------------------------------------
// The march integrates dx/dsigma = v, dv/dsigma = n grad n, so |v| = n and the optical path length int n dl is
// int n^2 dsigma: opl = sum_{k<K} ds n_k^2 over the masked samples n_k that fwd_step_c<0> takes at x_k (0 while the ray
// is not inside: free flight outside the box adds nothing), accumulated in fp32 as opl = fmaf(ds n_k, n_k, opl) in
// iteration order from 0.f.  Not in the reference.
struct OplIntegrand {
  float ds, opl = 0.f;
  DRRT_HD void operator()(const Cell&, bool, float n) { opl = fmaf(ds * n, n, opl); }
  DRRT_HD void step(const FwdState&) {}
};

// trace for ONE ray, with its optical path length.
template <typename TapFn>
DRRT_HD RayOut trace_opl_ray(const Vol& V, float ds, int max_steps, const float p[3], const float v[3], TapFn&& taps,
                             float& opl) {
  OplIntegrand q{ds};
  const RayOut o = trace_integral_ray(V, ds, max_steps, p, v, taps, q);
  opl = q.opl;
  return o;
}

// Adjoint of trace_opl_ray for ONE ray: dL/dpos, dL/dvel AND the contributions to dL/dn, from the seeds (dx, dv, dopl) on
// (xt, vt, opl).  Each reverse iteration uses
//   dn = mu . grad n_k + 2 dopl n_k
// wherever backtrace_ray_state uses mu . grad n_k: d opl / d n_k = 2 ds n_k adds 2 dopl n_k ds to the value weight of
// the splat, and d opl / d x_k = 2 ds n_k grad n_k adds the same multiple of grad n_k to lambda, which is what adj_recur
// does with dn.
struct OplTerm {
  float dopl2;                               // 2 dopl
  DRRT_HD void enter(const Vol&, const Cell&, AdjState&) {}
  DRRT_HD float dn(const Vol&, const Cell&, const AdjSample& m, float mg) { return fmaf(dopl2, m.n, mg); }
  DRRT_HD void pull(const Vol&, const Cell&, const AdjSample&, AdjState&, bool) {}
  DRRT_HD void after() {}
};

template <typename TapFn, typename Sink>
DRRT_HD RayGrad opl_backtrace_ray(const Vol& V, float ds, float grad_scale, int max_steps, unsigned K, const float p0[3],
                                  const float v0[3], const float xt[3], const float vt[3], const float dx[3],
                                  const float dv[3], float dopl, TapFn&& taps, Sink&& sink) {
  return integral_backtrace_ray(V, ds, grad_scale, max_steps, K, p0, v0, xt, vt, dx, dv, taps, sink, OplTerm{dopl + dopl});
}

// ---- line integral of a second field ---------------------------------------------------------------------------------
// tau = int a dl of a second voxel field `a` (absorption, emission, group index) on the grid of n, along the bent ray:
// |v| = n, so dl = n dsigma and tau = sum_{k<K} ds n_k a_k, a_k the trilinear sample of the field at the cell, the weights
// and under the mask of n_k (0 while the ray is not inside), accumulated in fp32 as tau = fmaf(ds n_k, a_k, tau) in
// iteration order from 0.f.  With a = n (the same values) that is trace_opl_ray's opl bit for bit.  Not in the reference.

// The value weights of a splat alone: corner(a,b,c) = val X_a Y_b Z_c (splat_weights without its gradient part).
DRRT_HD Corners value_weights(float wx, float wy, float wz, float val) {
  const float x1 = wx, x0 = 1.f - wx, y1 = wy, y0 = 1.f - wy, z1 = wz, z0 = 1.f - wz;
  const float a0 = val * x0, a1 = val * x1;
  const float yz00 = y0 * z0, yz10 = y1 * z0, yz01 = y0 * z1, yz11 = y1 * z1;
  Corners c;
  c.c000 = yz00 * a0;  c.c100 = yz00 * a1;
  c.c010 = yz10 * a0;  c.c110 = yz10 * a1;
  c.c001 = yz01 * a0;  c.c101 = yz01 * a1;
  c.c011 = yz11 * a0;  c.c111 = yz11 * a1;
  return c;
}

template <typename FieldTapFn>
struct FieldIntegrand {
  FieldTapFn& ftaps;
  float ds, tau = 0.f;
  DRRT_HD void operator()(const Cell& c, bool inside, float n) {
    float a = 0.f;
    if (inside) a = interp<false>(ftaps(c), c.wx, c.wy, c.wz).n;
    tau = fmaf(ds * n, a, tau);
  }
  DRRT_HD void step(const FwdState&) {}
};

// trace for ONE ray, with the line integral of the field whose taps `ftaps(c)` returns (`taps(c)`: those of n).
template <typename TapFn, typename FieldTapFn>
DRRT_HD RayOut trace_field_ray(const Vol& V, float ds, int max_steps, const float p[3], const float v[3], TapFn&& taps,
                               FieldTapFn&& ftaps, float& tau) {
  FieldIntegrand<FieldTapFn> q{ftaps, ds};
  const RayOut o = trace_integral_ray(V, ds, max_steps, p, v, taps, q);
  tau = q.tau;
  return o;
}

// Adjoint of trace_field_ray for ONE ray: dL/dpos, dL/dvel and the contributions to dL/dn AND dL/da, from the seeds
// (dx, dv, dtau) on (xt, vt, tau).  With a_k, grad a_k the sample of the field at the cell of n_k (grad a_k scaled by
// 1 / h like grad n_k), each reverse iteration uses
//   dn = mu . grad n_k + dtau a_k                    (d tau / d n_k = ds a_k)
// where backtrace_ray_state uses mu . grad n_k, which also puts dtau ds a_k grad n_k into lambda (adj_recur), and adds the
// term no other march has, the pull of the field's own gradient on the sample position,
//   lambda += (dtau ds n_k) grad a_k                 (d tau / d x_k = ds (a_k grad n_k + n_k grad a_k))
// `fsink(c, val)` receives the contribution to dL/da, val = dtau ds n_k: the caller adds value_weights(c.wx, c.wy, c.wz,
// val) at the taps of c (tau is linear in a: no gradient splat, no grad_scale, the exact discrete derivative either way).
template <typename FieldTapFn, typename FieldSink>
struct FieldTerm {
  FieldTapFn& ftaps;
  FieldSink& fsink;
  float dtau, dtds;                          // dtau, dtau ds
  Sample a;
  DRRT_HD void enter(const Vol&, const Cell&, AdjState&) {}
  DRRT_HD float dn(const Vol&, const Cell& c, const AdjSample& m, float mg) {
    a = interp<false>(ftaps(c), c.wx, c.wy, c.wz);
    return fmaf(dtau, a.n, mg);
  }
  DRRT_HD void pull(const Vol& V, const Cell& c, const AdjSample& m, AdjState& s, bool) {
    const float fv = dtds * m.n;                                          // dtau ds n_k
    fsink(c, fv);
    s.lx = fmaf(fv, a.gx * V.inv_h, s.lx); s.ly = fmaf(fv, a.gy * V.inv_h, s.ly); s.lz = fmaf(fv, a.gz * V.inv_h, s.lz);
  }
  DRRT_HD void after() {}
};

template <typename TapFn, typename FieldTapFn, typename Sink, typename FieldSink>
DRRT_HD RayGrad field_backtrace_ray(const Vol& V, float ds, float grad_scale, int max_steps, unsigned K, const float p0[3],
                                    const float v0[3], const float xt[3], const float vt[3], const float dx[3],
                                    const float dv[3], float dtau, TapFn&& taps, FieldTapFn&& ftaps, Sink&& sink,
                                    FieldSink&& fsink) {
  FieldTerm<FieldTapFn, FieldSink> term{ftaps, fsink, dtau, dtau * ds, {}};
  return integral_backtrace_ray(V, ds, grad_scale, max_steps, K, p0, v0, xt, vt, dx, dv, taps, sink, term);
}

// ---- emission with self-absorption -----------------------------------------------------------------------------------
// rad = int e(s) exp(-int_0^s a) ds: what a camera sees through a medium that emits (e) and absorbs (a) along the ray that
// n bends.  Two voxel fields on the grid of n.  With w_k = ds n_k (n_k masked as in trace_opl_ray) and e_k, a_k the
// trilinear samples of the two fields at the cell and weights of n_k, in fp32 and in iteration order from tau = rad = 0:
//   T_k       = exp_neg(tau_k)                 transmittance in front of sample k
//   rad_{k+1} = fmaf(T_k w_k, e_k, rad_k)      emit, then absorb
//   tau_{k+1} = fmaf(w_k, a_k, tau_k)          trace_field_ray's tau of the field a, bit for bit
// With a = 0 everywhere T_k = exp_neg(0) = 1.0f exactly and rad is trace_field_ray's tau of the field e bit for bit.  Not
// in the reference.

// exp(-t) for the transmittance, as an explicit sequence of +, *, fmaf, comparisons, int <-> float conversions of exact
// integers and one bit cast: no libm call and no device intrinsic, so the host build and the gfx950 kernel agree bit for
// bit under -ffp-contract=off.  x = -t is clamped to [-87, 87], where the result is a normal fp32 (negative a, i.e. gain,
// is legal input); NaN in gives NaN out, and the float -> int conversion never sees it.  x = k ln2 + r with k = round(x
// log2 e), |k| <= 126, and r in about [-ln2 / 2, ln2 / 2] by a two-constant (Cody-Waite) reduction whose first product is
// exact; exp(r) is the degree-7 Taylor polynomial in Horner form (truncation <= 5.2e-9 relative on that interval), scaled
// by 2^k through the exponent field.  Relative error against float64 exp over the clamped range and at all reduction
// boundaries: 7.9e-8 measured (tests/test_emission.py::test_exp_neg); exp_neg(0) == 1.0f exactly.
DRRT_HD float exp_neg(float t) {
  float x = -t;
  x = x < -87.f ? -87.f : x;
  x = x > 87.f ? 87.f : x;
  const bool num = (x == x);
  const float xs = num ? x : 0.f;                                         // what the conversion below sees is in [-87, 87]
  const float kf0 = xs * 1.44269504088896341f;
  const int k = (int)(kf0 + (kf0 >= 0.f ? 0.5f : -0.5f));                 // round to nearest, |k| <= 126
  const float kf = (float)k;
  float r = fmaf(-kf, 0.693145751953125f, xs);                            // ln2's upper bits: 9 trailing zeros, kf ln2_hi exact
  r = fmaf(-kf, 1.428606765330187e-06f, r);
  float p = 1.f / 5040.f;
  p = fmaf(p, r, 1.f / 720.f);
  p = fmaf(p, r, 1.f / 120.f);
  p = fmaf(p, r, 1.f / 24.f);
  p = fmaf(p, r, 1.f / 6.f);
  p = fmaf(p, r, 0.5f);
  p = fmaf(p, r, 1.f);
  p = fmaf(p, r, 1.f);
  const float scale = __builtin_bit_cast(float, (uint32_t)(k + 127) << 23);   // 2^k, k + 127 in [1, 253]
  return num ? p * scale : x;
}

template <typename EmisTapFn, typename AbsTapFn>
struct EmissionIntegrand {
  EmisTapFn& etaps;
  AbsTapFn& ataps;
  float ds, rad = 0.f, tau = 0.f;
  DRRT_HD void operator()(const Cell& c, bool inside, float n) {
    float a = 0.f, e = 0.f;
    if (inside) {
      e = interp<false>(etaps(c), c.wx, c.wy, c.wz).n;
      a = interp<false>(ataps(c), c.wx, c.wy, c.wz).n;
    }
    const float w = ds * n;
    rad = fmaf(exp_neg(tau) * w, e, rad);                                 // emit with the transmittance in front of the sample
    tau = fmaf(w, a, tau);                                                // then absorb
  }
  DRRT_HD void step(const FwdState&) {}
};

// trace for ONE ray with the emission integral; `taps(c)`: the taps of n, `etaps(c)` / `ataps(c)`: those of the emission and
// absorption fields.  tau is trace_field_ray's with the field a, bit for bit; a ray that never samples inside has
// rad = tau = 0.
template <typename TapFn, typename EmisTapFn, typename AbsTapFn>
DRRT_HD RayOut trace_emission_ray(const Vol& V, float ds, int max_steps, const float p[3], const float v[3], TapFn&& taps,
                                  EmisTapFn&& etaps, AbsTapFn&& ataps, float& rad, float& tau) {
  EmissionIntegrand<EmisTapFn, AbsTapFn> q{etaps, ataps, ds};
  const RayOut o = trace_integral_ray(V, ds, max_steps, p, v, taps, q);
  rad = q.rad; tau = q.tau;
  return o;
}

// Adjoint of trace_emission_ray for ONE ray: dL/dpos, dL/dvel and the contributions to dL/dn, dL/de AND dL/da, from the
// seeds (dx, dv, drad, dtau) on (xt, vt, rad, tau) and the forward's tau.  Two running scalars: t, the optical depth in
// front of the sample, which starts at the forward's tau and is stepped back by t = fmaf(-w, a_k, t) (tau_k again, to
// rounding), and
//   P_{k+1} = dtau - drad sum_{j>k} T_j w_j e_j        (d L / d tau_{k+1}: every later emission is dimmed by this sample)
// which starts at dtau.  With ce = drad exp_neg(tau_k) each reverse iteration uses
//   dn = mu . grad n_k + (ce e_k + P a_k)              (d L / d w_k = drad T_k e_k + P_{k+1} a_k)
// where backtrace_ray_state uses mu . grad n_k, gives `esink(c, ce w)` the contribution to dL/de and `asink(c, P w)` that
// to dL/da (value weights at the 8 taps of c, as field_backtrace_ray's fsink), adds the pull of both fields' gradients on
// the sample position, lambda += (ce w) grad e_k + (P w) grad a_k, BEFORE adj_recur, and then P = fmaf(-(ce w), e_k, P).
// T is always recovered from tau, never by dividing T, so an opaque ray (T at the clamp of exp_neg) gets finite gradients.
// Because tau_k is recomputed by subtraction, T_k here differs from the forward's by rounding only: dL/de, dL/da and the
// ray gradients are the derivative of the discrete forward to fp32 rounding, with either setting of grad_scale; dL/dn is
// the same derivative with grad_scale = 1 / h (DRRT_FLAG_CORRECTED_H).  With drad = 0 this is field_backtrace_ray with the
// field a: ce = 0, P stays dtau, and nothing reaches dL/de.
template <typename EmisTapFn, typename AbsTapFn, typename EmisSink, typename AbsSink>
struct EmissionTerm {
  EmisTapFn& etaps;
  AbsTapFn& ataps;
  EmisSink& esink;
  AbsSink& asink;
  float ds, drad, t, P;                      // t starts at the forward's tau, P at dtau
  Sample em, ab;
  float w, ce, ev;
  DRRT_HD void enter(const Vol&, const Cell&, AdjState&) {}
  DRRT_HD float dn(const Vol&, const Cell& c, const AdjSample& m, float mg) {
    em = interp<false>(etaps(c), c.wx, c.wy, c.wz);
    ab = interp<false>(ataps(c), c.wx, c.wy, c.wz);
    w = ds * m.n;
    t = fmaf(-w, ab.n, t);                                                // tau_k
    ce = drad * exp_neg(t);
    return mg + fmaf(ce, em.n, P * ab.n);
  }
  DRRT_HD void pull(const Vol& V, const Cell& c, const AdjSample&, AdjState& s, bool) {
    ev = ce * w;
    const float av = P * w;
    esink(c, ev);
    asink(c, av);
    s.lx = fmaf(ev, em.gx * V.inv_h, s.lx); s.ly = fmaf(ev, em.gy * V.inv_h, s.ly); s.lz = fmaf(ev, em.gz * V.inv_h, s.lz);
    s.lx = fmaf(av, ab.gx * V.inv_h, s.lx); s.ly = fmaf(av, ab.gy * V.inv_h, s.ly); s.lz = fmaf(av, ab.gz * V.inv_h, s.lz);
  }
  DRRT_HD void after() { P = fmaf(-ev, em.n, P); }
};

template <typename TapFn, typename EmisTapFn, typename AbsTapFn, typename Sink, typename EmisSink, typename AbsSink>
DRRT_HD RayGrad emission_backtrace_ray(const Vol& V, float ds, float grad_scale, int max_steps, unsigned K,
                                       const float p0[3], const float v0[3], const float xt[3], const float vt[3],
                                       float tau, const float dx[3], const float dv[3], float drad, float dtau,
                                       TapFn&& taps, EmisTapFn&& etaps, AbsTapFn&& ataps, Sink&& sink, EmisSink&& esink,
                                       AbsSink&& asink) {
  EmissionTerm<EmisTapFn, AbsTapFn, EmisSink, AbsSink> term{etaps, ataps, esink, asink, ds, drad, tau, dtau, {}, {},
                                                            0.f, 0.f, 0.f};
  return integral_backtrace_ray(V, ds, grad_scale, max_steps, K, p0, v0, xt, vt, dx, dv, taps, sink, term);
}

// ---- line integral of a vector field ---------------------------------------------------------------------------------
// circ = int u . dl of a vector field u (flow velocity, n_e B) given as three component planes on the grid of n, along the
// bent ray: plane c pairs with component c of pos / vel (x, y, z).  With u_k the trilinear sample of the three planes at the
// cell, the weights and under the mask of n_k (0 while the ray is not inside) and v_{k+1} the velocity BEHIND the update from
// sample k -- the one that carries the ray from x_k to x_{k+1} --
//   circ = sum_{k<K} ds (u_k . v_{k+1}) = sum_k u(x_k) . (x_{k+1} - x_k)
// accumulated in fp32 in iteration order from 0.f as t = ux vx; t = fmaf(uy, vy, t); t = fmaf(uz, vz, t);
// circ = fmaf(ds, t, circ).  The sum telescopes: for a uniform u, circ = u . (xt - x_e), x_e the first in-box sample.  Not
// in the reference.
template <typename VecTapFn>
struct VectorIntegrand {
  VecTapFn& vtaps;                           // vtaps(c, k): the 8 taps of plane k at cell c
  float ds, circ = 0.f;
  float ux = 0.f, uy = 0.f, uz = 0.f;
  DRRT_HD void operator()(const Cell& c, bool inside, float) {
    ux = uy = uz = 0.f;
    if (inside) {
      ux = interp<false>(vtaps(c, 0), c.wx, c.wy, c.wz).n;
      uy = interp<false>(vtaps(c, 1), c.wx, c.wy, c.wz).n;
      uz = interp<false>(vtaps(c, 2), c.wx, c.wy, c.wz).n;
    }
  }
  DRRT_HD void step(const FwdState& s) {
    float t = ux * s.vx;
    t = fmaf(uy, s.vy, t);
    t = fmaf(uz, s.vz, t);
    circ = fmaf(ds, t, circ);
  }
};

// trace for ONE ray, with the line integral of the vector field whose taps `vtaps(c, k)` returns (`taps(c)`: those of n).
template <typename TapFn, typename VecTapFn>
DRRT_HD RayOut trace_vector_ray(const Vol& V, float ds, int max_steps, const float p[3], const float v[3], TapFn&& taps,
                                VecTapFn&& vtaps, float& circ) {
  VectorIntegrand<VecTapFn> q{vtaps, ds};
  const RayOut o = trace_integral_ray(V, ds, max_steps, p, v, taps, q);
  circ = q.circ;
  return o;
}

// Adjoint of trace_vector_ray for ONE ray: dL/dpos, dL/dvel and the contributions to dL/dn AND the three planes of dL/du,
// from the seeds (dx, dv, dcirc) on (xt, vt, circ).  The summand ds u(x_k) . v_{k+1} depends on the velocity the reverse
// march holds when it arrives at x_k, so the term acts in `enter`, before the sample steps v back: with g = dcirc ds,
//   mu += g u_k                                      (d circ / d v_{k+1} = ds u_k): the seed on v_{k+1}, there before
//                                                    dn = mu . grad n_k is formed, so the splat into dL/dn sees it
//   w   = g v_{k+1}                                  kept for pull
// and in `pull`, `vsink(k, c, w[k])` receives the contribution to plane k of dL/du (value weights at the taps of c: circ
// is linear in u, no gradient splat, no grad_scale) and
//   lambda += (grad u_k)^T w                         (d circ / d x_k = ds (grad u_k)^T v_{k+1}, grad u_k scaled by 1 / h)
// dn, the contribution to dL/dn, adj_recur and the closing dvel = mu_prev + e ds lambda are the skeleton's; mu_prev is taken
// behind the seed.  With dcirc = 0 this is backtrace_ray_state with the contributions to dL/dn.
template <typename VecTapFn, typename VecSink>
struct VectorTerm {
  VecTapFn& vtaps;
  VecSink& vsink;
  float g;                                   // dcirc ds
  Sample ux, uy, uz;
  float wx, wy, wz;
  DRRT_HD void enter(const Vol&, const Cell& c, AdjState& s) {
    ux = interp<false>(vtaps(c, 0), c.wx, c.wy, c.wz);
    uy = interp<false>(vtaps(c, 1), c.wx, c.wy, c.wz);
    uz = interp<false>(vtaps(c, 2), c.wx, c.wy, c.wz);
    wx = g * s.vx; wy = g * s.vy; wz = g * s.vz;
    s.mx = fmaf(g, ux.n, s.mx); s.my = fmaf(g, uy.n, s.my); s.mz = fmaf(g, uz.n, s.mz);
  }
  DRRT_HD float dn(const Vol&, const Cell&, const AdjSample&, float mg) { return mg; }
  DRRT_HD void pull(const Vol& V, const Cell& c, const AdjSample&, AdjState& s, bool) {
    vsink(0, c, wx); vsink(1, c, wy); vsink(2, c, wz);
    s.lx = fmaf(dot3(ux.gx, uy.gx, uz.gx, wx, wy, wz), V.inv_h, s.lx);
    s.ly = fmaf(dot3(ux.gy, uy.gy, uz.gy, wx, wy, wz), V.inv_h, s.ly);
    s.lz = fmaf(dot3(ux.gz, uy.gz, uz.gz, wx, wy, wz), V.inv_h, s.lz);
  }
  DRRT_HD void after() {}
};

template <typename TapFn, typename VecTapFn, typename Sink, typename VecSink>
DRRT_HD RayGrad vector_backtrace_ray(const Vol& V, float ds, float grad_scale, int max_steps, unsigned K, const float p0[3],
                                     const float v0[3], const float xt[3], const float vt[3], const float dx[3],
                                     const float dv[3], float dcirc, TapFn&& taps, VecTapFn&& vtaps, Sink&& sink,
                                     VecSink&& vsink) {
  VectorTerm<VecTapFn, VecSink> term{vtaps, vsink, dcirc * ds, {}, {}, {}, 0.f, 0.f, 0.f};
  return integral_backtrace_ray(V, ds, grad_scale, max_steps, K, p0, v0, xt, vt, dx, dv, taps, sink, term);
}

// ---- ray paths ---------------------------------------------------------------------------------------------------------
// Where the ray went: the march's state in front of every stride-th iteration, as two series of M entries per ray, the
// positions (path) and, for a caller that asks for it, the velocities beside them (vpath: the march's phase-space state).
// With K the ray's iteration count, x_k the marching position in front of iteration k (x_0 = p, the march's own fp32 values)
// and v_k the marching velocity there (v_0 = v, and for k >= 1 the velocity that carried the ray from x_{k-1} to x_k,
// x_k = fmaf(ds, v_k, x_{k-1}) in fwd_step_c),
//   count    = min(M, ceil(K / stride))              the strided samples with j stride < K that fit
//   path[j]  = x_{j stride},  vpath[j] = v_{j stride}   for j < count
//   path[j]  = xt,            vpath[j] = vt             for count <= j < M
// The padding makes a series that is long enough end on the exit state (xt, vt): a ray that never samples inside the box
// has xt = p and vt = v (Q6), and vt is the stale v for a failed ray (Q6).  M stride < K truncates the series (no padding,
// no error).  x_K, the position behind the last iteration, is no sample: it is xt for a ray that left through a face.
// |v| = n along the march, so |vpath[j]| is the refractive index the ray saw there.  One routine pair does this,
// trace_phase_ray / phase_backtrace_ray; path alone is the same pair with the velocity series absent -- trace_path_ray
// drops the velocities in front of the caller's store, path_backtrace_ray seeds none (NoVSeed) -- and every other output,
// and the adjoint without a seed on vpath, is bit for bit what it is with the series.  Not in the reference.
constexpr unsigned path_count(unsigned K, unsigned stride, unsigned M) {
  const unsigned all = K ? (K - 1u) / stride + 1u : 0u;
  return all < M ? all : M;
}

// `store(j, x, y, z, vx, vy, vz)` writes path[j] and vpath[j] of the ray.  The iteration behind which the next sample is due
// is counted down to (no division in the loop).  The state behind iteration `it` is (x_{it+1}, v_{it+1}): it is written when
// it + 1 is a multiple of stride, the series has room, and the iteration did not flag the ray (then K = it + 1 and x_K is no
// sample).  A failed ray (K = max_steps, never flagged) may write x_K when stride divides K; that entry is padding, and
// xt = x_K for such a ray.
template <typename StoreFn>
struct PathIntegrand {
  StoreFn& store;
  unsigned stride, M, cd, j;
  DRRT_HD void operator()(const Cell&, bool, float) {}
  DRRT_HD void step(const FwdState& s) {
    if (--cd != 0u) return;
    cd = stride;
    if (!s.esc & (j < M)) store(j, s.x, s.y, s.z, s.vx, s.vy, s.vz);
    ++j;
  }
};

// trace for ONE ray, with both series: stride >= 1, M >= 1.  All M entries are written: sample 0 in front of the loop, the
// samples from the loop, the padding behind it.
template <typename TapFn, typename StoreFn>
DRRT_HD RayOut trace_phase_ray(const Vol& V, float ds, int max_steps, const float p[3], const float v[3], unsigned stride,
                               unsigned M, TapFn&& taps, StoreFn&& store, unsigned& count) {
  store(0u, p[0], p[1], p[2], v[0], v[1], v[2]);
  PathIntegrand<StoreFn> q{store, stride, M, stride, 1u};
  const RayOut o = trace_integral_ray(V, ds, max_steps, p, v, taps, q);
  count = path_count(o.steps, stride, M);
  for (unsigned j = count; j < M; ++j) store(j, o.xt[0], o.xt[1], o.xt[2], o.vt[0], o.vt[1], o.vt[2]);
  return o;
}
// with the positions alone: `store(j, x, y, z)` writes path[j]
template <typename TapFn, typename StoreFn>
DRRT_HD RayOut trace_path_ray(const Vol& V, float ds, int max_steps, const float p[3], const float v[3], unsigned stride,
                              unsigned M, TapFn&& taps, StoreFn&& store, unsigned& count) {
  auto positions = [&](unsigned j, float x, float y, float z, float, float, float) { store(j, x, y, z); };
  return trace_phase_ray(V, ds, max_steps, p, v, stride, M, taps, positions, count);
}

// Adjoint of trace_phase_ray for ONE ray: dL/dpos, dL/dvel and the contributions to dL/dn from the seeds (dx, dv) on
// (xt, vt), `seed(j, g)`, which writes the seed on path[j] to g[3] (zeros when there is none), and `vseed(j, g)`, which
// writes the seed on vpath[j] to g[3] and returns true, or returns false when there is none (nothing is added then), with K
// and count held fixed.  Where each kind of seed enters:
//   * a sample x_k, k > e: the reverse iteration that arrives at x_k adds its seed to lambda in `pull`, in front of
//     adj_recur, whose closing mu += ds lambda must see it (x_k = x_{k-1} + ds v_k);
//   * a sample v_k, e < k < K, enters only through x_k = x_{k-1} + ds v_k and v_{k+1} = v_k + ..., so its seed is one on
//     the total adjoint of v_k: mu when the reverse iteration that arrives at x_{k-1} begins.  It is added in `enter`, in
//     front of that iteration's sample, so that dn, the contribution to dL/dn and q (dL/dvel) see it -- one reverse
//     iteration behind the position seed on x_k; the sample k = e + 1 is seeded in the entry iteration.
// The iterations are counted down to the next sample as in the forward.  What the reverse march does not reach is added
// around it, in this order:
//   * padding: the seeds on path[count .. M-1] / vpath[count .. M-1] are seeds on xt / vt and are added to dx / dv in
//     ascending j, in fp32, before the march is initialised, so mu = dv + ds dx sees them;
//   * prefix: the samples x_k = p + k ds v of the free flight in front of the box, k <= e (x_e included: the reverse march
//     ends on lambda = dL/dx_e), are added to the result behind the march in ascending j: dpos += g,
//     dvel = fmaf((float)k * ds, g, dvel), k = j stride -- the way the skeleton forms e ds.  v_k = v bit for bit for
//     k <= e, so the velocity seeds of the prefix are added to dvel behind the position seeds, in ascending j; they add
//     nothing to dpos.
// A ray that never sampled inside (e = K) returns (dx, dv) with its padding and prefix seeds (every vpath seed on dvel) and
// contributes nothing; a failed ray returns zeros (no seed is read).
template <typename SeedFn, typename VSeedFn>
struct PathTerm {
  SeedFn& seed;
  VSeedFn& vseed;
  unsigned stride, cd, cdv;                  // cd / cdv: reverse iterations until one arrives at x_k / x_{k-1} of a sample k
  int j, jv;                                 // the next sample of each series; < 0: none left
  DRRT_HD void enter(const Vol&, const Cell&, AdjState& s) {
    if (cdv-- != 0u) return;
    cdv = stride - 1u;
    if (jv >= 0) {
      float g[3];
      if (vseed((unsigned)jv, g)) { s.mx += g[0]; s.my += g[1]; s.mz += g[2]; }
    }
    --jv;
  }
  DRRT_HD float dn(const Vol&, const Cell&, const AdjSample&, float mg) { return mg; }
  DRRT_HD void pull(const Vol&, const Cell&, const AdjSample&, AdjState& s, bool entry) {
    if (cd-- != 0u) return;
    cd = stride - 1u;
    if ((j >= 0) & !entry) {
      float g[3];
      seed((unsigned)j, g);
      s.lx += g[0]; s.ly += g[1]; s.lz += g[2];
    }
    --j;
  }
  DRRT_HD void after() {}
};

template <typename TapFn, typename SeedFn, typename VSeedFn, typename Sink>
DRRT_HD RayGrad phase_backtrace_ray(const Vol& V, float ds, float grad_scale, int max_steps, unsigned K, const float p0[3],
                                    const float v0[3], const float xt[3], const float vt[3], const float dx[3],
                                    const float dv[3], unsigned stride, unsigned M, SeedFn&& seed, VSeedFn&& vseed,
                                    TapFn&& taps, Sink&& sink) {
  float dxp[3] = {dx[0], dx[1], dx[2]}, dvp[3] = {dv[0], dv[1], dv[2]};
  unsigned count = 0;
  const bool failed = max_steps <= 0 || K >= (unsigned)max_steps;
  if (!failed) {
    count = path_count(K, stride, M);
    for (unsigned j = count; j < M; ++j) {
      float g[3];
      seed(j, g);
      dxp[0] += g[0]; dxp[1] += g[1]; dxp[2] += g[2];
      if (vseed(j, g)) { dvp[0] += g[0]; dvp[1] += g[1]; dvp[2] += g[2]; }
    }
  }
  // the last sample is x_k, k = (count - 1) stride <= K - 1: the march arrives at x_k after K - 1 - k iterations and at
  // x_{k-1} one later (never for k = 0: the countdown then outlasts the march)
  const unsigned back = count ? (K - 1u) - (count - 1u) * stride : 0u;
  PathTerm<SeedFn, VSeedFn> term{seed, vseed, stride, back, back + 1u, (int)count - 1, (int)count - 1};
  RayGrad r = integral_backtrace_ray(V, ds, grad_scale, max_steps, K, p0, v0, xt, vt, dxp, dvp, taps, sink, term);
  if (r.failed) return r;
  const unsigned e = K - r.steps;                                         // the skeleton's free-flight prefix
  for (unsigned j = 0, k = 0; j < count && k <= e; ++j, k += stride) {
    float g[3];
    seed(j, g);
    const float kds = (float)k * ds;
    for (int a = 0; a < 3; ++a) { r.dp[a] += g[a]; r.dv[a] = fmaf(kds, g[a], r.dv[a]); }
  }
  for (unsigned j = 0, k = 0; j < count && k <= e; ++j, k += stride) {
    float g[3];
    if (vseed(j, g)) { r.dv[0] += g[0]; r.dv[1] += g[1]; r.dv[2] += g[2]; }
  }
  return r;
}
// Adjoint of trace_path_ray: no seed on vpath
template <typename TapFn, typename SeedFn, typename Sink>
DRRT_HD RayGrad path_backtrace_ray(const Vol& V, float ds, float grad_scale, int max_steps, unsigned K, const float p0[3],
                                   const float v0[3], const float xt[3], const float vt[3], const float dx[3],
                                   const float dv[3], unsigned stride, unsigned M, SeedFn&& seed, TapFn&& taps, Sink&& sink) {
  return phase_backtrace_ray(V, ds, grad_scale, max_steps, K, p0, v0, xt, vt, dx, dv, stride, M, seed, NoVSeed{}, taps, sink);
}

// ---- the fibre (cable) march: one forward loop, one record-anchored reverse march -------------------------------------
// trace_cable, with or without a line integral over the samples it takes anyway, is one loop; the adjoints that start
// from its closest-approach record are one reverse march.  Both skeletons are written once here; an operator supplies an
// integrand (forward) and a term (reverse), defined with its mathematics further down.  backtrace_cable, the reference's
// continuous adjoint, is a different march (cable_backtrace_ray).

// The LDS rule of the cable kernels: the block's dynamic LDS in bytes -- `nprof` profiles (floats) and `ngrad` f64
// accumulator arrays of rres entries each -- or 0 when everything goes to global memory: above kCableMaxRes, or when the
// need passes 48 KiB (one profile: rres <= 4096 with or without its gradient; two profiles: <= 4096 / 3072 / 2048 with
// 0 / 1 / 2 gradients).  Nothing to stage (rres, nprof < 1, ngrad < 0) is 0 as well.
constexpr int kCableMaxRes = 4096;
constexpr size_t kCableMaxLds = 49152;
DRRT_HD size_t cable_lds_bytes(int rres, int nprof, int ngrad) {
  const size_t need = (size_t)rres * (sizeof(float) * (size_t)nprof + sizeof(double) * (size_t)ngrad);
  return nprof >= 1 && ngrad >= 0 && rres <= kCableMaxRes && need <= kCableMaxLds ? need : 0;
}

// The forward loop for ONE ray (src/tracer.cpp:312-382): cable_fwd_step from (p, v) until the ray is flagged escaped, at
// most max_steps times.  `q.sample(C, s)` is called once per iteration in front of the step, s.x / s.z being where the
// step samples (unmasked, clamped beyond the radius); `q.latch()` whenever the step updated the record (strict <, :365).
// j is the iteration count at the last update (0: the record is the input).  An integrand owns its accumulator, which
// starts at 0.f and is updated in iteration order, and the copy it latches with the record (0.f when j = 0).
struct CableTrace { RayOut o; unsigned j; };

struct CableNoIntegrand {                    // trace_cable itself: nothing is integrated
  DRRT_HD void sample(const Cyl&, const FwdState&) {}
  DRRT_HD void latch() {}
};

template <typename Integrand>
DRRT_HD CableTrace cable_trace_integral_ray(const Cyl& C, float ds, int max_steps, const float p[3], const float v[3],
                                            const float tg[3], Integrand&& q) {
  FwdState s;
  s.x = p[0]; s.y = p[1]; s.z = p[2]; s.vx = v[0]; s.vy = v[1]; s.vz = v[2];
  s.xtx = s.x; s.xty = s.y; s.xtz = s.z; s.vtx = s.vx; s.vty = s.vy; s.vtz = s.vz;
  s.aux0 = tg[0]; s.aux1 = tg[1]; s.aux2 = tg[2]; s.aux4 = s.aux5 = 0.f;
  float ex = s.x - tg[0], ey = s.y - tg[1], ez = s.z - tg[2];
  s.aux3 = dot3(ex, ey, ez, ex, ey, ez);                                  // :340
  s.inside = cyl_inbounds(C, s.x, s.y, s.z);                              // :344
  s.esc = false;
  CableTrace t;
  unsigned steps = 0;
  t.j = 0;
  for (int it = 0; it < max_steps; ++it) {
    const float best = s.aux3;
    q.sample(C, s);
    cable_fwd_step(C, ds, s);
    ++steps;
    if (s.aux3 < best) { q.latch(); t.j = steps; }
    if (s.esc) break;          // state is frozen once !active (:353-354): nothing changes later
  }
  RayOut& o = t.o;
  o.xt[0] = s.xtx; o.xt[1] = s.xty; o.xt[2] = s.xtz; o.vt[0] = s.vtx; o.vt[1] = s.vty; o.vt[2] = s.vtz;
  o.dist2 = s.aux3; o.esc = s.esc; o.act = !s.esc; o.steps = steps;
  return t;
}

// trace_cable for ONE ray
DRRT_HD RayOut cable_trace_ray(const Cyl& C, float ds, int max_steps, const float p[3], const float v[3],
                               const float tg[3]) {
  return cable_trace_integral_ray(C, ds, max_steps, p, v, tg, CableNoIntegrand{}).o;
}

// backtrace_cable for ONE ray (src/tracer.cpp:511-567); sink(i0, i1, a0, a1)
template <typename Sink>
DRRT_HD unsigned cable_backtrace_ray(const Cyl& C, float ds, int max_steps, const float xt[3], const float vt[3],
                                     const float dx[3], const float dv[3], Sink&& sink) {
  AdjState s;
  s.x = xt[0]; s.y = xt[1]; s.z = xt[2]; s.vx = vt[0]; s.vy = vt[1]; s.vz = vt[2];
  s.lx = dx[0]; s.ly = dx[1]; s.lz = dx[2];                               // :536
  s.mx = fmaf(ds, dx[0], dv[0]); s.my = fmaf(ds, dx[1], dv[1]); s.mz = fmaf(ds, dx[2], dv[2]);  // :537
  s.active = !cyl_escaped(C, s.x, s.y, s.z, -s.vx, -s.vy, -s.vz);         // :540-541
  s.outside = false;
  unsigned steps = 0;
  for (int it = 0; it < max_steps && s.active; ++it) {
    int i0, i1; float a0, a1;
    if (!cable_adj_step(C, ds, s, i0, i1, a0, a1)) break;
    ++steps;
    sink(i0, i1, a0, a1);
  }
  return steps;
}

// The reverse march for ONE ray: dL/dpos, dL/dvel from the seeds (dx, dv) on the record (xt, vt) = (x_j, v_j), given the
// forward's input position p0 and the record's iteration j, and the contributions to dL/d(profile).
//   * The record is held fixed (as autograd through a masked select does); a seed on dist2 does not enter.
//   * j is the ONLY loop bound and may come from caller memory, so a j above max_steps (the forward's own bound: no
//     forward call returns one) does no iterations: zero gradients, failed = true.  A ray that ran out of steps still has
//     a valid record and a gradient.
//   * j reverse iterations from (xt, vt), seeded like cable_backtrace_ray (lambda = dx, mu = dv + ds dx), with neither its
//     backward-escape test nor its step bound; after the last one lambda = dL/dx_0 and the mu it was updated from is
//     dL/dv_0 (j = 0: the identity, no contribution).  There is no free-flight prefix: the cable march samples from p0 on.
//     The last reverse iteration samples at p0 itself instead of its reconstruction x_1 - ds v_1: a start exactly on a
//     profile knot or on the axis must see the forward's sample.
// What an operator adds is its `term`, called in this order in every reverse iteration, m the sample at x_k:
//   dn = term.dn(m, mu . grad n_k)        the factor of ds grad n_k that cable_adj_recur adds to lambda: dL / dn_k over ds
//   sink(i0, i1, a0, a1)                  cable_adj_step's two profile contributions for that dn (cylinder_volume::splat,
//                                         :113-148), formed with mu BEFORE cable_adj_recur updates it
//   term.after(C, m, s)                   the term's contributions to its own profile and its pulls on lambda, BEFORE
//                                         cable_adj_recur, whose closing mu += ds lambda must see them; a term touches
//                                         nothing else of s.  It may keep what dn() sampled for after(): both are
//                                         called, in this order, in every iteration
// A term takes the sample by value, as cable_adj_recur does and for its reason: by reference the compiler schedules the
// iteration of the rays-only field adjoint differently (measured 2 % slower on MI355X, NOTES.md).
struct CableNoTerm {                         // trace_cable itself: nothing is integrated
  DRRT_HD float dn(CylAdjSample, float mg) { return mg; }
  DRRT_HD void after(const Cyl&, CylAdjSample, AdjState&) {}
};

template <typename Term, typename Sink>
DRRT_HD RayGrad cable_record_backtrace_ray(const Cyl& C, float ds, int max_steps, const float p0[3], const float xt[3],
                                           const float vt[3], unsigned j, const float dx[3], const float dv[3],
                                           Term&& term, Sink&& sink) {
  RayGrad g;
  g.failed = max_steps < 0 || j > (unsigned)max_steps;
  g.steps = g.failed ? 0u : j;
  if (g.failed) {
    g.dp[0] = g.dp[1] = g.dp[2] = 0.f; g.dv[0] = g.dv[1] = g.dv[2] = 0.f;
    return g;
  }
  AdjState s;
  s.x = xt[0]; s.y = xt[1]; s.z = xt[2]; s.vx = vt[0]; s.vy = vt[1]; s.vz = vt[2];
  s.lx = dx[0]; s.ly = dx[1]; s.lz = dx[2];                               // :536
  s.mx = fmaf(ds, dx[0], dv[0]); s.my = fmaf(ds, dx[1], dv[1]); s.mz = fmaf(ds, dx[2], dv[2]);  // :537
  float qx = dv[0], qy = dv[1], qz = dv[2];                               // mu before its last update
  for (unsigned k = j; k > 0; --k) {
    s.x = fmaf(-ds, s.vx, s.x); s.y = fmaf(-ds, s.vy, s.y); s.z = fmaf(-ds, s.vz, s.z);   // :547
    if (k == 1u) { s.x = p0[0]; s.y = p0[1]; s.z = p0[2]; }              // the forward's first sample, as it took it
    const CylAdjSample m = cable_adj_sample(C, ds, s);
    const CylCell& c = m.c;
    const float dn = term.dn(m, fmaf(s.mz, m.gz, s.mx * m.gx));           // :557
    const float val = dn * ds;
    const float gv = (m.n * ds) * fmaf(s.mz, c.rhz, s.mx * c.rhx);
    const float gvh = gv * C.inv_h;
    sink(c.i0, c.i1, fmaf(val, 1.f - c.w0, -gvh), fmaf(val, c.w0, gvh));
    term.after(C, m, s);
    qx = s.mx; qy = s.my; qz = s.mz;
    cable_adj_recur(ds, s, m, dn);
  }
  g.dp[0] = s.lx; g.dp[1] = s.ly; g.dp[2] = s.lz;
  g.dv[0] = qx; g.dv[1] = qy; g.dv[2] = qz;
  return g;
}

// Ray-state adjoint of trace_cable for ONE ray, given only the forward's inputs (p0, v0) and its target.  The forward does
// not report j, so it is replayed with the forward loop itself: the replayed record is (xt, vt), the caller cannot hand in
// a mismatched pair, and the march's refusal cannot fire.  Then the reverse march with no term and no sink.  j = 0 is the
// identity whatever max_steps is; `failed` stays false; steps = replay + reverse iterations.  `rec` (optional) receives
// the replayed record.
struct CableRecord { float xt[3], vt[3]; unsigned j; };

DRRT_HD RayGrad cable_backtrace_ray_state(const Cyl& C, float ds, int max_steps, const float p0[3], const float v0[3],
                                          const float tg[3], const float dx[3], const float dv[3],
                                          CableRecord* rec = nullptr) {
  const CableTrace t = cable_trace_integral_ray(C, ds, max_steps, p0, v0, tg, CableNoIntegrand{});
  if (rec) {
    for (int k = 0; k < 3; ++k) { rec->xt[k] = t.o.xt[k]; rec->vt[k] = t.o.vt[k]; }
    rec->j = t.j;
  }
  RayGrad g;
  if (t.j == 0) {
    g.dp[0] = dx[0]; g.dp[1] = dx[1]; g.dp[2] = dx[2]; g.dv[0] = dv[0]; g.dv[1] = dv[1]; g.dv[2] = dv[2];
  } else {
    g = cable_record_backtrace_ray(C, ds, max_steps, p0, t.o.xt, t.o.vt, t.j, dx, dv, CableNoTerm{},
                                   [](int, int, float, float) {});
  }
  g.failed = false;
  g.steps = t.o.steps + t.j;
  return g;
}

// n at (px, pz) as cable_fwd_step samples it (its `f`): the same operations on the same operands, so a caller that
// evaluates it in front of cable_fwd_step gets the step's own value (the compiler merges the two).
DRRT_HD float cable_sample_n(const Cyl& C, float px, float pz) {
  const CylCell c = cyl_locate(C, px, pz);
  const float v0 = C.data[c.i0], v1 = C.data[c.i1];
  return fmaf(v1, c.w0, v0 * (1.f - c.w0));                               // :53
}

// trace_cable for ONE ray, with the optical path length up to its record and the record's iteration: acc =
// fmaf(ds n_k, n_k, acc) (OplIntegrand's sequence), n_k the step's own sample at x_k, so opl = sum_{k<j} ds n_k^2.  It is
// the integral of n along the path when the rays enter with |v| = n.  Not in the reference.
struct CableOplIntegrand {
  float ds, acc = 0.f, opl = 0.f;
  DRRT_HD void sample(const Cyl& C, const FwdState& s) {
    const float n = cable_sample_n(C, s.x, s.z);
    acc = fmaf(ds * n, n, acc);
  }
  DRRT_HD void latch() { opl = acc; }
};

DRRT_HD RayOut cable_trace_opl_ray(const Cyl& C, float ds, int max_steps, const float p[3], const float v[3],
                                   const float tg[3], float& opl, unsigned& j) {
  CableOplIntegrand q{ds};
  const CableTrace t = cable_trace_integral_ray(C, ds, max_steps, p, v, tg, q);
  opl = q.opl; j = t.j;
  return t.o;
}

// Adjoint of cable_trace_opl_ray for ONE ray, from the seeds (dx, dv, dopl) on (xt, vt, opl): the reverse march with
// dn = mu . grad n_k + 2 dopl n_k (d opl / d n_k = 2 ds n_k) where the ray-state adjoint has mu . grad n_k.
struct CableOplTerm {
  float dopl2;                               // 2 dopl
  DRRT_HD float dn(CylAdjSample m, float mg) { return fmaf(dopl2, m.n, mg); }
  DRRT_HD void after(const Cyl&, CylAdjSample, AdjState&) {}
};

template <typename Sink>
DRRT_HD RayGrad cable_opl_backtrace_ray(const Cyl& C, float ds, int max_steps, const float p0[3], const float xt[3],
                                        const float vt[3], unsigned j, const float dx[3], const float dv[3], float dopl,
                                        Sink&& sink) {
  return cable_record_backtrace_ray(C, ds, max_steps, p0, xt, vt, j, dx, dv, CableOplTerm{2.f * dopl}, sink);
}

// trace_cable for ONE ray, with the line integral of a second radial profile `fa` (C.rres samples on C's knots; it may be
// C.data itself, both are only read) up to its record, and the record's iteration.  a_k = cable_sample_n's operations on
// `fa` in the cell of the step's own sample n_k (unmasked, clamped beyond the radius like it); acc = fmaf(ds n_k, a_k, acc),
// so tau = sum_{k<j} ds n_k a_k.  With fa = C.data it is cable_trace_opl_ray's opl bit for bit.  It is the integral of a
// along the path when the rays enter with |v| = n.  Not in the reference.
struct CableFieldIntegrand {
  const float* fa;
  float ds, acc = 0.f, tau = 0.f;
  DRRT_HD void sample(const Cyl& C, const FwdState& s) {
    const CylCell c = cyl_locate(C, s.x, s.z);
    const float n = fmaf(C.data[c.i1], c.w0, C.data[c.i0] * (1.f - c.w0));    // cable_sample_n
    const float ak = fmaf(fa[c.i1], c.w0, fa[c.i0] * (1.f - c.w0));           // ... on the other profile
    acc = fmaf(ds * n, ak, acc);
  }
  DRRT_HD void latch() { tau = acc; }
};

DRRT_HD RayOut cable_trace_field_ray(const Cyl& C, const float* fa, float ds, int max_steps, const float p[3],
                                     const float v[3], const float tg[3], float& tau, unsigned& j) {
  CableFieldIntegrand q{fa, ds};
  const CableTrace t = cable_trace_integral_ray(C, ds, max_steps, p, v, tg, q);
  tau = q.tau; j = t.j;
  return t.o;
}

// Adjoint of cable_trace_field_ray for ONE ray, from the seeds (dx, dv, dtau) on (xt, vt, tau): the reverse march with,
// per iteration, in the cell (i0, i1, w0) of the sample:
//   dn = mu . grad n_k + dtau a_k                (d tau / d n_k = ds a_k)
//   fv = (dtau ds) n_k                           (d tau / d a_k); fsink(i0, i1, fv (1 - w0), fv w0), the contributions to
//                                                dL/d(fa)
//   lambda += fv a'_k rhat, a'_k = (fa[i1] - fa[i0]) / h   (a_k moves with x_k along fa's own radial slope)
// a' follows grad n's conventions by construction: rhat = 0 where cyl_locate says tiny, and i0 = i1 beyond the radius.
// dtau = 0 leaves cable_opl_backtrace_ray's iteration with dopl = 0 and sends zeros to fsink.
// Written out, not as a term of cable_record_backtrace_ray, whose iteration it restates with the three lines of its own:
// as a term, the kernels that store no ray gradients compiled differently and measured 0.4-0.8 % slower (NOTES.md).
template <typename Sink, typename FieldSink>
DRRT_HD RayGrad cable_field_backtrace_ray(const Cyl& C, const float* fa, float ds, int max_steps, const float p0[3],
                                          const float xt[3], const float vt[3], unsigned j, const float dx[3],
                                          const float dv[3], float dtau, Sink&& sink, FieldSink&& fsink) {
  RayGrad g;
  g.failed = max_steps < 0 || j > (unsigned)max_steps;
  g.steps = g.failed ? 0u : j;
  if (g.failed) {
    g.dp[0] = g.dp[1] = g.dp[2] = 0.f; g.dv[0] = g.dv[1] = g.dv[2] = 0.f;
    return g;
  }
  AdjState s;
  s.x = xt[0]; s.y = xt[1]; s.z = xt[2]; s.vx = vt[0]; s.vy = vt[1]; s.vz = vt[2];
  s.lx = dx[0]; s.ly = dx[1]; s.lz = dx[2];                               // :536
  s.mx = fmaf(ds, dx[0], dv[0]); s.my = fmaf(ds, dx[1], dv[1]); s.mz = fmaf(ds, dx[2], dv[2]);  // :537
  float qx = dv[0], qy = dv[1], qz = dv[2];                               // mu before its last update
  const float gds = dtau * ds;
  for (unsigned k = j; k > 0; --k) {
    s.x = fmaf(-ds, s.vx, s.x); s.y = fmaf(-ds, s.vy, s.y); s.z = fmaf(-ds, s.vz, s.z);   // :547
    if (k == 1u) { s.x = p0[0]; s.y = p0[1]; s.z = p0[2]; }              // the forward's first sample, as it took it
    const CylAdjSample m = cable_adj_sample(C, ds, s);
    const CylCell& c = m.c;
    const float f0 = fa[c.i0], f1 = fa[c.i1];
    const float w1 = 1.f - c.w0;
    const float ak = fmaf(f1, c.w0, f0 * w1);
    const float dn = fmaf(dtau, ak, fmaf(s.mz, m.gz, s.mx * m.gx));       // :557, plus d(ds n a)/dn / ds
    // cylinder_volume::splat (:113-148) as cable_adj_step forms it
    const float val = dn * ds;
    const float gv = (m.n * ds) * fmaf(s.mz, c.rhz, s.mx * c.rhx);
    const float gvh = gv * C.inv_h;
    sink(c.i0, c.i1, fmaf(val, w1, -gvh), fmaf(val, c.w0, gvh));
    const float fv = gds * m.n;                                           // d(ds n a)/da
    fsink(c.i0, c.i1, fv * w1, fv * c.w0);
    const float fp = fv * ((f1 - f0) * C.inv_h);                          // ... and through a's own radial slope
    s.lx = fmaf(fp, c.rhx, s.lx); s.lz = fmaf(fp, c.rhz, s.lz);
    qx = s.mx; qy = s.my; qz = s.mz;
    cable_adj_recur(ds, s, m, dn);
  }
  g.dp[0] = s.lx; g.dp[1] = s.ly; g.dp[2] = s.lz;
  g.dv[0] = qx; g.dv[1] = qy; g.dv[2] = qz;
  return g;
}

// Ray-state adjoint of trace_plane (MODE 1) / trace_sdf (MODE 2) for ONE ray: dL/dpos, dL/dvel from the seeds (dx, dv) on
// the record (xt, vt) = (x_j, v_j), given only the forward's inputs (p0, v0) and its plane / SDF.  j = the iteration count at
// the LAST cross (fwd_step_c :378-386), 0 when there was none (the record is the input).  Iteration k samples n grad n at x_k
// only when m_k, the forward's `inside` flag at that moment, was set; j and every m_k are held fixed (as autograd through a
// masked select does).
//   * The forward is replayed from (p0, v0) with fwd_init / fwd_step_c<MODE> themselves, looped as trace_ray loops them
//     (FULL = false: until the ray is flagged escaped, at most max_steps) or as ray_full does (FULL = true: exactly `total`
//     iterations of the reference's global loop, for the rays the first pass flags with `again`, see plane_again and
//     trace_ray<2>).  A flagged ray of the first pass returns after its replay: only its second pass knows the record.
//   * trace_plane, never flagged escaped (failmask set; xt is the final x, vt stale): zero gradient, failed = true.
//     trace_sdf has no such fix-up: a ray that never crosses keeps (xt, vt) = (p0, v0), j = 0.
//   * j = 0: the gradient is the identity (dx, dv).
//   * otherwise the iterations j-1 .. 0 are undone run by run, a run being a stretch [lo, hi) of equal m_k: the seeded
//     reverse run (rev_seed on the record, rev_sampled / rev_flight per run, x set to the replayed x_lo behind a flight).
//     First pass: the march stops at its first cross, so the masks are F^e T^(j-e) -- the run that ends at j is known from
//     the replay and what is left of it is the free-flight prefix from p0.  Second pass: the masks need not be monotone
//     (a ray that starts in bounds past its plane and heads back through it: T, F..F, T..T, F -- m_0 carries no plane term);
//     each earlier run is found by replaying the forward again up to it, so no mask is stored and any sequence is honoured.
//   * steps = every forward iteration replayed + every reverse iteration; fwd = the iterations of the first replay (the
//     ray's count in the forward's own statistics: its maximum over the call is the global loop count of the second pass).
// The 1/h of DRRT_FLAG_CORRECTED_H does not enter; no gradient flows to the plane, the SDF, h or ds.
// `taps(c)` returns the 8 taps of cell c of the index grid.  `rec` (optional) receives the replayed record.
struct StopRecord { float xt[3], vt[3]; unsigned j; bool esc; };
struct StopGrad { float dp[3], dv[3]; unsigned steps, fwd; bool failed, again; };

template <int MODE, bool FULL, typename TapFn>
DRRT_HD StopGrad stop_backtrace_ray_state(const Vol& V, const float* __restrict__ sdf, float ds, int max_steps,
                                          unsigned total, const float p0[3], const float v0[3], const float* pln_o,
                                          const float* pln_d, const float dx[3], const float dv[3], TapFn&& taps,
                                          StopRecord* rec = nullptr) {
  static_assert(MODE == 1 || MODE == 2, "trace_plane or trace_sdf");
  FwdState f;
  Cell c;
  fwd_begin<MODE>(V, p0, v0, pln_o, pln_d, f, c);
  const unsigned lim = FULL ? total : (max_steps > 0 ? (unsigned)max_steps : 0u);
  unsigned steps = 0, j = 0;
  unsigned lo = 0, jlo = 0;                          // first iteration of the current sampled run / of the one that ended at j
  float lx = f.x, ly = f.y, lz = f.z, jx = f.x, jy = f.y, jz = f.z;   // the positions sampled there
  bool prev = false;
  for (unsigned it = 0; it < lim; ++it) {
    const bool was = f.inside;
    if (was & !prev) { lo = it; lx = f.x; ly = f.y; lz = f.z; }
    prev = was;
    Taps t = taps_zero();
    if (was) t = taps(c);
    fwd_step_c<MODE>(V, sdf, ds, f, c, t);
    ++steps;
    if (was & !f.inside) { j = steps; jlo = lo; jx = lx; jy = ly; jz = lz; }     // cross: the record was written
    if (!FULL && f.esc) break;
  }
  if (rec) {
    rec->xt[0] = f.xtx; rec->xt[1] = f.xty; rec->xt[2] = f.xtz;
    rec->vt[0] = f.vtx; rec->vt[1] = f.vty; rec->vt[2] = f.vtz;
    if (MODE == 1 && !f.esc) { rec->xt[0] = f.x; rec->xt[1] = f.y; rec->xt[2] = f.z; }   // :167
    rec->j = j; rec->esc = f.esc;
  }
  StopGrad g;
  g.failed = false; g.again = false; g.fwd = steps; g.steps = steps;
  g.dp[0] = dx[0]; g.dp[1] = dx[1]; g.dp[2] = dx[2]; g.dv[0] = dv[0]; g.dv[1] = dv[1]; g.dv[2] = dv[2];
  if (MODE == 1 && !f.esc) {
    g.dp[0] = g.dp[1] = g.dp[2] = g.dv[0] = g.dv[1] = g.dv[2] = 0.f;
    g.failed = true;
    return g;
  }
  if (!FULL) {
    g.again = MODE == 1 ? (f.esc && plane_again(V, f)) : (f.esc & f.inside);
    if (g.again) return g;
  }
  if (j == 0) return g;
  const float xj[3] = {f.xtx, f.xty, f.xtz}, vj[3] = {f.vtx, f.vty, f.vtz};
  RevMarch r;
  rev_seed(r, ds, xj, vj, dx, dv);
  unsigned hi = j;
  bool sampled = true;
  lo = jlo; lx = jx; ly = jy; lz = jz;
  for (;;) {
    if (sampled) {
      rev_sampled(V, ds, 1.f, r, hi, lo, lx, ly, lz, taps, NoSink{}, NoTerm{});
      g.steps += hi - lo;
    } else {
      rev_flight(r, hi - lo, ds);
      r.s.x = lx; r.s.y = ly; r.s.z = lz;
    }
    hi = lo;
    if (hi == 0) break;
    if (!FULL) {                                     // F^e T^(j-e): the free-flight prefix from p0
      sampled = false; lo = 0;
      continue;
    }
    // the run that holds iteration hi - 1: replay the forward up to it
    fwd_begin<MODE>(V, p0, v0, pln_o, pln_d, f, c);
    for (unsigned it = 0;; ++it) {
      if (it == 0 || f.inside != prev) { lo = it; lx = f.x; ly = f.y; lz = f.z; }
      prev = f.inside;
      if (it == hi - 1u) break;
      Taps t = taps_zero();
      if (f.inside) t = taps(c);
      fwd_step_c<MODE>(V, sdf, ds, f, c, t);
      ++g.steps;
    }
    sampled = prev;
  }
  rev_store(r, g.dp, g.dv);
  return g;
}

// Ray-state adjoint of trace_target for ONE ray: dL/dpos, dL/dvel from the seeds (dx, dv) on the closest-approach record
// (xt, vt) = (x_j, v_j) and the seed dd2 on dist2 = |x_j - t|^2, given only the forward's inputs (p0, v0), its target t and
// `total`, the call's global loop count (the maximum of the phase-A iteration counts over the call's rays).  j = the iteration
// count at the LAST record update (strict <, :217; 0: the record is the input); j and the forward's `inside` masks are held
// fixed (as autograd through a masked select does).
//   * The forward is replayed from (p0, v0) with its own operations, looped as it loops them: phase A is fwd_init /
//     fwd_step_c<3> (what target_ray_a's fwd_step_r<3> runs on the taps it fetches) until the ray is flagged escaped, at
//     most max_steps: `done` iterations; phase B is the straight flight of target_ray_b over the iterations done .. total-1.
//     Phase A ends at the first cross, so its masks are F^e T^(done-e): e = the index of the first in-box sample (done
//     when there is none), x_e the position sampled there.
//   * The effective position seed is gx = dx + 2 dd2 (x_j - t), one fmaf per component.  j = 0: the result is (gx, dv).
//   * Otherwise the iterations j-1 .. 0 are undone with the seeded reverse run (rev_seed with gx on the record): the free
//     flight done .. j-1 of a record written after the escape (j > done), behind which the march continues from phase A's
//     end state; the sampled run e .. min(j, done)-1; the free flight of the prefix 0 .. e-1, where there is one.
//   * A ray that ran out of steps keeps its record and its gradient (as in the cable routine); `failed` only reports it.
//   * steps = the forward iterations replayed (done, plus total - done of phase B) + the reverse iterations of the sampled
//     run; fwd = done.
// The 1/h of DRRT_FLAG_CORRECTED_H does not enter; dL/dt = -2 dd2 (x_j - t) is a point-wise expression of the forward's
// outputs and is left to the caller.  `taps(c)` returns the 8 taps of cell c.  `rec` (optional) receives the replayed record.
struct TargetRecord { float xt[3], vt[3], dist2; unsigned j; };
struct TargetGrad { float dp[3], dv[3]; unsigned steps, fwd; bool failed; };
struct TargetReplay {
  FwdState f;              // phase A's end state: (x, v) is what phase B continues from, (xt, vt, aux3) the record so far
  unsigned done, j, e;
  float ex, ey, ez;        // x_e
};

// phase A of the forward, replayed: also the whole of the first pass, which needs `done` only
template <typename TapFn>
DRRT_HD void target_replay_a(const Vol& V, float ds, int max_steps, const float p0[3], const float v0[3], const float tg[3],
                             TapFn&& taps, TargetReplay& r) {
  FwdState& f = r.f;
  Cell c;
  fwd_begin<3>(V, p0, v0, tg, nullptr, f, c);
  unsigned steps = 0, j = 0, e = 0;
  bool entered = false;
  r.ex = f.x; r.ey = f.y; r.ez = f.z;
  for (int it = 0; it < max_steps; ++it) {
    const bool was = f.inside;
    if (was & !entered) { entered = true; e = steps; r.ex = f.x; r.ey = f.y; r.ez = f.z; }
    Taps t = taps_zero();
    if (was) t = taps(c);
    const float best = f.aux3;
    fwd_step_c<3>(V, nullptr, ds, f, c, t);
    ++steps;
    if (f.aux3 < best) j = steps;                                         // the record was updated (strict <, :217)
    if (f.esc) break;
  }
  r.done = steps; r.j = j; r.e = entered ? e : steps;
}

template <typename TapFn>
DRRT_HD TargetGrad target_backtrace_ray_state(const Vol& V, float ds, int max_steps, unsigned total, const float p0[3],
                                              const float v0[3], const float tg[3], const float dx[3], const float dv[3],
                                              float dd2, TapFn&& taps, TargetRecord* rec = nullptr) {
  TargetReplay r;
  target_replay_a(V, ds, max_steps, p0, v0, tg, taps, r);
  const FwdState& f = r.f;
  const unsigned done = r.done, e = r.e;
  unsigned j = r.j;
  float xj[3] = {f.xtx, f.xty, f.xtz}, vj[3] = {f.vtx, f.vty, f.vtz};
  float best = f.aux3;
  TargetGrad g;
  g.failed = !f.esc; g.fwd = done; g.steps = done;
  if (done < total) {                                                     // phase B, as target_ray_b
    float x = f.x, y = f.y, z = f.z;
    bool upd = false;
    for (unsigned k = done; k < total; ++k) {
      x = fmaf(ds, f.vx, x); y = fmaf(ds, f.vy, y); z = fmaf(ds, f.vz, z);
      const float bx = x - tg[0], by = y - tg[1], bz = z - tg[2];
      const float cur = dot3(bx, by, bz, bx, by, bz);
      if (cur < best) { best = cur; xj[0] = x; xj[1] = y; xj[2] = z; j = k + 1u; upd = true; }
    }
    if (upd) { vj[0] = f.vx; vj[1] = f.vy; vj[2] = f.vz; }
    g.steps += total - done;
  }
  if (rec) {
    for (int k = 0; k < 3; ++k) { rec->xt[k] = xj[k]; rec->vt[k] = vj[k]; }
    rec->dist2 = best; rec->j = j;
  }
  const float w = dd2 + dd2;
  const float gx[3] = {fmaf(w, xj[0] - tg[0], dx[0]), fmaf(w, xj[1] - tg[1], dx[1]), fmaf(w, xj[2] - tg[2], dx[2])};
  g.dp[0] = gx[0]; g.dp[1] = gx[1]; g.dp[2] = gx[2]; g.dv[0] = dv[0]; g.dv[1] = dv[1]; g.dv[2] = dv[2];
  if (j == 0) return g;
  RevMarch m;
  rev_seed(m, ds, xj, vj, gx, dv);
  unsigned hi = j;
  if (j > done) {                                    // the record was written after the escape: free flight back to phase A's end
    rev_flight(m, j - done, ds);
    m.s.x = f.x; m.s.y = f.y; m.s.z = f.z; m.s.vx = f.vx; m.s.vy = f.vy; m.s.vz = f.vz;
    hi = done;
  }
  if (hi > e) {                                      // the sampled run e .. hi-1
    rev_sampled(V, ds, 1.f, m, hi, e, r.ex, r.ey, r.ez, taps, NoSink{}, NoTerm{});
    g.steps += hi - e;
    hi = e;
  }
  if (hi > 0) rev_flight(m, hi, ds);                 // the free-flight prefix from p0
  rev_store(m, g.dp, g.dv);
  return g;
}

#if defined(__HIPCC__)
// fp32 atomic add without return: one global_atomic_add_f32 on gfx950 (no CAS loop).
__device__ __forceinline__ void atomic_add_f32(float* p, float v) { unsafeAtomicAdd(p, v); }
// The same at element idx of a grid whose base pointer is wave-uniform: ONE 32-bit byte offset per lane against the scalar
// base (global_atomic_add_f32 ... saddr), no 64-bit address arithmetic.  make_vol keeps byte offsets below 2^31.
__device__ __forceinline__ void atomic_add_f32_at(float* base, unsigned idx, float v) {
  unsafeAtomicAdd((float*)((char*)base + (idx << 2)), v);
}

// ---- wave reductions (64 lanes) -------------------------------------------------------------
__device__ __forceinline__ unsigned wave_sum_u32(unsigned v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
  return v;
}
__device__ __forceinline__ unsigned wave_max_u32(unsigned v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, (unsigned)__shfl_xor(v, o, kWave));
  return v;
}
#endif

}  // namespace drrt
