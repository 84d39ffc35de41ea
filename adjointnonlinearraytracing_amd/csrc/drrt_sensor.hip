// drrt_sensor.hip -- sensor image splat and its backward ("next" row 1):
// the step that follows the march in the reference's image experiments.
//
// Reference semantics (all torch, /root/reference/core):
//   sensor.py:195-202  trace_rays_to_plane   t = n.(p - x) / n.v ;  x' = x + t v
//   sensor.py:5-28     generate_sensor       2-D coords of x' in the sensor frame (t1 = n x t2, t2),
//                                            foreshortening fs = |v.n|, Grid.Splat(xn, fs*e, average=False)
//   sensor.py:31-53    generate_inf_sensor   far-field ("infinite distance") sensor: 2-D coords of the NORMALISED
//                                            direction in the sensor frame + ang_cut, ang_cut = sin(angle_span/2),
//                                            cell size 2*ang_cut/res, weight e (no foreshortening), same Splat
//   grid.py:37-64      Grid.index_values     u = xn/h - 0.5, 4x4 taps around floor(u), r = |u - idx|
//   grid.py:77-81      rbf_tent              w = max(sqrt(2) - r, 0)
//   grid.py:133-151    Grid.Splat            image[idx] += w/sum(w) * f  for taps inside the image
//                                            (normalised over ALL 16 taps, in or out)
// The reference builds ~20 (N,16)-sized temporaries per call and scatters with
// index_put_(accumulate=True); its backward is torch.autograd through all of that.  Here both
// directions are one fused kernel each: ray -> plane -> frame -> 16 taps -> fp32 atomics, and the
// analytic backward (gather 16 taps of dL/dimage, chain through the tent weights, the frame and the
// plane intersection) producing (grad_x, grad_v) directly -- the seed of Tracer::backtrace.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "drrt_host.h"

namespace drrt {

struct SensorArgs {
  const float* x; const float* v; const float* e;   // e nullable -> e_scalar
  float e_scalar;
  float p[3], n[3], t1[3], t2[3];
  const float* frame_dev;      // nullable: 12 device floats (p, n, t1, t2) read by the kernel INSTEAD of the four above --
                               // the *_dframe entries: a caller whose plane lives on the device needs no host copy / sync
  int res; float span, inv_hs, half_span;
  int far;                     // 1: generate_inf_sensor (coordinates from the direction only; span = 2*ang_cut);
                               // 2: get_sdf_vals_far (coordinates from the UN-normalised direction, sensor.py:134)
  float* image;                // forward out (res*res)
  const float* grad_image;     // backward in (tex_get: the texture being sampled)
  const float* grad_f;         // tex_get backward in: dL/df per ray
  float* f_out;                // tex_get forward out: one value per ray
  float* grad_x; float* grad_v;
  size_t n_rays;
  const float* rad;            // radiance splats: (n, channels) per-ray values (`e` stays null, so SensorRay::F is |v.n| or 1)
  int channels;                // ... image and grad_image are then (channels, res, res)
  float* grad_rad;             // radiance backward out (n, channels); like grad_x / grad_v there, written only when non-null
};

__device__ __forceinline__ void sensor_frame(SensorArgs& a) {       // wave-uniform scalar loads
  if (a.frame_dev != nullptr) {
#pragma unroll
    for (int k = 0; k < 3; ++k) { a.p[k] = a.frame_dev[k]; a.n[k] = a.frame_dev[3 + k]; a.t1[k] = a.frame_dev[6 + k]; a.t2[k] = a.frame_dev[9 + k]; }
  }
}

struct SensorRay {
  float den, t, F, u[2];
  int i1[2];
  bool ok;
};

__device__ __forceinline__ SensorRay sensor_locate(const SensorArgs& a, size_t i, float x[3], float v[3]) {
  SensorRay r;
  x[0] = a.x[3 * i]; x[1] = a.x[3 * i + 1]; x[2] = a.x[3 * i + 2];
  v[0] = a.v[3 * i]; v[1] = a.v[3 * i + 1]; v[2] = a.v[3 * i + 2];
  if (a.far) {                                                          // sensor.py:36-47
    const float nv = a.far == 2 ? 1.f : sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    const float inv = 1.f / nv;
    const float h0 = v[0] * inv, h1 = v[1] * inv, h2 = v[2] * inv;      // v / norm(v)
    const float xa = h0 * a.t1[0] + h1 * a.t1[1] + h2 * a.t1[2] + a.half_span;   // + ang_cut
    const float xb = h0 * a.t2[0] + h1 * a.t2[1] + h2 * a.t2[2] + a.half_span;
    r.den = nv; r.t = 0.f;
    r.u[0] = xa * a.inv_hs - 0.5f; r.u[1] = xb * a.inv_hs - 0.5f;
    const float f0 = floorf(r.u[0]), f1 = floorf(r.u[1]);
    r.ok = (f0 >= -3.f) & (f0 <= (float)(a.res + 1)) & (f1 >= -3.f) & (f1 <= (float)(a.res + 1));
    r.i1[0] = r.ok ? (int)f0 : 0; r.i1[1] = r.ok ? (int)f1 : 0;
    r.F = a.e ? a.e[i] : a.e_scalar;                                    // :49 (no foreshortening)
    return r;
  }
  r.den = v[0] * a.n[0] + v[1] * a.n[1] + v[2] * a.n[2];
  const float num = (a.p[0] - x[0]) * a.n[0] + (a.p[1] - x[1]) * a.n[1] + (a.p[2] - x[2]) * a.n[2];
  r.t = num / r.den;                                                  // sensor.py:199-200
  const float q0 = x[0] + r.t * v[0] - a.p[0], q1 = x[1] + r.t * v[1] - a.p[1], q2 = x[2] + r.t * v[2] - a.p[2];
  const float xa = q0 * a.t1[0] + q1 * a.t1[1] + q2 * a.t1[2] + a.half_span;    // sensor.py:22-23
  const float xb = q0 * a.t2[0] + q1 * a.t2[1] + q2 * a.t2[2] + a.half_span;
  r.u[0] = xa * a.inv_hs - 0.5f; r.u[1] = xb * a.inv_hs - 0.5f;       // grid.py:38
  const float f0 = floorf(r.u[0]), f1 = floorf(r.u[1]);
  // rays that miss the image by more than the tap footprint (or are NaN) contribute nothing
  r.ok = (f0 >= -3.f) & (f0 <= (float)(a.res + 1)) & (f1 >= -3.f) & (f1 <= (float)(a.res + 1));
  r.i1[0] = r.ok ? (int)f0 : 0; r.i1[1] = r.ok ? (int)f1 : 0;
  r.F = fabsf(r.den) * (a.e ? a.e[i] : a.e_scalar);                   // sensor.py:18-19
  return r;
}

// Forward splat.  Caustic / focused images put most rays on a few pixels, and same-address global
// atomics are serialised at the memory side (measured: 5.4 ms for 1M Luneburg-focused rays onto 512^2,
// 0.5 ms for spread-out rays).  Rays of a block are neighbours in the source and therefore land close
// together, so each block accumulates into an LDS tile of the image (doubles, ds_add_f64) anchored at
// the block's smallest hit pixel and flushes it with one global atomic per touched pixel; taps
// outside the tile go to global memory directly.
constexpr int kTile = 48;                       // tile edge in pixels (48*48 doubles = 18 KiB)
constexpr int kVoteCell = 32, kVote = 40;       // anchor vote: 40x40 coarse cells of 32 pixels (images up to 1277^2; larger ones clamp)

// The tile anchor of a block, shared by the two forward splats.  If all the block's hits fit one tile, anchor at the
// smallest hit pixel.  Otherwise (a focused bundle plus stray rays: the min corner would leave the FOCUS outside the
// tile, on the slow same-address global atomics) the rays vote on a coarse kVoteCell-pixel grid and the tile is centred
// on the winning cell.
struct TileAnchor {
  unsigned vote[kVote * kVote];
  int min[2];
  unsigned best;
};

__device__ __forceinline__ void anchor_reset(TileAnchor& s) {           // the caller's __syncthreads() follows
  for (int k = threadIdx.x; k < kVote * kVote; k += 256) s.vote[k] = 0u;
  if (threadIdx.x < 2) s.min[threadIdx.x] = 0x7fffffff;
  if (threadIdx.x == 0) s.best = 0u;
}

__device__ __forceinline__ void anchor_vote(TileAnchor& s, const SensorRay& r, int& oa, int& ob) {   // -> tile origin (block-uniform)
  int ca = 0, cb = 0;
  if (r.ok) {
    atomicMin(&s.min[0], r.i1[0] - 1); atomicMin(&s.min[1], r.i1[1] - 1);
    ca = min(max((r.i1[0] + 3) / kVoteCell, 0), kVote - 1); cb = min(max((r.i1[1] + 3) / kVoteCell, 0), kVote - 1);
    atomicAdd(&s.vote[ca * kVote + cb], 1u);
  }
  __syncthreads();
  {
    // argmax over the votes: pack (count, cell) so that atomicMax picks the fullest cell
    unsigned best = 0u;
    for (int k = threadIdx.x; k < kVote * kVote; k += 256) best = max(best, (s.vote[k] << 12) | (unsigned)k);
    if (best >> 12) atomicMax(&s.best, best);
  }
  __syncthreads();
  oa = s.min[0]; ob = s.min[1];
  {
    const int wa = (int)((s.best & 0xfffu) / kVote), wb = (int)((s.best & 0xfffu) % kVote);
    const int va = wa * kVoteCell - 3 - (kTile - kVoteCell) / 2, vb = wb * kVoteCell - 3 - (kTile - kVoteCell) / 2;
    // keep the min-corner anchor when it already covers the winning cell entirely
    if (va + (kTile - kVoteCell) / 2 + kVoteCell + 3 > oa + kTile || vb + (kTile - kVoteCell) / 2 + kVoteCell + 3 > ob + kTile) {
      oa = va; ob = vb;
    }
  }
}

__device__ __forceinline__ SensorRay no_ray() {                          // a thread past the last ray
  SensorRay r;
  r.ok = false; r.i1[0] = r.i1[1] = 0; r.u[0] = r.u[1] = 0.f; r.F = 0.f; r.den = 1.f; r.t = 0.f;
  return r;
}

__global__ void __launch_bounds__(256) k_sensor_splat(SensorArgs a) {
  sensor_frame(a);
  __shared__ double s_tile[kTile * kTile];
  __shared__ TileAnchor s_anchor;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  for (int k = threadIdx.x; k < kTile * kTile; k += 256) s_tile[k] = 0.0;
  anchor_reset(s_anchor);
  __syncthreads();
  float x[3], v[3];
  SensorRay r = no_ray();
  if (i < a.n_rays) r = sensor_locate(a, i, x, v);
  int oa, ob;
  anchor_vote(s_anchor, r, oa, ob);
  if (r.ok) {
    float w[16], wsum = 0.f;
#pragma unroll
    for (int ja = 0; ja < 4; ++ja) {
      const float da = r.u[0] - (float)(r.i1[0] - 1 + ja);
#pragma unroll
      for (int jb = 0; jb < 4; ++jb) {
        const float db = r.u[1] - (float)(r.i1[1] - 1 + jb);
        const float ww = fmaxf(1.41421356237f - sqrtf(da * da + db * db), 0.f);   // grid.py:79
        w[ja * 4 + jb] = ww; wsum += ww;
      }
    }
    const float scale = r.F / wsum;                                     // grid.py:145 (all 16 taps)
    const int la = r.i1[0] - 1 - oa, lb = r.i1[1] - 1 - ob;             // tile coords of the first tap
    const bool in_tile = (la >= 0) & (lb >= 0) & (la + 3 < kTile) & (lb + 3 < kTile);
#pragma unroll
    for (int ja = 0; ja < 4; ++ja) {
      const int ia = r.i1[0] - 1 + ja;
#pragma unroll
      for (int jb = 0; jb < 4; ++jb) {
        const int ib = r.i1[1] - 1 + jb;
        const float c = w[ja * 4 + jb] * scale;
        if (((unsigned)ia < (unsigned)a.res) & ((unsigned)ib < (unsigned)a.res) & (c != 0.f)) {   // grid.py:140
          if (in_tile) atomicAdd(&s_tile[(la + ja) * kTile + (lb + jb)], (double)c);
          else unsafeAtomicAdd(a.image + (size_t)ia * a.res + ib, c);
        }
      }
    }
  }
  __syncthreads();
  for (int k = threadIdx.x; k < kTile * kTile; k += 256) {
    const double g = s_tile[k];
    if (g != 0.0) {
      const int ia = oa + k / kTile, ib = ob + k % kTile;     // only in-image taps were accumulated
      unsafeAtomicAdd(a.image + (size_t)ia * a.res + ib, (float)g);
    }
  }
}

__global__ void __launch_bounds__(256) k_sensor_splat_bwd(SensorArgs a) {
  sensor_frame(a);
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n_rays) return;
  float x[3], v[3];
  const SensorRay r = sensor_locate(a, i, x, v);
  float gx[3] = {0.f, 0.f, 0.f}, gv[3] = {0.f, 0.f, 0.f};
  if (r.ok) {
    float W = 0.f, gw = 0.f, gda = 0.f, gdb = 0.f, sda = 0.f, sdb = 0.f;
#pragma unroll
    for (int ja = 0; ja < 4; ++ja) {
      const int ia = r.i1[0] - 1 + ja;
      const float da = r.u[0] - (float)ia;
#pragma unroll
      for (int jb = 0; jb < 4; ++jb) {
        const int ib = r.i1[1] - 1 + jb;
        const float db = r.u[1] - (float)ib;
        const float rr = sqrtf(da * da + db * db);
        const float ww = fmaxf(1.41421356237f - rr, 0.f);
        const bool valid = ((unsigned)ia < (unsigned)a.res) & ((unsigned)ib < (unsigned)a.res);
        const float g = valid ? a.grad_image[(size_t)ia * a.res + ib] : 0.f;
        const bool live = (ww > 0.f) & (rr > 0.f);
        const float inv_r = live ? 1.f / rr : 0.f;
        const float dwa = -da * inv_r, dwb = -db * inv_r;             // d w / d u
        W += ww; gw += g * ww; gda += g * dwa; gdb += g * dwb; sda += dwa; sdb += dwb;
      }
    }
    const float G = gw / W;
    const float k = r.F / W * a.inv_hs;
    const float ga = k * (gda - G * sda), gb = k * (gdb - G * sdb);    // dL/d xn
    const float gp0 = ga * a.t1[0] + gb * a.t2[0], gp1 = ga * a.t1[1] + gb * a.t2[1], gp2 = ga * a.t1[2] + gb * a.t2[2];
    if (a.far) {
      // coordinates depend on v only, through vhat = v/|v|:  d vhat / d v = (I - vhat vhat^T) / |v|
      const float inv = 1.f / r.den;
      const float h0 = v[0] * inv, h1 = v[1] * inv, h2 = v[2] * inv;
      const float hg = h0 * gp0 + h1 * gp1 + h2 * gp2;
      gv[0] = (gp0 - h0 * hg) * inv; gv[1] = (gp1 - h1 * hg) * inv; gv[2] = (gp2 - h2 * hg) * inv;
      a.grad_x[3 * i] = 0.f; a.grad_x[3 * i + 1] = 0.f; a.grad_x[3 * i + 2] = 0.f;
      a.grad_v[3 * i] = gv[0]; a.grad_v[3 * i + 1] = gv[1]; a.grad_v[3 * i + 2] = gv[2];
      return;
    }
    const float vg = (v[0] * gp0 + v[1] * gp1 + v[2] * gp2) / r.den;
    gx[0] = gp0 - a.n[0] * vg; gx[1] = gp1 - a.n[1] * vg; gx[2] = gp2 - a.n[2] * vg;     // (I - v n^T/den)^T
    const float ef = G * (a.e ? a.e[i] : a.e_scalar) * (r.den > 0.f ? 1.f : (r.den < 0.f ? -1.f : 0.f));
    gv[0] = r.t * gx[0] + ef * a.n[0]; gv[1] = r.t * gx[1] + ef * a.n[1]; gv[2] = r.t * gx[2] + ef * a.n[2];
  }
  a.grad_x[3 * i] = gx[0]; a.grad_x[3 * i + 1] = gx[1]; a.grad_x[3 * i + 2] = gx[2];
  a.grad_v[3 * i] = gv[0]; a.grad_v[3 * i + 1] = gv[1]; a.grad_v[3 * i + 2] = gv[2];
}

// ---- radiance splats: a per-ray, per-channel energy rad (n, C) onto an image (C, res, res), differentiable w.r.t. the
// rays AND rad.  Channel c is generate_sensor / generate_inf_sensor with e = rad[:, c]; all channels of a ray share its
// landing point, its 16 weights and its block's tile anchor, which are formed once.
constexpr int kMaxChannels = 32;

// Forward.  k_sensor_splat with a loop over the channels around its accumulate / flush: the ONE LDS tile is reused by every
// channel (the flush hands it back zeroed), so the LDS footprint does not grow with C, and the focused-bundle reasoning
// above holds for each channel as it stands -- a channel's taps meet the same pixels as any other's.
__global__ void __launch_bounds__(256) k_sensor_radiance(SensorArgs a) {
  sensor_frame(a);
  __shared__ double s_tile[kTile * kTile];
  __shared__ TileAnchor s_anchor;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  for (int k = threadIdx.x; k < kTile * kTile; k += 256) s_tile[k] = 0.0;
  anchor_reset(s_anchor);
  __syncthreads();
  float x[3], v[3];
  SensorRay r = no_ray();
  if (i < a.n_rays) r = sensor_locate(a, i, x, v);
  int oa, ob;
  anchor_vote(s_anchor, r, oa, ob);
  float w[16], wsum = 0.f;
#pragma unroll
  for (int ja = 0; ja < 4; ++ja) {
    const float da = r.u[0] - (float)(r.i1[0] - 1 + ja);
#pragma unroll
    for (int jb = 0; jb < 4; ++jb) {
      const float db = r.u[1] - (float)(r.i1[1] - 1 + jb);
      const float ww = fmaxf(1.41421356237f - sqrtf(da * da + db * db), 0.f);     // grid.py:79
      w[ja * 4 + jb] = ww; wsum += ww;
    }
  }
  const int la = r.i1[0] - 1 - oa, lb = r.i1[1] - 1 - ob;               // tile coords of the first tap
  const bool in_tile = (la >= 0) & (lb >= 0) & (la + 3 < kTile) & (lb + 3 < kTile);
  const size_t plane = (size_t)a.res * a.res;
  for (int ch = 0; ch < a.channels; ++ch) {
    float* const image = a.image + ch * plane;
    if (r.ok) {
      const float scale = r.F * a.rad[i * a.channels + ch] / wsum;      // grid.py:145 (all 16 taps)
#pragma unroll
      for (int ja = 0; ja < 4; ++ja) {
        const int ia = r.i1[0] - 1 + ja;
#pragma unroll
        for (int jb = 0; jb < 4; ++jb) {
          const int ib = r.i1[1] - 1 + jb;
          const float c = w[ja * 4 + jb] * scale;
          if (((unsigned)ia < (unsigned)a.res) & ((unsigned)ib < (unsigned)a.res) & (c != 0.f)) {   // grid.py:140
            if (in_tile) atomicAdd(&s_tile[(la + ja) * kTile + (lb + jb)], (double)c);
            else unsafeAtomicAdd(image + (size_t)ia * a.res + ib, c);
          }
        }
      }
    }
    __syncthreads();
    for (int k = threadIdx.x; k < kTile * kTile; k += 256) {
      const double g = s_tile[k];
      if (g != 0.0) {
        const int ia = oa + k / kTile, ib = ob + k % kTile;     // only in-image taps were accumulated
        unsafeAtomicAdd(image + (size_t)ia * a.res + ib, (float)g);
        s_tile[k] = 0.0;                                        // ... and the next channel finds the tile empty
      }
    }
    __syncthreads();
  }
}

// Backward: a deterministic gather, no atomics.  With gI the (C, res, res) seed and sums over the 16 taps j of the ray,
//   W = sum_j w_j,   G_c = sum_{j in image} gI[c, tap_j] w_j / W,
//   dL/drad_c = |v.n| G_c  (far field: G_c),
//   dL/du_a   = (1 / W) sum_c F_c (sum_{j in image} gI[c, tap_j] dw_j/du_a - G_c sum_j dw_j/du_a),   F_c = |v.n| rad_c,
// then k_sensor_splat_bwd's chain through inv_hs, the frame and the plane; the foreshortening term of dL/dv is
// (sum_c G_c rad_c) sign(v.n) n.  Register strategy: the 16 weights and their 32 derivatives are HELD and each channel
// re-gathers its 16 seed values against them in a rolled loop -- the register count does not depend on C (per-channel
// accumulators would take 3 C of them).  G_c is summed in the tap order ja, jb whatever C is and whichever outputs are
// asked for, so dL/drad[:, c] of a C-channel call is the 1-channel call's bit for bit.  Each of grad_rad, grad_x, grad_v
// is written only when non-null; with neither ray output asked for the derivative weights stay zero (no divides).
__global__ void __launch_bounds__(256) k_sensor_radiance_bwd(SensorArgs a) {
  sensor_frame(a);
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n_rays) return;
  float x[3], v[3];
  const SensorRay r = sensor_locate(a, i, x, v);
  const int C = a.channels;
  const bool rays = (a.grad_x != nullptr) | (a.grad_v != nullptr);
  float gx[3] = {0.f, 0.f, 0.f}, gv[3] = {0.f, 0.f, 0.f};
  if (r.ok) {
    float w[16], dwa[16], dwb[16], W = 0.f, sda = 0.f, sdb = 0.f;
#pragma unroll
    for (int ja = 0; ja < 4; ++ja) {
      const float da = r.u[0] - (float)(r.i1[0] - 1 + ja);
#pragma unroll
      for (int jb = 0; jb < 4; ++jb) {
        const float db = r.u[1] - (float)(r.i1[1] - 1 + jb);
        const float rr = sqrtf(da * da + db * db);
        const float ww = fmaxf(1.41421356237f - rr, 0.f);
        const bool live = (ww > 0.f) & (rr > 0.f) & rays;
        const float inv_r = live ? 1.f / rr : 0.f;
        w[ja * 4 + jb] = ww; dwa[ja * 4 + jb] = -da * inv_r; dwb[ja * 4 + jb] = -db * inv_r;       // d w / d u
        W += ww; sda += dwa[ja * 4 + jb]; sdb += dwb[ja * 4 + jb];
      }
    }
    const size_t plane = (size_t)a.res * a.res;
    float ga = 0.f, gb = 0.f, ef = 0.f;
    for (int ch = 0; ch < C; ++ch) {
      const float* const seed = a.grad_image + ch * plane;
      float gw = 0.f, gda = 0.f, gdb = 0.f;
#pragma unroll
      for (int ja = 0; ja < 4; ++ja) {
        const int ia = r.i1[0] - 1 + ja;
#pragma unroll
        for (int jb = 0; jb < 4; ++jb) {
          const int ib = r.i1[1] - 1 + jb;
          const bool valid = ((unsigned)ia < (unsigned)a.res) & ((unsigned)ib < (unsigned)a.res);
          const float g = valid ? seed[(size_t)ia * a.res + ib] : 0.f;
          gw += g * w[ja * 4 + jb]; gda += g * dwa[ja * 4 + jb]; gdb += g * dwb[ja * 4 + jb];
        }
      }
      const float G = gw / W;
      if (a.grad_rad) a.grad_rad[i * C + ch] = r.F * G;
      if (rays) {
        const float rc = a.rad[i * C + ch];
        ga += rc * (gda - G * sda); gb += rc * (gdb - G * sdb); ef += G * rc;
      }
    }
    const float k = r.F / W * a.inv_hs;
    ga *= k; gb *= k;                                                   // dL/d xn
    const float gp0 = ga * a.t1[0] + gb * a.t2[0], gp1 = ga * a.t1[1] + gb * a.t2[1], gp2 = ga * a.t1[2] + gb * a.t2[2];
    if (a.far) {                                                        // d vhat / d v = (I - vhat vhat^T) / |v|
      const float inv = 1.f / r.den;
      const float h0 = v[0] * inv, h1 = v[1] * inv, h2 = v[2] * inv;
      const float hg = h0 * gp0 + h1 * gp1 + h2 * gp2;
      gv[0] = (gp0 - h0 * hg) * inv; gv[1] = (gp1 - h1 * hg) * inv; gv[2] = (gp2 - h2 * hg) * inv;
    } else {
      const float vg = (v[0] * gp0 + v[1] * gp1 + v[2] * gp2) / r.den;
      gx[0] = gp0 - a.n[0] * vg; gx[1] = gp1 - a.n[1] * vg; gx[2] = gp2 - a.n[2] * vg;   // (I - v n^T/den)^T
      ef *= r.den > 0.f ? 1.f : (r.den < 0.f ? -1.f : 0.f);
      gv[0] = r.t * gx[0] + ef * a.n[0]; gv[1] = r.t * gx[1] + ef * a.n[1]; gv[2] = r.t * gx[2] + ef * a.n[2];
    }
  } else if (a.grad_rad) {
    for (int ch = 0; ch < C; ++ch) a.grad_rad[i * C + ch] = 0.f;        // a ray that misses: exactly 0
  }
  if (a.grad_x) { a.grad_x[3 * i] = gx[0]; a.grad_x[3 * i + 1] = gx[1]; a.grad_x[3 * i + 2] = gx[2]; }
  if (a.grad_v) { a.grad_v[3 * i] = gv[0]; a.grad_v[3 * i + 1] = gv[1]; a.grad_v[3 * i + 2] = gv[2]; }
}

// ---- texture lookups at the sensor: core/sensor.py:102-138 get_sdf_vals_near / get_sdf_vals_far ---------------------
// Grid(d_tex, h).Get(xn) (core/grid.py:100-124) at the rays' sensor coordinates: the same 4x4 radial tent taps as the
// splat, used as an interpolant f = sum_i w_i f_i / sum_i w_i with tap indices CLIPPED to the texture (grid.py:57),
// not masked (a point off the texture is extrapolated from the edge texels).  The backward is the interpolant's analytic derivative (what Get returns as its second value),
// chained through the sensor frame and the plane intersection to (dL/dx, dL/dv).
struct TexTaps { float W, fw, fda, fdb, sda, sdb; };
// The taps follow the point (their texels are clipped, not the taps), so a point anywhere off the texture still has its
// 16 taps around it -- unlike the splat, which drops rays that miss the image: re-derive the tap origin without that test.
// Once floor(u) is below -4 or above res + 2 every tap clips to the edge texel, and the interpolant depends on frac(u)
// only; the point is folded back to that many texels off the edge, keeping frac(u): u - floor(u) is exact and so is
// adding the (smaller) integer back, so value and derivative are unchanged -- and a point 2^20 or more texels away no
// longer gets 16 zero weights (0/0).  An infinite u folds to inf - inf = NaN, a NaN u stays: both give NaN.
__device__ __forceinline__ void tex_origin(const SensorArgs& a, SensorRay& r) {
  const float lo = -4.f, hi = (float)(a.res + 2);
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const float fl = floorf(r.u[k]);
    if (fl < lo) r.u[k] = (r.u[k] - fl) + lo;
    else if (fl > hi) r.u[k] = (r.u[k] - fl) + hi;
    r.i1[k] = (int)fminf(fmaxf(floorf(r.u[k]), lo), hi);                 // NaN -> a bound; the weights are NaN/0 then
  }
  r.ok = true;
}
__device__ __forceinline__ TexTaps tex_taps(const SensorArgs& a, const SensorRay& r) {
  TexTaps t{0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ja = 0; ja < 4; ++ja) {
    const int ia = r.i1[0] - 1 + ja;
    const float da = r.u[0] - (float)ia;
    const int ca = min(max(ia, 0), a.res - 1);
#pragma unroll
    for (int jb = 0; jb < 4; ++jb) {
      const int ib = r.i1[1] - 1 + jb;
      const float db = r.u[1] - (float)ib;
      const int cb = min(max(ib, 0), a.res - 1);
      const float rr = sqrtf(da * da + db * db);
      const float ww = fmaxf(1.41421356237f - rr, 0.f);
      const float f = a.grad_image[(size_t)ca * a.res + cb];
      const bool live = (ww > 0.f) & (rr > 0.f);
      const float inv_r = live ? 1.f / rr : 0.f;
      const float dwa = -da * inv_r, dwb = -db * inv_r;               // d w / d u
      t.W += ww; t.fw += f * ww; t.fda += f * dwa; t.fdb += f * dwb; t.sda += dwa; t.sdb += dwb;
    }
  }
  return t;
}

__global__ void __launch_bounds__(256) k_sensor_tex_get(SensorArgs a) {
  sensor_frame(a);
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n_rays) return;
  float x[3], v[3];
  SensorRay r = sensor_locate(a, i, x, v);
  tex_origin(a, r);
  const TexTaps t = tex_taps(a, r);
  a.f_out[i] = t.fw / t.W;                                            // NaN coordinates: all weights 0 -> 0/0 = NaN
}

__global__ void __launch_bounds__(256) k_sensor_tex_get_bwd(SensorArgs a) {
  sensor_frame(a);
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n_rays) return;
  float x[3], v[3];
  SensorRay r = sensor_locate(a, i, x, v);
  tex_origin(a, r);
  float gx[3] = {0.f, 0.f, 0.f}, gv[3] = {0.f, 0.f, 0.f};
  {
    const TexTaps t = tex_taps(a, r);
    const float f = t.fw / t.W;
    const float k = a.grad_f[i] / t.W * a.inv_hs;
    const float ga = k * (t.fda - f * t.sda), gb = k * (t.fdb - f * t.sdb);        // dL/d xn
    const float gp0 = ga * a.t1[0] + gb * a.t2[0], gp1 = ga * a.t1[1] + gb * a.t2[1], gp2 = ga * a.t1[2] + gb * a.t2[2];
    if (a.far) {                                    // far == 2: xn = v . T + ang_cut
      gv[0] = gp0; gv[1] = gp1; gv[2] = gp2;
    } else {
      const float vg = (v[0] * gp0 + v[1] * gp1 + v[2] * gp2) / r.den;
      gx[0] = gp0 - a.n[0] * vg; gx[1] = gp1 - a.n[1] * vg; gx[2] = gp2 - a.n[2] * vg;
      gv[0] = r.t * gx[0]; gv[1] = r.t * gx[1]; gv[2] = r.t * gx[2];
    }
  }
  a.grad_x[3 * i] = gx[0]; a.grad_x[3 * i + 1] = gx[1]; a.grad_x[3 * i + 2] = gx[2];
  a.grad_v[3 * i] = gv[0]; a.grad_v[3 * i + 1] = gv[1]; a.grad_v[3 * i + 2] = gv[2];
}

// ---- host half: every entry point is one filler (the rays, the frame and the image geometry of its coordinate family ->
// SensorArgs) followed by one runner (its kind of output -> the launch) --------------------------------------------------

// Where the sensor frame of a call is: 12 floats on the device (p, n, t1, t2) that the kernel reads itself -- the *_dframe
// entries --, or host vectors, of which the far field gives the last two only.
struct Frame {
  const float* dev;
  const float* host[4];     // p, n, t1, t2; the first 4 - n_host are absent
  int n_host;               // 0: the frame is `dev`
};
static Frame host_frame(const float* p, const float* n, const float* t1, const float* t2) { return {nullptr, {p, n, t1, t2}, 4}; }
static Frame host_frame(const float* t1, const float* t2) { return {nullptr, {nullptr, nullptr, t1, t2}, 2}; }
static Frame device_frame(const float* frame12) { return {frame12, {nullptr, nullptr, nullptr, nullptr}, 0}; }

// Near plane: generate_sensor (rays -> plane -> sensor frame, cell size span / res).
static int fill_near(SensorArgs& a, size_t n, const float* x, const float* v, const float* e, float e_scalar, const Frame& f,
                     int res, float span) {
  if (f.n_host == 0 && !f.dev) return fail(DRRT_ERR_ARG, "null frame pointer");
  bool null = !x || !v;
  for (int j = 4 - f.n_host; j < 4; ++j) null |= !f.host[j];
  if (null) return fail(DRRT_ERR_ARG, "null pointer");
  if (res < 1 || res > 32768 || !(span > 0.f)) return fail(DRRT_ERR_ARG, "bad sensor resolution / span");
  a.x = x; a.v = v; a.e = e; a.e_scalar = e_scalar; a.n_rays = n;
  float* const vec[4] = {a.p, a.n, a.t1, a.t2};       // (absent vectors stay zero)
  for (int j = 4 - f.n_host; j < 4; ++j)
    for (int k = 0; k < 3; ++k) vec[j][k] = f.host[j][k];
  a.frame_dev = f.dev;
  a.res = res; a.span = span; a.inv_hs = 1.0f / (span / (float)res); a.half_span = span / 2;
  a.far = 0;
  return DRRT_OK;
}

// Far field (core/sensor.py:31-53 generate_inf_sensor, called at core/image_opt.py:116): the splat kernels with
// SensorArgs::far set.  `ang_cut` = sin(0.5 * deg2rad(angle_span)) is computed by the caller (the reference evaluates it in
// the rays' dtype, sensor.py:38); the image spans [0, 2*ang_cut)^2.  Reads t1, t2 only; the directions stand in for x.
static int fill_far(SensorArgs& a, size_t n, const float* v, const float* e, float e_scalar, const Frame& f, int res,
                    float ang_cut) {
  if (int rc = fill_near(a, n, v, v, e, e_scalar, f, res, 2.0f * ang_cut)) return rc;
  a.half_span = ang_cut; a.inv_hs = 1.0f / (2.0f * ang_cut / (float)res);   // Grid(zeros, 2*ang_cut/res), :44
  a.far = 1;
  return DRRT_OK;
}

// Texture lookups (core/sensor.py:102-138), see k_sensor_tex_get.  mode 0: get_sdf_vals_near (rays -> plane -> sensor
// frame, cell size span / res); mode 1: get_sdf_vals_far (coordinates v . T + ang_cut from the direction as it is, cell
// size 2 ang_cut / res; pass span = 2 * ang_cut).
static int fill_tex(SensorArgs& a, size_t n, const float* x, const float* v, const Frame& f, const float* tex, int res,
                    float span, int mode) {
  if (int rc = fill_near(a, n, x, v, nullptr, 1.f, f, res, span)) return rc;
  if (!tex) return fail(DRRT_ERR_ARG, "null texture pointer");
  if (mode != 0 && mode != 1) return fail(DRRT_ERR_ARG, "mode must be 0 (near) or 1 (far)");
  a.far = mode == 1 ? 2 : 0;
  a.grad_image = tex;
  return DRRT_OK;
}

// Radiance splats: the near or the far family's coordinates with a per-ray, per-channel energy in place of `e` (which
// stays null with e_scalar 1, so that the kernels find F = |v.n| or 1 in SensorRay).  `span` is ang_cut for the far field.
static int fill_radiance(SensorArgs& a, bool far, size_t n, const float* x, const float* v, const float* rad, int channels,
                         const Frame& f, int res, float span) {
  if (int rc = far ? fill_far(a, n, v, nullptr, 1.f, f, res, span) : fill_near(a, n, x, v, nullptr, 1.f, f, res, span)) return rc;
  if (!rad) return fail(DRRT_ERR_ARG, "null pointer");
  if (channels < 1 || channels > kMaxChannels) return fail(DRRT_ERR_ARG, "channels must lie in 1..32");
  a.rad = rad; a.channels = channels;
  return DRRT_OK;
}

// The runners differ in when they look at their outputs, and callers rely on it: the splats check theirs before the
// n == 0 return (and the forward has zeroed the image by then), the lookups return DRRT_OK for n == 0 first.
static int run_image(SensorArgs& a, float* image, unsigned flags, void* stream) {
  if (!image) return fail(DRRT_ERR_ARG, "null image pointer");
  if (!(flags & DRRT_FLAG_NO_ZERO)) {
    const size_t planes = a.rad ? (size_t)a.channels : 1;             // a radiance image is (channels, res, res)
    const hipError_t e = hipMemsetAsync(image, 0, planes * a.res * a.res * sizeof(float), (hipStream_t)stream);
    if (e != hipSuccess) return fail(DRRT_ERR_HIP, hipGetErrorString(e));
  }
  if (a.n_rays == 0) return DRRT_OK;
  a.image = image;
  return launch_1d(a.rad ? k_sensor_radiance : k_sensor_splat, a.n_rays, stream, a);
}

// The radiance backward: every output is optional, and a call that asks for none has nothing to launch.
static int run_radiance_grads(SensorArgs& a, const float* grad_image, float* grad_rad, float* grad_x, float* grad_v,
                              void* stream) {
  if (!grad_image) return fail(DRRT_ERR_ARG, "null gradient pointer");
  if (a.n_rays == 0 || (!grad_rad && !grad_x && !grad_v)) return DRRT_OK;
  a.grad_image = grad_image; a.grad_rad = grad_rad; a.grad_x = grad_x; a.grad_v = grad_v;
  return launch_1d(k_sensor_radiance_bwd, a.n_rays, stream, a);
}

// `seed`: dL/dimage of a splat, dL/df of a lookup (whose texture fill_tex has put where the splat's dL/dimage goes)
static int run_ray_grads(bool lookup, SensorArgs& a, const float* seed, float* grad_x, float* grad_v, void* stream) {
  if (lookup && a.n_rays == 0) return DRRT_OK;
  if (!seed || !grad_x || !grad_v) return fail(DRRT_ERR_ARG, "null gradient pointer");
  if (a.n_rays == 0) return DRRT_OK;
  (lookup ? a.grad_f : a.grad_image) = seed; a.grad_x = grad_x; a.grad_v = grad_v;
  return launch_1d(lookup ? k_sensor_tex_get_bwd : k_sensor_splat_bwd, a.n_rays, stream, a);
}

static int run_values(SensorArgs& a, float* f_out, void* stream) {
  if (a.n_rays == 0) return DRRT_OK;
  if (!f_out) return fail(DRRT_ERR_ARG, "null output pointer");
  a.f_out = f_out;
  return launch_1d(k_sensor_tex_get, a.n_rays, stream, a);
}

}  // namespace drrt

using namespace drrt;

extern "C" int drrt_sensor_splat_f32(size_t n, const float* x, const float* v, const float* e, float e_scalar,
                                     const float plane_p[3], const float plane_n[3], const float t1[3],
                                     const float t2[3], int res, float span, float* image, unsigned flags,
                                     void* stream) {
  SensorArgs a{};
  const int rc = fill_near(a, n, x, v, e, e_scalar, host_frame(plane_p, plane_n, t1, t2), res, span);
  return rc ? rc : run_image(a, image, flags, stream);
}
extern "C" int drrt_sensor_splat_dframe_f32(size_t n, const float* x, const float* v, const float* e, float e_scalar,
                                            const float* frame12, int res, float span, float* image, unsigned flags,
                                            void* stream) {
  SensorArgs a{};
  const int rc = fill_near(a, n, x, v, e, e_scalar, device_frame(frame12), res, span);
  return rc ? rc : run_image(a, image, flags, stream);
}
extern "C" int drrt_sensor_splat_bwd_f32(size_t n, const float* x, const float* v, const float* e, float e_scalar,
                                         const float plane_p[3], const float plane_n[3], const float t1[3],
                                         const float t2[3], int res, float span, const float* grad_image,
                                         float* grad_x, float* grad_v, void* stream) {
  SensorArgs a{};
  const int rc = fill_near(a, n, x, v, e, e_scalar, host_frame(plane_p, plane_n, t1, t2), res, span);
  return rc ? rc : run_ray_grads(false, a, grad_image, grad_x, grad_v, stream);
}
extern "C" int drrt_sensor_splat_dframe_bwd_f32(size_t n, const float* x, const float* v, const float* e, float e_scalar,
                                                const float* frame12, int res, float span, const float* grad_image,
                                                float* grad_x, float* grad_v, void* stream) {
  SensorArgs a{};
  const int rc = fill_near(a, n, x, v, e, e_scalar, device_frame(frame12), res, span);
  return rc ? rc : run_ray_grads(false, a, grad_image, grad_x, grad_v, stream);
}

extern "C" int drrt_sensor_far_splat_f32(size_t n, const float* v, const float* e, float e_scalar, const float t1[3],
                                         const float t2[3], int res, float ang_cut, float* image, unsigned flags,
                                         void* stream) {
  SensorArgs a{};
  const int rc = fill_far(a, n, v, e, e_scalar, host_frame(t1, t2), res, ang_cut);
  return rc ? rc : run_image(a, image, flags, stream);
}
extern "C" int drrt_sensor_far_splat_dframe_f32(size_t n, const float* v, const float* e, float e_scalar,
                                                const float* frame12, int res, float ang_cut, float* image,
                                                unsigned flags, void* stream) {
  SensorArgs a{};
  const int rc = fill_far(a, n, v, e, e_scalar, device_frame(frame12), res, ang_cut);
  return rc ? rc : run_image(a, image, flags, stream);
}
extern "C" int drrt_sensor_far_splat_bwd_f32(size_t n, const float* v, const float* e, float e_scalar, const float t1[3],
                                             const float t2[3], int res, float ang_cut, const float* grad_image,
                                             float* grad_x, float* grad_v, void* stream) {
  SensorArgs a{};
  const int rc = fill_far(a, n, v, e, e_scalar, host_frame(t1, t2), res, ang_cut);
  return rc ? rc : run_ray_grads(false, a, grad_image, grad_x, grad_v, stream);
}
extern "C" int drrt_sensor_far_splat_dframe_bwd_f32(size_t n, const float* v, const float* e, float e_scalar,
                                                    const float* frame12, int res, float ang_cut,
                                                    const float* grad_image, float* grad_x, float* grad_v, void* stream) {
  SensorArgs a{};
  const int rc = fill_far(a, n, v, e, e_scalar, device_frame(frame12), res, ang_cut);
  return rc ? rc : run_ray_grads(false, a, grad_image, grad_x, grad_v, stream);
}

extern "C" int drrt_sensor_radiance_f32(size_t n, const float* x, const float* v, const float* rad, int channels,
                                        const float plane_p[3], const float plane_n[3], const float t1[3],
                                        const float t2[3], int res, float span, float* image, unsigned flags, void* stream) {
  SensorArgs a{};
  const int rc = fill_radiance(a, false, n, x, v, rad, channels, host_frame(plane_p, plane_n, t1, t2), res, span);
  return rc ? rc : run_image(a, image, flags, stream);
}
extern "C" int drrt_sensor_radiance_dframe_f32(size_t n, const float* x, const float* v, const float* rad, int channels,
                                               const float* frame12, int res, float span, float* image, unsigned flags,
                                               void* stream) {
  SensorArgs a{};
  const int rc = fill_radiance(a, false, n, x, v, rad, channels, device_frame(frame12), res, span);
  return rc ? rc : run_image(a, image, flags, stream);
}
extern "C" int drrt_sensor_radiance_bwd_f32(size_t n, const float* x, const float* v, const float* rad, int channels,
                                            const float plane_p[3], const float plane_n[3], const float t1[3],
                                            const float t2[3], int res, float span, const float* grad_image,
                                            float* grad_rad, float* grad_x, float* grad_v, void* stream) {
  SensorArgs a{};
  const int rc = fill_radiance(a, false, n, x, v, rad, channels, host_frame(plane_p, plane_n, t1, t2), res, span);
  return rc ? rc : run_radiance_grads(a, grad_image, grad_rad, grad_x, grad_v, stream);
}
extern "C" int drrt_sensor_radiance_dframe_bwd_f32(size_t n, const float* x, const float* v, const float* rad, int channels,
                                                   const float* frame12, int res, float span, const float* grad_image,
                                                   float* grad_rad, float* grad_x, float* grad_v, void* stream) {
  SensorArgs a{};
  const int rc = fill_radiance(a, false, n, x, v, rad, channels, device_frame(frame12), res, span);
  return rc ? rc : run_radiance_grads(a, grad_image, grad_rad, grad_x, grad_v, stream);
}

extern "C" int drrt_sensor_radiance_far_f32(size_t n, const float* v, const float* rad, int channels, const float t1[3],
                                            const float t2[3], int res, float ang_cut, float* image, unsigned flags,
                                            void* stream) {
  SensorArgs a{};
  const int rc = fill_radiance(a, true, n, v, v, rad, channels, host_frame(t1, t2), res, ang_cut);
  return rc ? rc : run_image(a, image, flags, stream);
}
extern "C" int drrt_sensor_radiance_far_dframe_f32(size_t n, const float* v, const float* rad, int channels,
                                                   const float* frame12, int res, float ang_cut, float* image,
                                                   unsigned flags, void* stream) {
  SensorArgs a{};
  const int rc = fill_radiance(a, true, n, v, v, rad, channels, device_frame(frame12), res, ang_cut);
  return rc ? rc : run_image(a, image, flags, stream);
}
extern "C" int drrt_sensor_radiance_far_bwd_f32(size_t n, const float* v, const float* rad, int channels, const float t1[3],
                                                const float t2[3], int res, float ang_cut, const float* grad_image,
                                                float* grad_rad, float* grad_x, float* grad_v, void* stream) {
  SensorArgs a{};
  const int rc = fill_radiance(a, true, n, v, v, rad, channels, host_frame(t1, t2), res, ang_cut);
  return rc ? rc : run_radiance_grads(a, grad_image, grad_rad, grad_x, grad_v, stream);
}
extern "C" int drrt_sensor_radiance_far_dframe_bwd_f32(size_t n, const float* v, const float* rad, int channels,
                                                       const float* frame12, int res, float ang_cut,
                                                       const float* grad_image, float* grad_rad, float* grad_x,
                                                       float* grad_v, void* stream) {
  SensorArgs a{};
  const int rc = fill_radiance(a, true, n, v, v, rad, channels, device_frame(frame12), res, ang_cut);
  return rc ? rc : run_radiance_grads(a, grad_image, grad_rad, grad_x, grad_v, stream);
}

extern "C" int drrt_sensor_tex_get_f32(size_t n, const float* x, const float* v, const float plane_p[3],
                                       const float plane_n[3], const float t1[3], const float t2[3], const float* tex,
                                       int res, float span, int mode, float* f_out, void* stream) {
  SensorArgs a{};
  const int rc = fill_tex(a, n, x, v, host_frame(plane_p, plane_n, t1, t2), tex, res, span, mode);
  return rc ? rc : run_values(a, f_out, stream);
}
extern "C" int drrt_sensor_tex_get_dframe_f32(size_t n, const float* x, const float* v, const float* frame12,
                                              const float* tex, int res, float span, int mode, float* f_out, void* stream) {
  SensorArgs a{};
  const int rc = fill_tex(a, n, x, v, device_frame(frame12), tex, res, span, mode);
  return rc ? rc : run_values(a, f_out, stream);
}
extern "C" int drrt_sensor_tex_get_bwd_f32(size_t n, const float* x, const float* v, const float plane_p[3],
                                           const float plane_n[3], const float t1[3], const float t2[3],
                                           const float* tex, int res, float span, int mode, const float* grad_f,
                                           float* grad_x, float* grad_v, void* stream) {
  SensorArgs a{};
  const int rc = fill_tex(a, n, x, v, host_frame(plane_p, plane_n, t1, t2), tex, res, span, mode);
  return rc ? rc : run_ray_grads(true, a, grad_f, grad_x, grad_v, stream);
}
extern "C" int drrt_sensor_tex_get_dframe_bwd_f32(size_t n, const float* x, const float* v, const float* frame12,
                                                  const float* tex, int res, float span, int mode, const float* grad_f,
                                                  float* grad_x, float* grad_v, void* stream) {
  SensorArgs a{};
  const int rc = fill_tex(a, n, x, v, device_frame(frame12), tex, res, span, mode);
  return rc ? rc : run_ray_grads(true, a, grad_f, grad_x, grad_v, stream);
}
