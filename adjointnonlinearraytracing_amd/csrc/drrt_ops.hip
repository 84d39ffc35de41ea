// drrt_ops.hip -- the small operators around the march that belong to no sensor and no source: multires up-sampling of a
// volume, the fused boundary-mask + Adam + clamp step, and the ray -> plane intersection.  Each is
// one kernel (two with its backward), one thread per element, and an entry point of include/drrt_hip.h.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "drrt_device.h"
#include "drrt_host.h"

using namespace drrt;

// =============================================================================================
// multires up-sampling of a volume (SURVEY.md 8.8 "next" row 3)
//
// Reference: core/optimizer.py:7-10 upres_scene -> core/grid.py:318-330 upres_volume: trilinear
// resampling of the (R,R,R) volume at linspace(0,1,S)^3 through Grid.GetLinear (:227-273), carried
// out in float64 and cast back.  The reference materialises an (S^3, 3) float64 point list plus ~20
// (S^3, 8)-sized temporaries (several GB at S = 256); this is one pass, one thread per output voxel.
// =============================================================================================
namespace drrt {

__global__ void __launch_bounds__(256) k_upres(const float* __restrict__ src, int r0, int r1, int r2,
                                               float* __restrict__ dst, int s0, int s1, int s2) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t total = (size_t)s0 * s1 * s2;
  if (i >= total) return;
  const int k = (int)(i % s2), j = (int)((i / s2) % s1), m = (int)(i / ((size_t)s2 * s1));
  const int idx[3] = {m, j, k}, sn[3] = {s0, s1, s2};
  const int rr = r0;                                   // the reference clips every axis with res[0] (grid.py:242)
  const double h = 1.0 / (double)(rr > 1 ? rr - 1 : 1);   // grid.py:319-320
  int i0[3], i1[3]; double w[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    // torch.linspace(0, 1, s): step*i for the first half, 1 - step*(s-1-i) for the second as ONE fused multiply-add
    // (torch's kernels contract it: one rounding); one step is the start alone.  The last bit matters: where a point
    // lands on a source node it decides floor(), and one ulp short of the node mixes 1e-16 of the neighbour in.
    const double step = sn[a] > 1 ? 1.0 / (double)(sn[a] - 1) : 0.0;
    const double x = (idx[a] < sn[a] / 2 || sn[a] == 1) ? step * idx[a] : fma(-step, (double)(sn[a] - 1 - idx[a]), 1.0);
    const double nx = x / h;                           // grid.py:232
    const double fl = floor(nx);
    double ww = nx - fl; ww = ww < 0.0 ? 0.0 : (ww > 1.0 ? 1.0 : ww);   // :235
    w[a] = ww;
    const int b = (int)fl;
    i0[a] = min(max(b, 0), rr - 1); i1[a] = min(max(b + 1, 0), rr - 1);  // :243
  }
  double acc = 0.0;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const int a0 = (c & 4) ? i1[0] : i0[0], a1 = (c & 2) ? i1[1] : i0[1], a2 = (c & 1) ? i1[2] : i0[2];
    const double ww = ((c & 4) ? w[0] : 1.0 - w[0]) * ((c & 2) ? w[1] : 1.0 - w[1]) * ((c & 1) ? w[2] : 1.0 - w[2]);
    acc += ww * (double)src[((size_t)a0 * r1 + a1) * r2 + a2];
  }
  dst[i] = (float)acc;
}

}  // namespace drrt

extern "C" int drrt_upres_volume_f32(const float* src, const int src_shape[3], float* dst, const int dst_shape[3],
                                     void* stream) {
  if (!src || !dst || !src_shape || !dst_shape) return fail(DRRT_ERR_ARG, "null pointer");
  for (int a = 0; a < 3; ++a)
    if (src_shape[a] < 1 || dst_shape[a] < 1) return fail(DRRT_ERR_ARG, "bad shape");
  if (src_shape[0] != src_shape[1] || src_shape[0] != src_shape[2])
    return fail(DRRT_ERR_ARG, "upres_volume expects a cubic source volume (the reference clips all axes with res[0])");
  const size_t total = (size_t)dst_shape[0] * dst_shape[1] * dst_shape[2];
  return launch_1d(k_upres, total, stream, src, src_shape[0], src_shape[1], src_shape[2], dst, dst_shape[0], dst_shape[1],
                   dst_shape[2]);
}

// =============================================================================================
// one optimiser iteration's tail (SURVEY.md 8.8 "next" row 3): boundary-gradient mask + Adam + clamp
//
// Reference: core/optimizer.py:57-69 -- `n.grad[mask] = 0` (mask = the outermost voxel layer, :54-55),
// `opto.step()` with torch.optim.Adam, `n.clamp_(min=1)`.  In torch that is a boolean-mask index_put (a nonzero()
// with a host sync), ~10 element-wise launches and three extra passes over the volume and its two moments; here it
// is ONE pass: 16 B read + 12 B written per voxel.  The update is torch's Adam (torch/optim/adam.py
// _single_tensor_adam, amsgrad = maximize = False), bias corrections computed by the caller in double:
//   g     = grad (0 on the boundary layer; written back there like the reference's in-place mask) + weight_decay * p
//   m     = w < 0.5 ? m + (g - m) * w : g - (g - m) * (1 - w)      (exp_avg.lerp_; w = 1 - beta1 rounded to fp32 and
//                                                                  1 - w its fp32 complement, as in ATen -- not beta1)
//   v     = beta2 * v + (1 - beta2) * g * g
//   p    -= step_size * m / (sqrt(v) / sqrt(bias_correction2) + eps),   step_size = lr / bias_correction1
//   p     = p < clamp_min ? clamp_min : p              (NaN stays NaN, like clamp_)
// =============================================================================================
namespace drrt {

struct AdamArgs {
  float* p; float* g; float* m; float* v;
  size_t n; int s0, s1, s2;             // torch shape (z, y, x): x fastest
  float step_size, bc2_sqrt, beta2, omb1, omb2, eps, weight_decay, clamp_min;   // omb = 1 - beta, rounded from double like torch's scalars
  int mask_boundary, clamp;
};

__global__ void __launch_bounds__(256) k_adam_masked(AdamArgs a) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n) return;
  float g = a.g[i];
  if (a.mask_boundary) {
    const int x = (int)(i % (size_t)a.s2), y = (int)((i / (size_t)a.s2) % (size_t)a.s1), z = (int)(i / ((size_t)a.s2 * a.s1));
    if ((x == 0) | (x == a.s2 - 1) | (y == 0) | (y == a.s1 - 1) | (z == 0) | (z == a.s0 - 1)) { g = 0.f; a.g[i] = 0.f; }
  }
  float p = a.p[i], m = a.m[i], v = a.v[i];
  if (a.weight_decay != 0.f) g = fmaf(a.weight_decay, p, g);
  // lerp_ weighs from the nearer end (ATen's lerp: |weight| < 0.5 from m, else from g), so beta1 = 0 gives m = g exactly
  const float d = g - m;
  m = (a.omb1 < 0.5f) ? fmaf(d, a.omb1, m) : fmaf(-d, 1.f - a.omb1, g);
  v = fmaf(a.omb2, g * g, a.beta2 * v);
  const float denom = sqrtf(v) / a.bc2_sqrt + a.eps;
  p = fmaf(-a.step_size, m / denom, p);
  if (a.clamp) p = (p < a.clamp_min) ? a.clamp_min : p;
  a.p[i] = p; a.m[i] = m; a.v[i] = v;
}

}  // namespace drrt

extern "C" int drrt_adam_step_f32(float* param, float* grad, float* exp_avg, float* exp_avg_sq, const int shape[3],
                                  double step, double lr, double beta1, double beta2, double eps, double weight_decay,
                                  double clamp_min, unsigned flags, void* stream) {
  if (!param || !grad || !exp_avg || !exp_avg_sq || !shape) return fail(DRRT_ERR_ARG, "null pointer");
  for (int k = 0; k < 3; ++k) if (shape[k] < 1) return fail(DRRT_ERR_ARG, "bad shape");
  if (!(step >= 1.0)) return fail(DRRT_ERR_ARG, "step must be >= 1 (the value AFTER the increment, like torch's)");
  AdamArgs a{};
  a.p = param; a.g = grad; a.m = exp_avg; a.v = exp_avg_sq;
  a.s0 = shape[0]; a.s1 = shape[1]; a.s2 = shape[2];
  a.n = (size_t)shape[0] * shape[1] * shape[2];
  const double bc1 = 1.0 - pow(beta1, step), bc2 = 1.0 - pow(beta2, step);       // torch/optim/adam.py
  a.step_size = (float)(lr / bc1); a.bc2_sqrt = (float)sqrt(bc2);
  a.beta2 = (float)beta2; a.omb1 = (float)(1.0 - beta1); a.omb2 = (float)(1.0 - beta2);
  a.eps = (float)eps; a.weight_decay = (float)weight_decay;
  a.clamp_min = (float)clamp_min;
  a.mask_boundary = (flags & DRRT_ADAM_MASK_BOUNDARY) ? 1 : 0;
  a.clamp = (flags & DRRT_ADAM_CLAMP_MIN) ? 1 : 0;
  return launch_1d(k_adam_masked, a.n, stream, a);
}

// =============================================================================================
// ray -> plane intersection as its own operator (the statement right after the march)
//
// Reference: core/sensor.py:195-202 trace_rays_to_plane: t = n.(p - x) / n.v ; x_out = x + t v ; v unchanged --
// written with torch.matmul on (N,1,3) x (N,3,1) operands, i.e. a batched matmul of N one-by-three products, which on
// the GPU costs ~25 ms forward and ~55 ms backward for 1M rays (tools/bench_iteration.py): 15x the march itself.
// Here: one thread per ray, forward and analytic backward (gradients w.r.t. the rays; the planes are constants in
// every experiment of the reference -- the Python wrapper falls back to the torch expressions if they require grad):
//   a = n.(p - x), b = n.v, t = a / b
//   d x_out / d x = I - v n^T / b            d x_out / d v = t I - (t / b) v n^T
//   => gx = g - (g.v / b) n                  gv = t g - (t / b)(g.v) n          (g = dL/dx_out)
// plane_stride = 3: one plane per ray; 0: one plane for all rays.
// =============================================================================================
namespace drrt {

__global__ void __launch_bounds__(256) k_rays_to_plane(size_t n, const float* __restrict__ x, const float* __restrict__ v,
                                                       const float* __restrict__ p, const float* __restrict__ nr,
                                                       int plane_stride, float* __restrict__ xo) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const size_t k = i * (size_t)plane_stride;
  const float x0 = x[3 * i], x1 = x[3 * i + 1], x2 = x[3 * i + 2], v0 = v[3 * i], v1 = v[3 * i + 1], v2 = v[3 * i + 2];
  const float n0 = nr[k], n1 = nr[k + 1], n2 = nr[k + 2];
  const float a = dot3(n0, n1, n2, p[k] - x0, p[k + 1] - x1, p[k + 2] - x2);        // :199
  const float t = a / dot3(n0, n1, n2, v0, v1, v2);                                   // :200
  xo[3 * i] = fmaf(t, v0, x0); xo[3 * i + 1] = fmaf(t, v1, x1); xo[3 * i + 2] = fmaf(t, v2, x2);   // :202
}

__global__ void __launch_bounds__(256) k_rays_to_plane_bwd(size_t n, const float* __restrict__ x, const float* __restrict__ v,
                                                           const float* __restrict__ p, const float* __restrict__ nr,
                                                           int plane_stride, const float* __restrict__ g,
                                                           float* __restrict__ gx, float* __restrict__ gv) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const size_t k = i * (size_t)plane_stride;
  const float x0 = x[3 * i], x1 = x[3 * i + 1], x2 = x[3 * i + 2], v0 = v[3 * i], v1 = v[3 * i + 1], v2 = v[3 * i + 2];
  const float n0 = nr[k], n1 = nr[k + 1], n2 = nr[k + 2];
  const float g0 = g[3 * i], g1 = g[3 * i + 1], g2 = g[3 * i + 2];
  const float a = dot3(n0, n1, n2, p[k] - x0, p[k + 1] - x1, p[k + 2] - x2);
  const float inv_b = 1.f / dot3(n0, n1, n2, v0, v1, v2);
  const float t = a * inv_b;
  const float c = dot3(g0, g1, g2, v0, v1, v2) * inv_b;       // g.v / b
  gx[3 * i] = fmaf(-c, n0, g0); gx[3 * i + 1] = fmaf(-c, n1, g1); gx[3 * i + 2] = fmaf(-c, n2, g2);
  const float tc = t * c;
  gv[3 * i] = fmaf(t, g0, -tc * n0); gv[3 * i + 1] = fmaf(t, g1, -tc * n1); gv[3 * i + 2] = fmaf(t, g2, -tc * n2);
}

}  // namespace drrt

extern "C" int drrt_rays_to_plane_f32(size_t n, const float* x, const float* v, const float* plane_p, const float* plane_n,
                                      int plane_stride, float* x_out, void* stream) {
  if (plane_stride != 0 && plane_stride != 3) return fail(DRRT_ERR_ARG, "plane_stride must be 0 or 3");
  if (n == 0) return DRRT_OK;
  if (!x || !v || !plane_p || !plane_n || !x_out) return fail(DRRT_ERR_ARG, "null pointer");
  return launch_1d(k_rays_to_plane, n, stream, n, x, v, plane_p, plane_n, plane_stride, x_out);
}

extern "C" int drrt_rays_to_plane_bwd_f32(size_t n, const float* x, const float* v, const float* plane_p,
                                          const float* plane_n, int plane_stride, const float* grad_x_out,
                                          float* grad_x, float* grad_v, void* stream) {
  if (plane_stride != 0 && plane_stride != 3) return fail(DRRT_ERR_ARG, "plane_stride must be 0 or 3");
  if (n == 0) return DRRT_OK;
  if (!x || !v || !plane_p || !plane_n || !grad_x_out || !grad_x || !grad_v) return fail(DRRT_ERR_ARG, "null pointer");
  return launch_1d(k_rays_to_plane_bwd, n, stream, n, x, v, plane_p, plane_n, plane_stride, grad_x_out, grad_x, grad_v);
}
