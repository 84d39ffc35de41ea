// drrt_keys.h -- the per-ray arithmetic of the locality-sort keys (drrt_sort.hip explains what the keys are for).
//
// __host__ __device__, like the per-ray code of drrt_device.h: k_lightfield_keys / k_chord_keys call it on the device, and
// tests/hostcheck compiles it for the host (`--cuda-host-only -ffp-contract=off`), where tests/test_sortkey_ref.py compares it
// with a numpy restatement bit for bit and with a float64 referee (oracle/sortkey_ref.py).  The order of the floating-point
// operations IS the key: the library is built with -ffp-contract=off, every FMA below is written out, and the GPU tier
// (tests/test_sort_order.py) asserts that the device's visit order equals the stable argsort of the host build's keys.
#pragma once
#include <stdint.h>

#include "drrt_device.h"

namespace drrt {

// ---- chord key (DRRT_FLAG_CHORD_KEY) ---------------------------------------------------------------------------------
constexpr int kKeyBitsPerAxis = 10;
constexpr int kKeyBits = 6 * kKeyBitsPerAxis;

// p: where the ray stands; d: where it heads (dir_sign already applied)
DRRT_HD uint64_t chord_key(const Vol& V, const float p[3], const float d[3]) {
  const float b[3] = {V.bx, V.by, V.bz};
  float tmin = 0.f, tmax = 3.0e38f;
  bool hit = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    if (fabsf(d[a]) > 1e-20f) {
      float inv = 1.f / d[a];
      float t1 = (0.f - p[a]) * inv, t2 = (b[a] - p[a]) * inv;
      tmin = fmaxf(tmin, fminf(t1, t2));
      tmax = fminf(tmax, fmaxf(t1, t2));
    } else if (p[a] < 0.f || p[a] > b[a]) {
      hit = false;
    }
  }
  hit = hit && tmax >= tmin;
  const float t0 = hit ? tmin : 0.f, t1 = hit ? tmax : 0.f;
  uint32_t q[6];
  const float scale = (float)(1 << kKeyBitsPerAxis);
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    float inv_b = b[a] > 0.f ? 1.f / b[a] : 0.f;
    float e0 = fminf(fmaxf(fmaf(t0, d[a], p[a]) * inv_b, 0.f), 0.99999f);
    float e1 = fminf(fmaxf(fmaf(t1, d[a], p[a]) * inv_b, 0.f), 0.99999f);
    q[a] = (uint32_t)(e0 * scale);
    q[3 + a] = (uint32_t)(e1 * scale);
  }
  uint64_t key = 0;
#pragma unroll
  for (int bit = 0; bit < kKeyBitsPerAxis; ++bit)
#pragma unroll
    for (int j = 0; j < 6; ++j)
      key |= (uint64_t)((q[j] >> bit) & 1u) << (6 * bit + (5 - j));
  return key;
}

// ---- light-field key ---------------------------------------------------------------------------------------------
constexpr int kDirHalf = 15;                         // direction cells per octahedral axis: 2 * kDirHalf + 1 = 31
constexpr int kPosBits = 11;                         // offset cells per axis: 2048
constexpr int kLfKeyBits = 2 * kPosBits + 10;        // 22 + 10 (31 * 31 = 961 direction cells < 2^10): 32 bits

DRRT_HD uint32_t hilbert2(uint32_t x, uint32_t y) {      // x, y < 2^kPosBits
  uint32_t d = 0;
#pragma unroll
  for (int b = kPosBits - 1; b >= 0; --b) {
    const uint32_t s = 1u << b, rx = (x >> b) & 1u, ry = (y >> b) & 1u;
    d += s * s * ((3u * rx) ^ ry);
    if (ry == 0u) {                                  // rotate / reflect the quadrant
      if (rx == 1u) { x = s - 1u - x; y = s - 1u - y; }
      const uint32_t t = x; x = y; y = t;
    }
    x &= s - 1u; y &= s - 1u;
  }
  return d;
}

// octahedral map of the UNIT direction d -> cell (a, b) in [-kDirHalf, kDirHalf]^2
DRRT_HD void lf_dir_cell(const float d[3], int& a, int& b) {
  const float l1 = fabsf(d[0]) + fabsf(d[1]) + fabsf(d[2]);
  float ox = d[0] / l1, oy = d[1] / l1;
  if (d[2] < 0.f) {
    const float fx = (1.f - fabsf(oy)) * (ox >= 0.f ? 1.f : -1.f), fy = (1.f - fabsf(ox)) * (oy >= 0.f ? 1.f : -1.f);
    ox = fx; oy = fy;
  }
  a = (int)rintf(ox * (float)kDirHalf); b = (int)rintf(oy * (float)kDirHalf);
  a = a < -kDirHalf ? -kDirHalf : (a > kDirHalf ? kDirHalf : a);
  b = b < -kDirHalf ? -kDirHalf : (b > kDirHalf ? kDirHalf : b);
}

// centre direction c of the cell (a, b), and ITS frame (t1, t2): the coordinate axis least aligned with c, made orthogonal
// to it, and c x t1.  A function of the two integers only, so every ray of a cell uses the same frame.
DRRT_HD void lf_cell_frame(int a, int b, float c[3], float t1[3], float t2[3]) {
  float cx = (float)a / (float)kDirHalf, cy = (float)b / (float)kDirHalf, cz = 1.f - fabsf(cx) - fabsf(cy);
  if (cz < 0.f) {
    const float fx = (1.f - fabsf(cy)) * (cx >= 0.f ? 1.f : -1.f), fy = (1.f - fabsf(cx)) * (cy >= 0.f ? 1.f : -1.f);
    cx = fx; cy = fy;
  }
  const float cl = 1.f / sqrtf(cx * cx + cy * cy + cz * cz);
  c[0] = cx * cl; c[1] = cy * cl; c[2] = cz * cl;
  int ax = 0;
  if (fabsf(c[1]) < fabsf(c[ax])) ax = 1;
  if (fabsf(c[2]) < fabsf(c[ax])) ax = 2;
  t1[0] = -c[ax] * c[0]; t1[1] = -c[ax] * c[1]; t1[2] = -c[ax] * c[2];
  t1[ax] += 1.f;
  const float tl = 1.f / sqrtf(t1[0] * t1[0] + t1[1] * t1[1] + t1[2] * t1[2]);
  t1[0] *= tl; t1[1] *= tl; t1[2] *= tl;
  t2[0] = c[1] * t1[2] - c[2] * t1[1]; t2[1] = c[2] * t1[0] - c[0] * t1[2]; t2[2] = c[0] * t1[1] - c[1] * t1[0];
}

// p: where the ray stands; d_in: where it heads (dir_sign already applied), any length
DRRT_HD uint32_t lightfield_key(const Vol& V, const float p[3], const float d_in[3]) {
  float d[3] = {d_in[0], d_in[1], d_in[2]};
  const float len = sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
  if (!(len > 1e-30f) || !(len < 3.0e38f)) return 0;                      // a ray at rest (or non-finite): any place will do
  const float il = 1.f / len;
  d[0] *= il; d[1] *= il; d[2] *= il;
  int a, b;
  lf_dir_cell(d, a, b);
  float c[3], t1[3], t2[3];
  lf_cell_frame(a, b, c, t1, t2);
  // the point of the line closest to the box centre, in that frame; scale 1 / (2 E), E = the largest box extent
  const float w[3] = {p[0] - 0.5f * V.bx, p[1] - 0.5f * V.by, p[2] - 0.5f * V.bz};
  const float wd = w[0] * d[0] + w[1] * d[1] + w[2] * d[2];
  const float q[3] = {w[0] - wd * d[0], w[1] - wd * d[1], w[2] - wd * d[2]};
  const float ext = fmaxf(V.bx, fmaxf(V.by, V.bz));
  const float sc = ext > 0.f ? 0.5f / ext : 0.f;
  const float u = (q[0] * t1[0] + q[1] * t1[1] + q[2] * t1[2]) * sc + 0.5f;
  const float v = (q[0] * t2[0] + q[1] * t2[1] + q[2] * t2[2]) * sc + 0.5f;
  const float cells = (float)(1 << kPosBits);
  const uint32_t qu = (uint32_t)fminf(fmaxf(u * cells, 0.f), cells - 1.f);
  const uint32_t qv = (uint32_t)fminf(fmaxf(v * cells, 0.f), cells - 1.f);
  const uint32_t cell = (uint32_t)((a + kDirHalf) * (2 * kDirHalf + 1) + (b + kDirHalf));
  return (cell << (2 * kPosBits)) | hilbert2(qu, qv);
}

}  // namespace drrt
