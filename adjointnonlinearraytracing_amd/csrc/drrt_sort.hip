// drrt_sort.hip -- locality sort of rays (device side, rocPRIM radix sort).
//
// Not part of the reference (enoki processes rays in caller order, array-at-a-time); this is the
// MI355X-side answer to SURVEY.md section 7 step 5: the 64 rays of a wave should stay spatially
// close for their WHOLE march, so that each of the 8 taps of a wave-step hits a handful of 128-B
// lines and the adjoint's scatter targets fall into the wave's LDS gradient window.
//
// Round 3 key ("light-field key", the default): a ray is the line it travels on, i.e. a direction and a 2-D offset in the
// plane perpendicular to it.
//   direction  octahedral map of the unit direction, cut into 31 x 31 cells (an ODD count: +-x, +-y, +z are cell CENTRES);
//              the cell index is the major part of the key, so a collimated view is one contiguous key range;
//   offset     the point of the line closest to the box centre, in the orthonormal frame (t1, t2) of the CELL's centre
//              direction (every ray of a cell uses the same frame), scaled by a power of two of the box extent and cut
//              into 2048 x 2048 cells; the minor part of the key is the HILBERT index of that cell.  10 + 22 bits: a 32-bit
//              key (the sort moves 8 instead of 12 bytes per ray and pass).
// Why Hilbert and not the Z-order interleave of rounds 1-2: 64 consecutive rays of a Z-order are an aligned 8 x 8 tile only
// when the sampling grid happens to be aligned with the key cells (the metric's pixel-aligned plane source); shift the
// same source by a third of a pixel and 11 % of the bundles straddle two far-apart tiles (measured: adjoint 4.8 -> 7.1 ms),
// and the views of core/source.py rand_rays_cube + random_rotate_ic, oblique to every axis, gave bundles whose box of grid
// cells was 12 cells wide in the median (82 % wider than the 9^3 window; adjoint 4.8 -> 20 ms: global-atomic fallback).  Any
// 64 consecutive cells of a Hilbert curve are a connected, compact patch; aligned 8 x 8 blocks are still contiguous, so the
// aligned source keeps its perfect tiles (tools/bundle_stats.py: offline comparison of the keys).  For the axis-aligned
// frame the power-of-two scale keeps pixel boundaries on key-cell boundaries.
//
// Rounds 1-2 key (DRRT_FLAG_CHORD_KEY, kept for A-B): 60-bit "light-field Z-order": the straight line through the ray
// (from where it meets the grid box along its march direction to where that line leaves the box again) is described by
// its two end points, each quantised to 10 bits per axis, and the 6 coordinates are bit-interleaved (Morton order in 6-D).
// For the adjoint the march direction is -vt and the "start" is the recorded exit sample xt.
// The permutation only changes the VISIT order; results are written back in the caller's ray order.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <stdint.h>

#include "drrt_device.h"
#include "drrt_keys.h"

namespace drrt {

// one ray component in storage format `io` (0 fp32, 1 IEEE half, 2 the 16-bit ray state of drrt_device.h)
__device__ __forceinline__ float ldr(const Vol& V, const void* p, size_t k, int io, bool is_pos) {
  if (io == 3) return is_pos ? q16_pos_dec(V, ((const uint16_t*)p)[k]) : ((const float*)p)[k];
  if (io == 2) return is_pos ? q16_pos_dec(V, ((const uint16_t*)p)[k]) : q16_vel_dec(((const int16_t*)p)[k]);
  return io ? __half2float(((const __half*)p)[k]) : ((const float*)p)[k];
}

__global__ void __launch_bounds__(256) k_chord_keys(Vol V, size_t n, const void* __restrict__ pos,
                                                    const void* __restrict__ vel, int io_half, float dir_sign,
                                                    uint64_t* __restrict__ keys, uint32_t* __restrict__ idx) {
  size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float p[3] = {ldr(V, pos, 3 * i, io_half, true), ldr(V, pos, 3 * i + 1, io_half, true), ldr(V, pos, 3 * i + 2, io_half, true)};
  float d[3] = {dir_sign * ldr(V, vel, 3 * i, io_half, false), dir_sign * ldr(V, vel, 3 * i + 1, io_half, false),
                dir_sign * ldr(V, vel, 3 * i + 2, io_half, false)};
  keys[i] = chord_key(V, p, d);
  idx[i] = (uint32_t)i;
}

// ---- light-field key: lightfield_key of drrt_keys.h ----------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_lightfield_keys(Vol V, size_t n, const void* __restrict__ pos,
                                                         const void* __restrict__ vel, int io_half, float dir_sign,
                                                         uint32_t* __restrict__ keys, uint32_t* __restrict__ idx) {
  size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float p[3] = {ldr(V, pos, 3 * i, io_half, true), ldr(V, pos, 3 * i + 1, io_half, true), ldr(V, pos, 3 * i + 2, io_half, true)};
  float d[3] = {dir_sign * ldr(V, vel, 3 * i, io_half, false), dir_sign * ldr(V, vel, 3 * i + 1, io_half, false),
                dir_sign * ldr(V, vel, 3 * i + 2, io_half, false)};
  idx[i] = (uint32_t)i;
  keys[i] = lightfield_key(V, p, d);
}

static inline size_t al(size_t v) { return (v + 255) / 256 * 256; }

// (rocPRIM picks the algorithm by size: up to radix_sort_config<>::merge_sort_limit = 1M items a block sort + merge passes
// -- 21 launches of 5-9 us for the metric's 1 048 576 rays, 0.167 ms --, Onesweep above.  Lowering the limit so that 1M rays
// take Onesweep was measured, same box: 0.170 ms at 1M rays, and 0.137 against 0.057 ms for a 131 072-ray shard -- Onesweep's
// fixed cost is larger than the merge passes'.  The default stays.)
static size_t radix_temp_bytes(size_t n) {
  size_t t64 = 0, t32 = 0;          // both key widths share the buffers: the larger temporary storage
  hipError_t e = rocprim::radix_sort_pairs(nullptr, t64, (const uint64_t*)nullptr, (uint64_t*)nullptr,
                                          (const uint32_t*)nullptr, (uint32_t*)nullptr, n, 0u, (unsigned)kKeyBits,
                                          (hipStream_t)0);
  hipError_t e2 = rocprim::radix_sort_pairs(nullptr, t32, (const uint32_t*)nullptr, (uint32_t*)nullptr,
                                           (const uint32_t*)nullptr, (uint32_t*)nullptr, n, 0u, (unsigned)kLfKeyBits,
                                           (hipStream_t)0);
  size_t temp = t64 > t32 ? t64 : t32;
  if (e != hipSuccess || e2 != hipSuccess || temp == 0) {   // no device visible (CPU-only import): conservative bound
    (void)hipGetLastError();
    temp = n * 32 + (1u << 20);
  }
  return temp;
}

size_t sort_workspace_bytes(size_t n) {
  return 2 * al(n * sizeof(uint64_t)) + 2 * al(n * sizeof(uint32_t)) + al(radix_temp_bytes(n));
}

hipError_t sort_rays_by_entry_voxel(const Vol& V, float h, size_t n, const void* pos, const void* vel, int io_half,
                                    float dir_sign, void* ws, size_t ws_bytes, const uint32_t** perm_out,
                                    hipStream_t stream, bool chord_key) {
  (void)h;
  char* base = (char*)ws;
  const size_t k8 = al(n * sizeof(uint64_t)), k4 = al(n * sizeof(uint32_t));
  uint64_t* keys_in = (uint64_t*)(base);
  uint64_t* keys_out = (uint64_t*)(base + k8);
  uint32_t* idx_in = (uint32_t*)(base + 2 * k8);
  uint32_t* idx_out = (uint32_t*)(base + 2 * k8 + k4);
  void* temp = base + 2 * k8 + 2 * k4;
  size_t temp_bytes = ws_bytes - (2 * k8 + 2 * k4);
  hipError_t e;
  if (chord_key) {
    hipLaunchKernelGGL(k_chord_keys, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, V, n, pos, vel,
                       io_half, dir_sign, keys_in, idx_in);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = rocprim::radix_sort_pairs(temp, temp_bytes, (const uint64_t*)keys_in, keys_out,
                                  (const uint32_t*)idx_in, idx_out, n, 0u, (unsigned)kKeyBits, stream);
  } else {                                     // 32-bit keys in the same buffers
    hipLaunchKernelGGL(k_lightfield_keys, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, V, n, pos, vel,
                       io_half, dir_sign, (uint32_t*)keys_in, idx_in);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = rocprim::radix_sort_pairs(temp, temp_bytes, (const uint32_t*)keys_in, (uint32_t*)keys_out,
                                  (const uint32_t*)idx_in, idx_out, n, 0u, (unsigned)kLfKeyBits, stream);
  }
  *perm_out = idx_out;
  return e;
}

}  // namespace drrt
