// drrt_adjoint_box.hip -- gfx950 kernels of the adjoint march Tracer::backtrace / backtrace_sdf
// (/root/reference/src/tracer.cpp:384-509) for compact ray bundles: k_backtrace_flat with its compile-time box window,
// the bundle classification that chooses between it and the ring-window kernel (drrt_adjoint_ring.hip), and the
// one-atomic-per-tap kernel every windowed variant is cross-checked against.
#include "drrt_march.h"

namespace drrt {

template <int MODE>
__global__ void __launch_bounds__(kBlock) k_backtrace_direct(BackArgs a) {
  const size_t t = (size_t)blockIdx.x * kBlock + threadIdx.x;
  unsigned steps = 0;
  size_t i;
  if (ray_index(a.perm, t, a.n, i)) {
    Ray3 p = ld3(a.xt, i, a.io_half, &a.vol, RAY_POS), u = ld3(a.vt, i, a.io_half, &a.vol, RAY_VEL), gxv = ld3(a.dx, i, a.io_half), gvv = ld3(a.dv, i, a.io_half);
    const float pp[3] = {p.x, p.y, p.z}, vv[3] = {u.x, u.y, u.z};
    const float dxx[3] = {gxv.x, gxv.y, gxv.z}, dvv[3] = {gvv.x, gvv.y, gvv.z};
    float* grad = a.grad;
    steps = backtrace_ray<MODE>(a.vol, a.sdf, a.ds, a.grad_scale, a.max_steps, pp, vv, dxx, dvv,
      [grad](const Cell& c, const Corners& w) {
        float* g = grad + c.base;
        atomic_add_f32(g, w.c000);                    atomic_add_f32(g + c.ox, w.c100);
        atomic_add_f32(g + c.oy, w.c010);             atomic_add_f32(g + c.oy + c.ox, w.c110);
        atomic_add_f32(g + c.oz, w.c001);             atomic_add_f32(g + c.oz + c.ox, w.c101);
        atomic_add_f32(g + c.oz + c.oy, w.c011);      atomic_add_f32(g + c.oz + c.oy + c.ox, w.c111);
      });
  }
  block_stats(a.stats, steps, 0u);
}

// ---------------------------------------------------------------------------------------------
// adjoint march with per-wave LDS gradient windows
//
// Why: one global fp32 atomic per tap runs at the memory-side atomic rate, and that rate collapses
// when many lanes hit the same few addresses (measured on MI355X, Luneburg 256^3 / 1M rays: 237 ms
// for 4.1e9 lane-atomics -- every ray passes through the handful of voxels around the focus).
// Rays of a wave are spatially coherent (locality sort), so each wave keeps a small box of
// gradient voxels ("window") in LDS and accumulates there (ds_add_f64, fed by per-lane register
// accumulators that emit one cell face at a time, see below); the window is flushed to the global
// grid -- one fp32 atomic per touched voxel, contiguous in x -- only when the rays walk out of it.  Lanes whose cell
// falls outside the window (incoherent wave, clamped boundary cell) fall back to direct global atomics, so the result
// never depends on the window.
//
//   window      kWinX x kWinY x kWinZ voxels of double accumulators, row pitch kWinPX (measured, final
//               kernels: edge 9 beats 7, 8, 10, 12; padding the pitch or not is within 1 %)
//   anchor      around the cell of the wave's median contributing lane, shifted towards its
//               direction of travel (most of the window lies ahead of the rays)
//   re-anchor   as soon as a contributing lane misses the window (wave-uniform decision); if lanes
//               still miss afterwards the window stays put for 4 steps (no thrashing)
//   sync        none across waves: every wave owns its window; all control flow around the
//               cooperative flush is wave-uniform (ballot / readlane values)
// ---------------------------------------------------------------------------------------------
#ifndef DRRT_WIN
#define DRRT_WIN 9     // measured on MI355X (256^3 / 1M rays, same box): 7 -> 6.75 ms, 8 -> 6.08, 9 -> 4.94, 10 -> 5.23
#endif
#ifndef DRRT_WIN_PAD
#define DRRT_WIN_PAD 1
#endif
constexpr int kWinX = DRRT_WIN, kWinY = DRRT_WIN, kWinZ = DRRT_WIN;
constexpr int kWinPX = DRRT_WIN + DRRT_WIN_PAD;           // row pitch
constexpr int kWinSY = kWinPX, kWinSZ = kWinPX * kWinY;   // LDS strides of y and z
constexpr int kWinFloats = kWinSZ * kWinZ;                // 810 slots = 6.3 KiB per wave (9^3 window, pitch 10)
static_assert(kWinFloats < (1 << 16), "win_face_key keeps a window slot in 16 bits");

// Flush the wave's window into the global grid and leave it zeroed.  Called with all 64 lanes.
// The window's rows (a row = the kWinX slots of one (ly, lz)) are contiguous in LDS at pitch kWinPX, so the flush walks
// them linearly: a pass covers 64 / kWinX rows (lane -> row lane / kWinX, slot lane % kWinX), the LDS address advances
// by a constant and the grid address by a constant plus a wrap from one z-slice to the next.  Passes go in batches of
// four: the four LDS exchanges are issued before the first result is used, so a flush costs ceil(rows / 7 / 4) LDS
// round trips (3 for a whole 9^3 window) instead of one per pass.
// Only the z-planes that lanes have held slots in since the last flush are walked: `planes` (wave-uniform, not 0; bit lz =
// plane lz may have been written, win_index) names them, and the walk goes from the pass that holds the first row of the
// lowest such plane to the last row of the highest.  The rest of the window holds zeros.  (The headline's bundles are two
// or three cells across: three or four planes of nine, two batches instead of three.)
__device__ __forceinline__ void win_flush(win_t* win, int ox, int oy, int oz, float* __restrict__ grad,
                                          const Vol& V, int lane, unsigned planes) {
  constexpr int kRowsPerPass = kWave / kWinX, kBatch = 4;
  static_assert(kWinX <= 16 && kRowsPerPass <= kWinY, "win_flush: one pass must not span more than two z-slices");
  wave_lds_fence();
  const int z_first = __builtin_ctz(planes), z_last = 31 - __builtin_clz(planes);
  const int p_first = (z_first * kWinY) / kRowsPerPass;                  // the pass of the first row to flush
  const int r_end = (z_last + 1) * kWinY;                                // one past the last row to flush
  const int rsub = lane / kWinX, lx = lane - rsub * kWinX;
  const bool lane_ok = rsub < kRowsPerPass;
  int r = p_first * kRowsPerPass + rsub;                                 // row index, its lz and ly
  const int lz = (int)((unsigned)r / (unsigned)kWinY);
  int ly = r - lz * kWinY;
  win_t* wl = win + r * kWinPX + lx;
  unsigned go = (unsigned)(oz + lz) * (unsigned)V.sz + (unsigned)(oy + ly) * (unsigned)V.sy + (unsigned)(ox + lx);
  const unsigned step_y = (unsigned)kRowsPerPass * (unsigned)V.sy, wrap = (unsigned)V.sz - (unsigned)kWinY * (unsigned)V.sy;
#pragma unroll 1
  for (int p0 = p_first; p0 * kRowsPerPass < r_end; p0 += kBatch) {
    win_t v[kBatch];
    unsigned g[kBatch];
#pragma unroll
    for (int b = 0; b < kBatch; ++b) {
      v[b] = (win_t)0; g[b] = go;
      // ds_wrxchg_rtn_b64: read the accumulated value and reset the slot in one LDS op
      if (lane_ok & (r < r_end)) v[b] = __hip_atomic_exchange(wl, (win_t)0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
      r += kRowsPerPass; wl += kRowsPerPass * kWinPX; ly += kRowsPerPass; go += step_y;
      if (ly >= kWinY) { ly -= kWinY; go += wrap; }
    }
#pragma unroll
    for (int b = 0; b < kBatch; ++b)
      if (v[b] != (win_t)0) atomic_add_f32_at(grad, g[b], (float)v[b]);
  }
  wave_lds_fence();
}


// ---------------------------------------------------------------------------------------------
// k_backtrace_flat: the adjoint march organised around ONE invariant -- the lane's register accumulators always belong to
// the cell the ray stands on -- so that the hot loop carries no second cell, no "accumulator cell" bookkeeping and no
// per-step window test:
//
//   top      taps(x_k) arrive (gather issued one iteration earlier) -> n, grad n, H -> v_k -> still active?
//            8 splat weights of step k (they need the in-cell fractions of cell k) -> accumulators += weights
//   step     x_{k+1} = x_k - ds v_k ; locate its cell IN PLACE (the fractions of cell k are dead by now) ;
//            issue its gather unless the ray stays in its cell
//   then     lambda / mu recurrences (under the gather)
//   leave    only if the cell changed: the ray LEAVES cell k -- a move across one face hands the four corners left
//            behind to the LDS window (pair / quad DPP pre-reduced) and carries the shared four; anything else hands
//            over all eight -- and the window index of the new cell is computed once, here (a miss votes for a
//            re-anchor).  A ray that ends hands over all eight.
// Per-ray arithmetic is adj_sample / adj_contrib of drrt_device.h (the two halves of adj_step, which the one-atomic-per-tap
// kernel above runs as is): bit-identical contributions, only the order in which they reach the grid differs, i.e. the
// usual fp32 summation-order noise.  (Rounds 1-2 had a predecessor, k_backtrace_win, with a second "accumulator cell" per
// lane: 5.45 ms against 4.5 ms for this kernel on 256^3 / 1M rays; removed in round 4, NOTES.md.)
// ---------------------------------------------------------------------------------------------
// ---- window of k_backtrace_flat --------------------------------------------------------------------------------
// (Bundles that do not sit in the compile-time window -- sparse views, views oblique to the grid -- are the ring kernel's.)
struct WinOrg { int ox, oy, oz; };   // corner 000 of the wave's window, in voxels (far away = nothing is inside); wave-uniform
__device__ __forceinline__ int wave_min_i32(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, kWave));
  return v;
}
__device__ __forceinline__ int wave_max_i32(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, kWave));
  return v;
}
// OR over the wave, wave-uniform.  Called with all 64 lanes: four row_shr steps leave a row's OR in its last lane (a lane a
// shift does not reach reads 0), and the four rows meet in scalars -- no LDS.
__device__ __forceinline__ unsigned wave_or_u32(unsigned v) {
  v |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xF, 0xF, false);   // row_shr:1
  v |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xF, 0xF, false);   // row_shr:2
  v |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xF, 0xF, false);   // row_shr:4
  v |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xF, 0xF, false);   // row_shr:8
  return (unsigned)(__builtin_amdgcn_readlane((int)v, 15) | __builtin_amdgcn_readlane((int)v, 31) |
                    __builtin_amdgcn_readlane((int)v, 47) | __builtin_amdgcn_readlane((int)v, 63));
}
// Window slot of the cell (cx, cy, cz), or -1 when it is not inside.  A cell that is inside has its two z-planes marked in the
// lane's `planes` here, where the lane gets the slot: every add a lane makes to the window goes to the cell whose slot it
// holds (a face, all eight corners, the hand-over of a ray that ends or is cut off by the step budget), so the marks cover
// every slot written, and win_flush walks the marked planes only.  (Marking where the slot is handed out costs a shift and
// an OR per leave; marking in the four places that add would need the plane again there, i.e. a register per lane.)
static_assert(kWinZ <= 31, "one bit per z-plane of the window");
__device__ __forceinline__ int win_index(int wox, int woy, int woz, int cx, int cy, int cz, unsigned& planes) {
  const int lx = cx - wox, ly = cy - woy, lz = cz - woz;
  const bool in = ((unsigned)lx < (unsigned)(kWinX - 1)) & ((unsigned)ly < (unsigned)(kWinY - 1)) &
                  ((unsigned)lz < (unsigned)(kWinZ - 1));
  planes |= (in ? 3u : 0u) << (lz & 31);
  // v_mad_u32_u24 by hand: with constant strides the compiler turns the 24-bit multiply into the quarter-rate
  // v_mul_lo_u32 (lx, ly, lz are small and non-negative whenever the result is used)
  int r;
  asm("v_mad_u32_u24 %0, %1, %2, %3" : "=v"(r) : "v"(ly), "s"(kWinSY), "v"(lx));
  asm("v_mad_u32_u24 %0, %1, %2, %3" : "=v"(r) : "v"(lz), "s"(kWinSZ), "v"(r));
  return in ? r : -1;
}

// all 8 accumulated corners of the regular cell `base` (window slot lidx, or -1: straight to the grid)
template <bool PRE = true>
__device__ __forceinline__ bool flat_emit8(win_t* win, int wsy, int wsz, float* grad, int sy, int sz, int lidx, int base,
                                           f2 p00, f2 p10, f2 p01, f2 p11) {
  if (lidx >= 0) {
    // PRE: quad pre-reduction -- when the 4 lanes of a quad hand over the same cell, one lane adds the quad's sums
    const bool same = PRE ? quad_same_key(lidx) : false;
    float v[8] = {p00.x, p00.y, p10.x, p10.y, p01.x, p01.y, p11.x, p11.y};
    if (PRE) {
#pragma unroll
      for (int k = 0; k < 8; ++k) { const float qs = quad_sum(v[k]); v[k] = same ? qs : v[k]; }
    }
    if (!same || (threadIdx.x & 3u) == 0u) {
      win_t* q = win + lidx;
      atomicAdd(q, (win_t)v[0]);                 atomicAdd(q + 1, (win_t)v[1]);
      atomicAdd(q + wsy, (win_t)v[2]);           atomicAdd(q + wsy + 1, (win_t)v[3]);
      atomicAdd(q + wsz, (win_t)v[4]);           atomicAdd(q + wsz + 1, (win_t)v[5]);
      atomicAdd(q + wsz + wsy, (win_t)v[6]);     atomicAdd(q + wsz + wsy + 1, (win_t)v[7]);
    }
    return true;
  }
  const unsigned g = (unsigned)base, gy = g + (unsigned)sy, gz = g + (unsigned)sz, gzy = gz + (unsigned)sy;
  atomic_add_f32_at(grad, g, p00.x);    atomic_add_f32_at(grad, g + 1u, p00.y);
  atomic_add_f32_at(grad, gy, p10.x);   atomic_add_f32_at(grad, gy + 1u, p10.y);
  atomic_add_f32_at(grad, gz, p01.x);   atomic_add_f32_at(grad, gz + 1u, p01.y);
  atomic_add_f32_at(grad, gzy, p11.x);  atomic_add_f32_at(grad, gzy + 1u, p11.y);
  return false;
}

// one face of a regular cell handed to the window: corners e0..e3 go to the slots qi, qi + LP, qi + LQ, qi + LQ + LP, where
// qi = key & 0xffff: the key names the face (slot of its first corner | axis << 16; win_face_key).
// Pair / quad pre-reduction: lanes of a quad that hand over the same face (same key; the lanes of a quad that are not in
// the branch read as -1 / 0) add once, the pair's or the quad's sums.  Returns whether this lane added.
__device__ __forceinline__ constexpr int win_face_key(int slot_offset, int axis) { return slot_offset | (axis << 16); }
__device__ __forceinline__ bool win_emit4(win_t* win, int key, int LP, int LQ, float e0, float e1, float e2, float e3) {
  const int qi = key & 0xffff;
  const int k1 = __builtin_amdgcn_update_dpp(-1, key, 0xB1, 0xF, 0xF, false);   // quad_perm [1,0,3,2]
  const int k2 = __builtin_amdgcn_update_dpp(-1, key, 0x4E, 0xF, 0xF, false);   // quad_perm [2,3,0,1]
  const int k3 = __builtin_amdgcn_update_dpp(-1, key, 0x1B, 0xF, 0xF, false);   // quad_perm [3,2,1,0]
  const bool psame = k1 == key;
  const bool same = psame & (k2 == key) & (k3 == key);
  // the sums are built under the tests (a lane's pair / quad partners pass the same test, so the lanes it reads are enabled):
  // q = e (+ the pair partner's), then (+ the other pair's) -- four v_add_f32_dpp per level, no selects
  float q0 = e0, q1 = e1, q2 = e2, q3 = e3;
  if (psame) {
    q0 += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, q0), 0xB1, 0xF, 0xF, false));
    q1 += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, q1), 0xB1, 0xF, 0xF, false));
    q2 += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, q2), 0xB1, 0xF, 0xF, false));
    q3 += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, q3), 0xB1, 0xF, 0xF, false));
  }
  if (same) {
    q0 += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, q0), 0x4E, 0xF, 0xF, false));
    q1 += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, q1), 0x4E, 0xF, 0xF, false));
    q2 += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, q2), 0x4E, 0xF, 0xF, false));
    q3 += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, q3), 0x4E, 0xF, 0xF, false));
  }
  const unsigned ql = threadIdx.x & 3u;
  const bool add = same ? ql == 0u : (psame ? (ql & 1u) == 0u : true);
  if (add) {
    win_t* q = win + qi;
    atomicAdd(q, (win_t)q0);      atomicAdd(q + LP, (win_t)q1);
    atomicAdd(q + LQ, (win_t)q2); atomicAdd(q + LQ + LP, (win_t)q3);
  }
  return add;
}

__global__ void __launch_bounds__(kBlock) k_bundle_classify(BackArgs a) {
  __shared__ unsigned s_cnt[7];                  // the block's counters ([5] is the host's): one set of global atomics per block, not per wave
  if (threadIdx.x < 7) s_cnt[threadIdx.x] = 0u;
  __syncthreads();
  const Vol& V = a.vol;
  const size_t t = (size_t)blockIdx.x * kClassifyStride * kBlock + threadIdx.x;
  const int lane = threadIdx.x & (kWave - 1);
  size_t i;
  bool ok = false;
  int cx = 0, cy = 0, cz = 0, cbase = -1;
  unsigned fk = 0u;                               // the forward march's iteration count of the ray (step hint), 0 without
  if (ray_index(a.perm, t, a.n, i)) {
    const Ray3 p = ld3(a.xt, i, a.io_half, &a.vol, RAY_POS);
    const Cell c = locate(V, p.x, p.y, p.z);
    cx = c.ix; cy = c.iy; cz = c.iz; cbase = c.base; ok = true;
    if (a.fsteps != nullptr) fk = a.fsteps[i];
  }
  const int pbase = __builtin_amdgcn_update_dpp(-2, cbase, 0xB1, 0xF, 0xF, false);      // the pair partner's cell (quad_perm [1,0,3,2])
  const unsigned paired = (unsigned)__popcll(__ballot(ok & (pbase == cbase)));
  const int big = 1 << 28;
  const int x0 = wave_min_i32(ok ? cx : big), x1 = wave_max_i32(ok ? cx : -big);
  const int y0 = wave_min_i32(ok ? cy : big), y1 = wave_max_i32(ok ? cy : -big);
  const int z0 = wave_min_i32(ok ? cz : big), z1 = wave_max_i32(ok ? cz : -big);
  const unsigned lanes = (unsigned)__popcll(__ballot(ok));
  // mean cell of the bundle (rounded); cells are < 2^24 per axis, 64 of them fit an int
  const float inv = 1.0f / (float)max(lanes, 1u);
  const int mx = (int)floorf((float)(int)wave_sum_u32(ok ? (unsigned)cx : 0u) * inv + 0.5f);
  const int my = (int)floorf((float)(int)wave_sum_u32(ok ? (unsigned)cy : 0u) * inv + 0.5f);
  const int mz = (int)floorf((float)(int)wave_sum_u32(ok ? (unsigned)cz : 0u) * inv + 0.5f);
  const bool far = ok && (abs(cx - mx) > kClassifyReach || abs(cy - my) > kClassifyReach || abs(cz - mz) > kClassifyReach);
  const unsigned outside = (unsigned)__popcll(__ballot(far));
  if (lane == 0 && lanes != 0u) {
    const int ex = x1 - x0 + 2, ey = y1 - y0 + 2, ez = z1 - z0 + 2;           // slots per axis
    const bool dflt = (ex <= kWinX - 2) & (ey <= kWinY - 2) & (ez <= kWinZ - 2);   // two slots of room for the placement
    if (!dflt) atomicAdd(&s_cnt[0], 1u);
    atomicAdd(&s_cnt[1], 1u);
    if (outside) atomicAdd(&s_cnt[2], outside);
    atomicAdd(&s_cnt[3], lanes);
    if (paired) atomicAdd(&s_cnt[4], paired);
  }
  // by how many iterations the bundle's rays left the forward march apart -- as a length: iterations * ds, in cells
  const int fki = (int)min(fk, 1u << 30);
  const int kspread = wave_max_i32(ok ? fki : 0) - wave_min_i32(ok ? fki : big);
  const bool long_ = (float)kspread * a.ds * V.inv_h >= kClassifyLongCells;
  if (lane == 0 && lanes != 0u && a.fsteps != nullptr && long_) atomicAdd(&s_cnt[6], 1u);
  __syncthreads();
  if (threadIdx.x < 7 && s_cnt[threadIdx.x] != 0u) atomicAdd(&a.select[threadIdx.x], s_cnt[threadIdx.x]);
}

#ifndef DRRT_ANCHOR_SHIFT
#define DRRT_ANCHOR_SHIFT 0.35f   // how far the window is pushed towards the direction of travel when it is anchored (0.5 = all of it ahead);
                                  // measured 256^3 / 1M rays, same box: 0.30 -> 4.85 ms, 0.35 -> 4.85, 0.40 -> 5.78 (trailing lanes miss), 0.45 -> 5.90
#endif
#ifndef DRRT_ADJ_WAVES
#define DRRT_ADJ_WAVES 5     // 5 waves per SIMD: caps the kernel at 96 VGPRs (it sits right at that edge); LDS allows 5 blocks per CU too
                             // (4 -> 4.89 ms, 5 -> 4.85, 6 -> 5.19 on the final kernel)
#endif
// PAIR: gather from the pair copy of the grid (two 16-byte loads per cell, see gather_rows).
// When the call has a visit order the host launches this kernel AND k_backtrace_ring, and each returns at once unless
// a.select picks it (k_bundle_classify decides on the device, from how the 64-ray bundles sit at their start, without a
// host round trip).  (Round 2's run-time-sized box windows -- a DYN instantiation of this kernel -- were replaced by the
// ring kernel in round 3 and are gone.)
// MODE: 0 = backtrace, 1 = backtrace_sdf (the ray also ends where the sdf sample turns non-negative, :488-497; the sdf
//       taps ride along with the grid's taps).
// CHUNK: the resumable instantiation behind drrt_backtrace_chunk_f32 (depth-chunked adjoint for the multi-GPU slab reduce,
//       DESIGN.md section 7): the launch marches a.max_steps iterations of every ray, starting from the exit rays or from
//       the state the previous chunk left in a.chunk_state (12 floats + a flag word per visit slot, SoA), hands every
//       accumulator over and flushes every window at its end, saves the state, and reduces the bounding box of the positions
//       and velocities of the rays that are still marching into a.chunk_progress.  Same arithmetic, same contributions;
//       only the order in which they reach the grid differs from the one-launch march.
// DBG: the instantiation with the event counters of DRRT_FLAG_DEBUG_COUNTERS (a.dbg), backtrace only.
template <bool DBG, bool PAIR, int MODE = 0, bool CHUNK = false>
__global__ void __launch_bounds__(kAdjBlock, DRRT_ADJ_WAVES) k_backtrace_flat(BackArgs a) {
  if (a.select != nullptr && bundles_want_ring(a.select)) return;
  constexpr int kSlots = kWinFloats;
  __shared__ win_t s_win[kAdjWavesPerBlock][kSlots];
  const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
  win_t* win = s_win[wid];
  for (int k = lane; k < kSlots; k += kWave) win[k] = (win_t)0;
  wave_lds_fence();

  const Vol& V = a.vol;
  const size_t t = (size_t)xcd_block(blockIdx.x, gridDim.x, a.xcd_order ? DRRT_FLAT_XCD_MODE : kXcdOff) * kAdjBlock + threadIdx.x;
  AdjState s;
  s.x = s.y = s.z = s.vx = s.vy = s.vz = s.lx = s.ly = s.lz = s.mx = s.my = s.mz = 0.f;
  s.active = false; s.outside = false;
  size_t i;
  const bool resume = CHUNK && a.chunk_resume != 0;
  if (resume) {                                                // continue where the previous chunk stopped
    const size_t S = a.chunk_stride;
    const float* cs = a.chunk_state + t;
    const unsigned fl = __float_as_uint(cs[12 * S]);
    s.x = cs[0]; s.y = cs[S]; s.z = cs[2 * S]; s.vx = cs[3 * S]; s.vy = cs[4 * S]; s.vz = cs[5 * S];
    s.lx = cs[6 * S]; s.ly = cs[7 * S]; s.lz = cs[8 * S]; s.mx = cs[9 * S]; s.my = cs[10 * S]; s.mz = cs[11 * S];
    s.active = (fl & 1u) != 0u; s.outside = (fl & 2u) != 0u;
  } else if (ray_index(a.perm, t, a.n, i)) {
    Ray3 p = ld3(a.xt, i, a.io_half, &a.vol, RAY_POS), u = ld3(a.vt, i, a.io_half, &a.vol, RAY_VEL), gxv = ld3(a.dx, i, a.io_half), gvv = ld3(a.dv, i, a.io_half);
    s.x = p.x; s.y = p.y; s.z = p.z; s.vx = u.x; s.vy = u.y; s.vz = u.z;
    adj_init(V, a.ds, gxv.x, gxv.y, gxv.z, gvv.x, gvv.y, gvv.z, s);
    if (MODE == 1 && s.active) {                                            // src/tracer.cpp:476-477
      const Cell c0 = locate(V, s.x, s.y, s.z);
      s.outside = interp<false>(fetch(a.sdf, c0), c0.wx, c0.wy, c0.wz).n >= 0.f;
    }
  }
  WinOrg W;                                                    // the wave's window (wave-uniform)
  W.ox = W.oy = W.oz = -(1 << 28);                             // far away = nothing is inside
  // the cell the ray stands on, located IN PLACE: flat index and coordinates of corner 000, in-cell fractions, window slot.
  // A boundary cell's clamp offsets are not carried: the boundary branch at the top of the step re-derives them from the
  // position (locate()).  The cell's predicates live in the two integers their consumers compare anyway, not in flags:
  //   strictly interior  <=>  tbase >= 0   (the lane holds the cell's taps, gathered ahead); a boundary cell has
  //   tbase = kEdge when it is regular all the same and kClamped when it is not, which is how step_locate reports the new
  //   cell's regularity to the leave
  //   regular (no clamped neighbour)  <=>  lidx > kIrregular;  lidx >= 0: window slot, kMiss: regular, outside the window
  //   (a miss votes for a re-anchor)
  //   still marching  <=>  lidx > kEnded: the loop's own copy of s.active (a ray that has ended, or a slot without a ray), so
  //   that the loop exit, the vote and the lane body's mask are compares of the one integer and no flag crosses the back edge
  constexpr int kMiss = -1, kIrregular = -2, kEnded = -3;
  constexpr int kNoFace = -(1 << 20);                        // no window slot is that far below kMiss
  int base = 0, ix = 0, iy = 0, iz = 0;
  float wx = 0.f, wy = 0.f, wz = 0.f;
  int lidx = kEnded;
  f4 q0 = f4{0.f, 0.f, 0.f, 0.f}, q1 = q0;                   // the taps, as gathered (gather_rows)
  constexpr int kClamped = -1, kEdge = -2;
  int tbase = kClamped;                                      // cell whose taps the lane holds (negative: none)
  Taps st;                                                   // MODE 1: the sdf taps of that cell, gathered with them
  st.a = st.b = st.e = st.f = f2{0.f, 0.f};
  f2 p00 = f2{0.f, 0.f}, p10 = p00, p01 = p00, p11 = p00;   // accumulators of the cell: x-pairs at (y0,z0) (y1,z0) (y0,z1) (y1,z1)
  const TapRows R = tap_rows<PAIR>(V);                       // wave-uniform row pointers + ONE 32-bit byte offset per lane
  // step to the next sample (:420), locate its cell in place and issue its gather unless the lane holds those taps
  auto step_locate = [&](int& nbase, bool move = true) {     // move = false: locate only (a resumed ray)
    if (move) { s.x = fmaf(-a.ds, s.vx, s.x); s.y = fmaf(-a.ds, s.vy, s.y); s.z = fmaf(-a.ds, s.vz, s.z); }
    const float fx = s.x * V.inv_h, fy = s.y * V.inv_h, fz = s.z * V.inv_h;
    ix = cvt_floor_i32(fx); iy = cvt_floor_i32(fy); iz = cvt_floor_i32(fz);
    const bool interior = (((unsigned)ix - 1u) < V.lx) & (((unsigned)iy - 1u) < V.ly) & (((unsigned)iz - 1u) < V.lz);
    if (interior) {
      // v_fract == f - floor(f) bit for bit for the non-negative coordinates of an interior cell
      wx = __builtin_amdgcn_fractf(fx); wy = __builtin_amdgcn_fractf(fy); wz = __builtin_amdgcn_fractf(fz);
      nbase = mad24(iz, V.sz, mad24(iy, V.sy, ix));
      if (nbase != tbase) {
        __builtin_assume(nbase >= 0 && nbase < (1 << 29));
        gather_rows<PAIR>(R, tap_offset<PAIR>(nbase), q0, q1);
        if (MODE == 1) {                                   // the sdf taps of the same cell ride along (src/tracer.cpp:488-497 reads them every step)
          const float* sp = a.sdf + (unsigned)nbase;
          st.a = ld_pair(sp); st.b = ld_pair(sp + V.sy); st.e = ld_pair(sp + V.sz); st.f = ld_pair(sp + V.sz + V.sy);
        }
        tbase = nbase;
      }
    } else {
      const Cell cb = locate(V, s.x, s.y, s.z);
      wx = cb.wx; wy = cb.wy; wz = cb.wz; ix = cb.ix; iy = cb.iy; iz = cb.iz; nbase = cb.base;
      tbase = ((cb.ox == 1) & (cb.oy == V.sy) & (cb.oz == V.sz)) ? kEdge : kClamped;
    }
  };
  if (s.active) {
    int nbase;
    if (resume) step_locate(nbase, false);                   // the saved position IS the next sample
    else        step_locate(nbase);                          // first sample
    base = nbase;
    lidx = tbase != kClamped ? kMiss : kIrregular;           // no window yet
  }
  unsigned planes = 0u;                                      // z-planes of the window the lane has held a slot in since the last flush (win_index)
  int cooldown = 0;                                          // wave-uniform (a scalar register)
  unsigned steps = 0;
  unsigned n_flush = 0;
  // CHUNK: bounding box of the samples this launch contributes at (which voxels it can have touched)
  float bx0 = 3.0e38f, by0 = 3.0e38f, bz0 = 3.0e38f, bx1 = -3.0e38f, by1 = -3.0e38f, bz1 = -3.0e38f;
  // event counters of the debug instantiation (a.dbg): [4] one-face leaves handed to the window, [5] of those, lanes that
  // issued the LDS adds after the pair / quad pre-reduction, [6] one-face leaves that went to global atomics (cell outside
  // the window), [7] leaves that handed over all eight corners, [8] wave-steps, [9] wave-steps with leaves across >= 2 axes,
  // [15] ray-steps in clamped cells (splat straight to the grid)
  unsigned ev_face = 0, ev_add = 0, ev_glob = 0, ev_all8 = 0, ev_wsteps = 0, ev_multi = 0, ev_clamp = 0;

#define WSY kWinSY
#define WSZ kWinSZ
#define WIN_INDEX(cx, cy, cz) win_index(W.ox, W.oy, W.oz, cx, cy, cz, planes)
    for (int it = 0; it < a.max_steps; ++it) {
      const bool marching = lidx > kEnded;
      if (__builtin_amdgcn_ballot_w64(marching) == 0ull) break;                 // wave-uniform exit; the mask is the lane body's too
      // ---- (re-)anchor the window around the cells the rays stand on (wave-uniform branch) ----
      if (cooldown != 0) {
        --cooldown;
      } else if (__builtin_amdgcn_ballot_w64(lidx == kMiss) != 0ull) {
        const unsigned dirty = wave_or_u32(planes);
        if (dirty != 0u) {
          win_flush(win, W.ox, W.oy, W.oz, a.grad, V, lane, dirty);
          planes = 0u; ++n_flush;
        }
        const bool ok = lidx > kIrregular;                                      // marching, in a regular cell
        const unsigned long long cm = __ballot(ok);
        const int first = __ffsll((long long)cm) - 1, last = 63 - __clzll((long long)cm);
        int ref = (first + last) >> 1;
        if (!((cm >> ref) & 1ull)) ref = first;
        const int rx = __shfl(ix, ref, kWave), ry = __shfl(iy, ref, kWave), rz = __shfl(iz, ref, kWave);
        // backward direction of travel of the reference lane
        const float dx_ = -__shfl(s.vx, ref, kWave), dy_ = -__shfl(s.vy, ref, kWave), dz_ = -__shfl(s.vz, ref, kWave);
        const float inv_dm = __builtin_amdgcn_rcpf(fmaxf(fmaxf(fabsf(dx_), fabsf(dy_)), fmaxf(fabsf(dz_), 1e-30f)));   // placement only
        {
          // default: a kWin^3 window around the median lane's cell, shifted towards the direction of travel
          const float fx = 0.5f - DRRT_ANCHOR_SHIFT * (dx_ * inv_dm), fy = 0.5f - DRRT_ANCHOR_SHIFT * (dy_ * inv_dm), fz = 0.5f - DRRT_ANCHOR_SHIFT * (dz_ * inv_dm);
          int ox = rx - (int)(fx * (float)(kWinX - 2));
          int oy = ry - (int)(fy * (float)(kWinY - 2));
          int oz = rz - (int)(fz * (float)(kWinZ - 2));
          ox = max(0, min(ox, V.W - kWinX)); oy = max(0, min(oy, V.H - kWinY)); oz = max(0, min(oz, V.D - kWinZ));
          W.ox = __builtin_amdgcn_readfirstlane(ox); W.oy = __builtin_amdgcn_readfirstlane(oy);
          W.oz = __builtin_amdgcn_readfirstlane(oz);
          if (ok) lidx = WIN_INDEX(ix, iy, iz);                                 // every marching lane's cell, in the new window
        }
        cooldown = (__builtin_amdgcn_ballot_w64(lidx == kMiss) != 0ull) ? 4 : 0;   // incoherent wave: do not thrash
      }
      if (marching) {
        const bool interior = tbase >= 0, regular = lidx > kIrregular;
        if (!interior) taps_set<PAIR>(fetch(V.data, locate(V, s.x, s.y, s.z)), q0, q1);   // boundary cell (clamped neighbours): fetched here, not ahead
        Cell c;                                              // what adj_sample reads of the cell: fractions, interior
        c.base = 0; c.ix = c.iy = c.iz = 0; c.ox = c.oy = c.oz = 0;
        c.wx = wx; c.wy = wy; c.wz = wz; c.interior = interior;
        if (MODE == 1 && !interior) c = locate(V, s.x, s.y, s.z);   // boundary cell: adj_sample<1> gathers its sdf taps itself
        const float px = s.x, py = s.y, pz = s.z;            // position of this sample (the clamped splat re-locates it)
        AdjSample m;
        if (!adj_sample_st<MODE>(V, a.sdf, a.ds, s, c, taps_of<PAIR>(q0, q1), m, st, MODE == 1 && interior)) {
          // the ray has ended (:426-428): it contributes nothing here; hand over what its cell has accumulated
          if (regular) flat_emit8<true>(win, WSY, WSZ, a.grad, V.sy, V.sz, lidx, base, p00, p10, p01, p11);
          lidx = kEnded;
        } else {
          ++steps;
          if (CHUNK) { bx0 = fminf(bx0, px); by0 = fminf(by0, py); bz0 = fminf(bz0, pz); bx1 = fmaxf(bx1, px); by1 = fmaxf(by1, py); bz1 = fmaxf(bz1, pz); }
          {
            // first half of adj_contrib: the 8 splat weights (they need the in-cell fractions of THIS cell)
            const float dn = dot3(s.mx, s.my, s.mz, m.gx, m.gy, m.gz);                            // :430
            const float nds = (m.n * a.ds) * a.grad_scale;
            if (regular) {
              const CornerPairs cp = splat_weights_pk(wx, wy, wz, dn * a.ds, nds * s.mx, nds * s.my, nds * s.mz);   // :431-432
              p00 += cp.c00; p10 += cp.c10; p01 += cp.c01; p11 += cp.c11;
            } else {
              // clamped boundary cell: taps coincide; straight to the grid
              const Cell cb = locate(V, px, py, pz);
              const Corners w = splat_weights(cb.wx, cb.wy, cb.wz, dn * a.ds, nds * s.mx, nds * s.my, nds * s.mz);
              const unsigned g = (unsigned)cb.base, gy = g + (unsigned)cb.oy, gz = g + (unsigned)cb.oz, gzy = gz + (unsigned)cb.oy;
              atomic_add_f32_at(a.grad, g, w.c000);          atomic_add_f32_at(a.grad, g + (unsigned)cb.ox, w.c100);
              atomic_add_f32_at(a.grad, gy, w.c010);         atomic_add_f32_at(a.grad, gy + (unsigned)cb.ox, w.c110);
              atomic_add_f32_at(a.grad, gz, w.c001);         atomic_add_f32_at(a.grad, gz + (unsigned)cb.ox, w.c101);
              atomic_add_f32_at(a.grad, gzy, w.c011);        atomic_add_f32_at(a.grad, gzy + (unsigned)cb.ox, w.c111);
              if (DBG && a.dbg) ++ev_clamp;
            }
            // step to the next sample and issue its gather (it + 1 == max_steps: located and fetched, never used)
            const int old_base = base;
            int nbase;
            step_locate(nbase);
            // second half of adj_contrib: lambda / mu (:434-435)
            const float hxy = m.hxy * V.inv_h2, hxz = m.hxz * V.inv_h2, hyz = m.hyz * V.inv_h2;
            const float hmx = fmaf(hxz, s.mz, hxy * s.my);
            const float hmy = fmaf(hyz, s.mz, hxy * s.mx);
            const float hmz = fmaf(hyz, s.my, hxz * s.mx);
            s.lx = fmaf(a.ds, fmaf(dn, m.gx, m.n * hmx), s.lx);
            s.ly = fmaf(a.ds, fmaf(dn, m.gy, m.n * hmy), s.ly);
            s.lz = fmaf(a.ds, fmaf(dn, m.gz, m.n * hmz), s.lz);
            s.mx = fmaf(a.ds, s.lx, s.mx); s.my = fmaf(a.ds, s.ly, s.my); s.mz = fmaf(a.ds, s.lz, s.mz);
            // ---- the ray leaves its cell ----
            // Two regions, one behind the other, both tested on integers the lane holds anyway.  The hot one: both cells regular
            // and the flat index moved -- one face crossed, unless no case below matches.  The cold one: whatever else changes
            // the cell (into or out of a clamped cell, which can share its flat index with its regular neighbour; a jump over
            // more than one face).  A ray that stays in its cell (d == 0 with the regularity unchanged) enters neither.
            const int d = nbase - old_base;
            const bool nregular = tbase != kClamped;
            const bool left = (d != 0) | (nregular != regular);
            base = nbase;
            int key = kNoFace;                               // the face (win_face_key); a case of the hot region sets it
            if (regular & nregular & (d != 0)) {
              // One face crossed (the flat index moved by one stride): emit the face left behind, carry the shared one.  Six
              // cases, axis and direction compile-time in each: a case copies the four emitted corners out (e0..e3, in (p, q)
              // in-face order), moves the carried ones once, and names the face's window slot and strides; ONE emission follows
              // the cases (wave-steps whose lanes leave across two or more axes are the common kind -- over half of the
              // headline's -- so an emission per case would run twice there).
              // AX: 0 = x, 1 = y, 2 = z; FWD: towards the higher index.
              float e0, e1, e2, e3;
              int lp, lq;                                    // window strides of p and q (slots)
              auto face = [&](auto AX, auto FWD) {
                constexpr int ax = decltype(AX)::value;
                constexpr bool fwd = decltype(FWD)::value;
                constexpr f2 zero = f2{0.f, 0.f};
                asm volatile("");                            // keeps the case's moves under the case's test (not speculated above it)
                key = lidx + win_face_key(fwd ? 0 : (ax == 0 ? 1 : (ax == 1 ? WSY : WSZ)), ax);   // lidx < 2^16: no carry into the axis
                lp = ax == 0 ? WSY : 1; lq = ax == 2 ? WSY : WSZ;
                if (ax == 0) {
                  e0 = fwd ? p00.x : p00.y; e1 = fwd ? p10.x : p10.y; e2 = fwd ? p01.x : p01.y; e3 = fwd ? p11.x : p11.y;
                  p00 = fwd ? f2{p00.y, 0.f} : f2{0.f, p00.x}; p10 = fwd ? f2{p10.y, 0.f} : f2{0.f, p10.x};
                  p01 = fwd ? f2{p01.y, 0.f} : f2{0.f, p01.x}; p11 = fwd ? f2{p11.y, 0.f} : f2{0.f, p11.x};
                } else if (ax == 1) {
                  const f2 ea = fwd ? p00 : p10, eb = fwd ? p01 : p11;
                  e0 = ea.x; e1 = ea.y; e2 = eb.x; e3 = eb.y;
                  if (fwd) { p00 = p10; p01 = p11; p10 = p11 = zero; } else { p10 = p00; p11 = p01; p00 = p01 = zero; }
                } else {
                  const f2 ea = fwd ? p00 : p01, eb = fwd ? p10 : p11;
                  e0 = ea.x; e1 = ea.y; e2 = eb.x; e3 = eb.y;
                  if (fwd) { p00 = p01; p10 = p11; p01 = p11 = zero; } else { p01 = p00; p11 = p10; p00 = p10 = zero; }
                }
              };
              using std::integral_constant;
              if (DBG && a.dbg) {
                const bool ax = (d == 1) | (d == -1), ay = (d == V.sy) | (d == -V.sy), az = (d == V.sz) | (d == -V.sz);
                if (ax | ay | az) {
                  const int nax = (__ballot(ax) != 0ull) + (__ballot(ay) != 0ull) + (__ballot(az) != 0ull);
                  if (lane == __ffsll((long long)__ballot(true)) - 1) ev_multi += nax >= 2;
                }
              }
              // flat, mutually exclusive tests (a regular cell has 1 < sy < sz), not an else-chain: each case is one
              // predicated region
              const bool yp = d == V.sy, ym = d == -V.sy, zp = d == V.sz, zm = d == -V.sz, xp = d == 1, xm = d == -1;
              if (yp) face(integral_constant<int, 1>{}, integral_constant<bool, true>{});
              if (ym) face(integral_constant<int, 1>{}, integral_constant<bool, false>{});
              if (zp) face(integral_constant<int, 2>{}, integral_constant<bool, true>{});
              if (zm) face(integral_constant<int, 2>{}, integral_constant<bool, false>{});
              if (xp) face(integral_constant<int, 0>{}, integral_constant<bool, true>{});
              if (xm) face(integral_constant<int, 0>{}, integral_constant<bool, false>{});
              if (key != kNoFace) {
                if (lidx >= 0) {
                  const bool add = win_emit4(win, key, lp, lq, e0, e1, e2, e3);
                  if (DBG && a.dbg) { ++ev_face; ev_add += add; }
                } else {
                  // the cell lies outside the window: straight to the grid.  |d| is the grid stride of the axis crossed, which
                  // names the strides of p and q; a face left behind in the negative direction is the cell's far one, |d| on.
                  if (DBG && a.dbg) ++ev_glob;
                  const int ad = abs(d);
                  const unsigned gp = ad == 1 ? (unsigned)V.sy : 1u, gq = ad == V.sz ? (unsigned)V.sy : (unsigned)V.sz;
                  const unsigned g = (unsigned)(old_base + max(-d, 0)), gqq = g + gq;
                  atomic_add_f32_at(a.grad, g, e0);   atomic_add_f32_at(a.grad, g + gp, e1);
                  atomic_add_f32_at(a.grad, gqq, e2); atomic_add_f32_at(a.grad, gqq + gp, e3);
                }
              }
            }
            if (left) {
              if (regular & (key == kNoFace)) {
                // jump over more than one face, or into a clamped cell: hand over all eight
                asm volatile("");                            // cold: stays under its test
                if (DBG && a.dbg) ++ev_all8;
                // (no quad pre-reduction here: two-face crossings are rarely shared by a quad -- 4.87 -> 4.81 ms without it)
                flat_emit8<false>(win, WSY, WSZ, a.grad, V.sy, V.sz, lidx, old_base, p00, p10, p01, p11);
                p00 = p10 = p01 = p11 = f2{0.f, 0.f};
              }
              lidx = nregular ? WIN_INDEX(ix, iy, iz) : kIrregular;
            }
          }
        }
      }
      if (DBG && a.dbg) ev_wsteps += lane == 0;
    }
  // rays still marching when max_steps ran out keep what their cell has accumulated: hand it over
  if (lidx > kIrregular) flat_emit8(win, WSY, WSZ, a.grad, V.sy, V.sz, lidx, base, p00, p10, p01, p11);
#undef WSY
#undef WSZ
#undef WIN_INDEX
  const unsigned dirty = wave_or_u32(planes);
  if (dirty != 0u) {
    win_flush(win, W.ox, W.oy, W.oz, a.grad, V, lane, dirty);
    ++n_flush;
  }
  if (CHUNK) {
    s.active = lidx > kEnded;
    // the state the next chunk resumes from (position = the next sample, already stepped to), and where the rays that are
    // still marching stand and head: bounding boxes of their positions [0..5] and velocities [6..11] as order-preserving
    // integer keys (min: 0..2 / 6..8, max: 3..5 / 9..11), [12] their number; [13..18] bounding box of the samples taken
    const size_t S = a.chunk_stride;
    float* cs = a.chunk_state + t;
    cs[0] = s.x; cs[S] = s.y; cs[2 * S] = s.z; cs[3 * S] = s.vx; cs[4 * S] = s.vy; cs[5 * S] = s.vz;
    cs[6 * S] = s.lx; cs[7 * S] = s.ly; cs[8 * S] = s.lz; cs[9 * S] = s.mx; cs[10 * S] = s.my; cs[11 * S] = s.mz;
    cs[12 * S] = __uint_as_float((s.active ? 1u : 0u) | (s.outside ? 2u : 0u));
    if (a.chunk_progress != nullptr && __any(s.active)) {
      const float vals[6] = {s.x, s.y, s.z, s.vx, s.vy, s.vz};
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        const int key = float_order_key(vals[k]);
        const int lo = wave_min_i32(s.active ? key : 0x7fffffff), hi = wave_max_i32(s.active ? key : (int)0x80000000);
        if (lane == 0) { atomicMin(&a.chunk_progress[(k / 3) * 6 + (k % 3)], lo); atomicMax(&a.chunk_progress[(k / 3) * 6 + 3 + (k % 3)], hi); }
      }
      const unsigned cnt = (unsigned)__popcll(__ballot(s.active));
      if (lane == 0) atomicAdd((unsigned*)&a.chunk_progress[12], cnt);
    }
    if (a.chunk_progress != nullptr && __any(steps != 0u)) {       // [13..15] min, [16..18] max of the samples of THIS chunk
      const float lo[3] = {bx0, by0, bz0}, hi[3] = {bx1, by1, bz1};
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const int l = wave_min_i32(float_order_key(lo[k])), h = wave_max_i32(float_order_key(hi[k]));
        if (lane == 0) { atomicMin(&a.chunk_progress[13 + k], l); atomicMax(&a.chunk_progress[16 + k], h); }
      }
    }
  }
  if (DBG && a.dbg) {
    if (lane == 0) atomicAdd(&a.dbg[0], (unsigned long long)n_flush);
    if (ev_face) atomicAdd(&a.dbg[4], (unsigned long long)ev_face);
    if (ev_add) atomicAdd(&a.dbg[5], (unsigned long long)ev_add);
    if (ev_glob) atomicAdd(&a.dbg[6], (unsigned long long)ev_glob);
    if (ev_all8) atomicAdd(&a.dbg[7], (unsigned long long)ev_all8);
    if (ev_wsteps) atomicAdd(&a.dbg[8], (unsigned long long)ev_wsteps);
    if (ev_multi) atomicAdd(&a.dbg[9], (unsigned long long)ev_multi);
    if (ev_clamp) atomicAdd(&a.dbg[15], (unsigned long long)ev_clamp);
  }
  block_stats<kAdjBlock>(a.stats, steps, 0u);
}

// ---- launchers ----------------------------------------------------------------------------------
void launch_backtrace_direct(int mode, const BackArgs& a, hipStream_t s) {
  const dim3 g(grid_for(a.n)), b(kBlock);
  if (mode == 1) hipLaunchKernelGGL(k_backtrace_direct<1>, g, b, 0, s, a);
  else           hipLaunchKernelGGL(k_backtrace_direct<0>, g, b, 0, s, a);
}
void launch_bundle_classify(const BackArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_bundle_classify, dim3((grid_for(a.n) + kClassifyStride - 1) / kClassifyStride), dim3(kBlock), 0, s, a);
}
// PAIR follows the call's pair grid; the other parameters are the launcher's choice
template <bool DBG, int MODE, bool CHUNK>
static void launch_flat(const BackArgs& a, hipStream_t s) {
  const dim3 g(adj_grid_for(a.n)), b(kAdjBlock);
  if (a.vol.pair != nullptr) hipLaunchKernelGGL((k_backtrace_flat<DBG, true, MODE, CHUNK>), g, b, 0, s, a);
  else                       hipLaunchKernelGGL((k_backtrace_flat<DBG, false, MODE, CHUNK>), g, b, 0, s, a);
}
void launch_backtrace_box(int mode, bool dbg, const BackArgs& a, hipStream_t s) {
  if (a.chunk_state != nullptr) launch_flat<false, 0, true>(a, s);     // resumable march (drrt_backtrace_chunk_f32): backtrace only
  else if (mode == 1)           launch_flat<false, 1, false>(a, s);    // the counter instantiation exists for backtrace only
  else if (dbg)                 launch_flat<true, 0, false>(a, s);
  else                          launch_flat<false, 0, false>(a, s);
}

}  // namespace drrt
