/*
 * drrt_hip.h -- C ABI of the MI355X-native eikonal ray-march library (libdrrt_hip.so).
 *
 * Drop-in boundary for the hot path of ArjunTeh/AdjointNonlinearRayTracing: one entry
 * point per method of the reference's `drrt.TracerC` pybind class
 * (reference: src/drrt.cpp:47-58, declarations include/tracer.h:15-89).  Plain pointers and
 * sizes only -- no torch / enoki / pybind types.
 *
 * Conventions shared by all entry points
 *   - every array pointer is a DEVICE pointer (HIP, gfx950) unless stated otherwise;
 *   - ray arrays (pos, vel, xt, vt, dx, dv, pln_o, pln_d, target) are (n,3) row-major fp32,
 *     exactly the torch tensors the reference's core/tracer.py hands to enoki
 *     (core/tracer.py:300-301); outputs have the same layout;
 *   - `rif` / `sdf` / `grad` are flat fp32[nvox], C-order flatten of the torch (D,H,W) tensor
 *     (core/tracer.py:299); `res` is a HOST pointer to 3 ints = tuple(rif.shape), used as
 *     (width,height,depth) with flat index (z*height + y)*width + x (src/volume.cpp:134-141);
 *   - `h`, `ds` are fp32 scalars (include/tracer.h:20-21 narrows python floats to float);
 *   - calls are ASYNCHRONOUS on `stream` (a hipStream_t; NULL = the null stream) and never
 *     allocate, free or synchronise; scratch memory comes from the caller-provided workspace;
 *   - return value: DRRT_OK or a negative DRRT_ERR_*; drrt_last_error() returns the message
 *     of the last failing call on this host thread.  The three messages of the reference
 *     (src/volume.cpp:28,37,115,124) are reproduced verbatim.
 *
 * Statistics: `stats` (nullable) is a DEVICE pointer to one drrt_stats that the call zeroes and
 * fills; read it back after synchronising the stream.  `n_failed > 0` is the condition under
 * which the reference prints "failed to exit all rays" (src/tracer.cpp:89-90).
 */
#ifndef DRRT_HIP_H
#define DRRT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define DRRT_API __attribute__((visibility("default")))
#else
#define DRRT_API
#endif

#define DRRT_OK                0
#define DRRT_ERR_RES_MISMATCH (-1)  /* "Resolution doesn't match data"  (src/volume.cpp:28,37)  */
#define DRRT_ERR_BAD_RES      (-2)  /* "volume: invalid resolution!"     (src/volume.cpp:124)    */
#define DRRT_ERR_ARG          (-3)  /* null pointer / workspace too small / bad flag             */
#define DRRT_ERR_HIP          (-4)  /* a HIP runtime call failed (message carries hipGetErrorString) */

/* flags (bit-or).  Bits 32u, 0x10000u..0x100000u carried A-B switches for kernels that were removed in round 4 (LDS
 * bricks, tap-reuse variants, the round-1 forward / adjoint kernels); they are ignored now. */
#define DRRT_FLAG_NONE         0u
#define DRRT_FLAG_SORT_RAYS    1u   /* locality-sort rays by entry voxel before marching (results
                                       are written back in the caller's ray order)                */
#define DRRT_FLAG_CORRECTED_H  2u   /* adjoint only: divide the gradient-splat term by h (exact
                                       discrete adjoint).  Default = as written in the reference,
                                       which omits it (src/volume.cpp:227-243 vs :178)            */
#define DRRT_FLAG_NO_ZERO      4u   /* adjoint only: accumulate into `grad` without zeroing it
                                       first (the reference always starts from zeros,
                                       src/tracer.cpp:401-403)                                    */
#define DRRT_FLAG_DIRECT_ATOMICS 8u /* adjoint only: bypass the LDS gradient windows and issue
                                       one global atomic per tap (debug / A-B measurement)        */

#define DRRT_FLAG_PAIR_GRID    64u  /* trace / trace_pln / trace_sdf / backtrace*: build the "pair copy" of the grid in the
                                       workspace (8 B per voxel: each voxel interleaved with its +y neighbour) and
                                       fetch the 8 corners of a strictly interior cell with two 16-byte loads instead
                                       of four 8-byte ones -- the march is bound by the number of gather instructions
                                       (DESIGN.md 5.1).  Bit-identical results.  Needs a 16-byte aligned workspace of
                                       drrt_workspace_bytes_grid() bytes.  Pays off when the call does well over ~4
                                       ray-steps per voxel (the copy costs 12 B of traffic per voxel)              */
#define DRRT_FLAG_PAIR_REUSE  128u  /* with PAIR_GRID: the workspace still holds the pair copy built by the previous
                                       call (same rif contents, same n, same flags & SORT_RAYS, same workspace) --
                                       e.g. the adjoint paired with its forward: skip the rebuild                  */
#define DRRT_FLAG_QUAD_GRID  DRRT_FLAG_PAIR_GRID    /* round-1 names (the copy then held an (x,y) quad per voxel)   */
#define DRRT_FLAG_QUAD_REUSE DRRT_FLAG_PAIR_REUSE
#define DRRT_FLAG_Q16_POS_ONLY 0x200000u  /* drrt_trace_q16io / drrt_backtrace_q16io: only the POSITION arrays are q16 codes;
                                             directions and adjoint seeds are fp32 arrays (18 B per exit ray instead of 12) */
#define DRRT_FLAG_CHORD_KEY 0x800000u      /* with SORT_RAYS (A-B measurement; same results): the rounds-1/2 sort key (6-D Morton interleave of the
                                              chord end points) instead of the light-field key (direction cell + Hilbert index of the
                                              transverse offset, csrc/drrt_sort.hip) */
/* Which adjoint kernel runs (same results up to fp32 summation order).  Default: with a visit order and a
 * drrt_workspace_bytes_grid() workspace the 64-ray bundles of the call are classified on the device and either the box-window
 * kernel (compact bundles) or the ring-window kernel (sparse views, views oblique to the grid) runs; the two flags force one. */
#define DRRT_FLAG_RING_WINDOW 0x1000000u   /* backtrace, backtrace_sdf: always the ring-window kernel (k_backtrace_ring: the wave's LDS window is
                                              addressed modulo its size and follows the rays; each voxel is flushed once; honours the step hint) */
#define DRRT_FLAG_RING_SPARSE  0x4000000u  /* with RING_WINDOW (A-B): the sparse-only instantiation of the ring-window kernel (every cell
                                              leave hands over all eight corners; chosen by itself for sparse ray sets) */
#define DRRT_FLAG_RING_GENERAL 0x8000000u  /* backtrace (A-B): never the sparse-only instantiation (the per-wave dense / sparse rule only) */
#define DRRT_FLAG_RING_DIRECT  0x10000000u /* with RING_WINDOW | RING_SPARSE (A-B): the DIRECT sparse-only instantiation (every step's eight
                                              contributions straight to the window; chosen by itself when few lanes share a cell) */
#define DRRT_FLAG_STATIC_WINDOW 0x400000u  /* backtrace, backtrace_sdf: always the box-window kernel (k_backtrace_flat, compile-time 9^3 gradient
                                              windows), no per-call bundle classification */
#define DRRT_FLAG_DISPATCH_IN_ORDER 0x2000000u /* trace, trace_pln, backtrace, backtrace_sdf (A-B measurement; forward bit-identical, adjoint the same
                                         up to fp32 summation order): block b of a launch marches block b of the visit order.  Default
                                         with a visit order: each of the chip's 8 XCDs (own L2; blocks are dealt to them round-robin)
                                         takes a contiguous run of the visit order, so neighbouring bundles share one L2 */
#define DRRT_FLAG_DEBUG_COUNTERS 16u /* adjoint only (development aid): uint64 counters are
                                       written to the last 512 bytes of the workspace:
                                       [0] LDS-window flushes, [1] ray-steps accumulated through
                                       the LDS window, [2] ray-steps that fell back to global atomics
                                       ([1], [2]: unused since round 4), [3] waves of the ring-window kernel;
                                       k_backtrace_flat events: [4] one-face cell leaves handed to the
                                       window, [5] lanes of those that issued the LDS adds after the
                                       pair / quad pre-reduction, [6] one-face leaves sent to global
                                       atomics (cell outside the window), [7] leaves that handed over
                                       all eight corners, [8] wave-steps, [9] wave-steps whose one-face
                                       leaves cross two or three different axes.
                                       Bits 8..15 of `flags` (backtrace*): 0, or 1 = zero `grad` and `stats`
                                       and launch no adjoint (a known-wrong result, for the benchmark's parity
                                       test); any other value is refused with DRRT_ERR_ARG */

/* Limits (violations are refused with DRRT_ERR_ARG and a message, never truncated silently):
 *   grid      fewer than 2^29 voxels (2 GiB of fp32), each extent and res[0]*res[1] below 2^24
 *             (e.g. up to 812^3, or 4095 x 4095 x 32); res[0], res[1] >= 2 as in the reference (src/volume.cpp:123)
 *   rays      n < 2^32 per call
 *   h, ds     positive and finite
 * Non-finite ray components are tolerated: such rays march until max_steps and do not affect other rays'
 * forward results (their adjoint contributions are non-finite, as in any IEEE implementation).
 * Thread-safety: the visit-order hand-over (drrt_last_order / drrt_set_order_hint) and drrt_last_error() are
 * PER HOST THREAD (thread_local): a hint set on one thread is only seen by march calls of that thread.  The
 * profiling aid (drrt_profile_*) is process-global and not thread-safe.  trace_pln / trace_sdf called with
 * stats == NULL use one library-owned 24-byte stats block per device, shared by all streams of that device:
 * pass your own stats block when running them concurrently on several streams of one device.        */

typedef struct drrt_stats {
  unsigned long long ray_steps;  /* sum over rays of march iterations executed while the ray was live */
  unsigned long long n_failed;   /* rays still live after max_steps                                  */
  unsigned int       iters;      /* max over rays of iterations = the reference's global loop count  */
  unsigned int       reserved;
} drrt_stats;

/* Bytes of device scratch a call over `n` rays may need (0 when flags need none). */
DRRT_API size_t drrt_workspace_bytes(size_t n, unsigned flags);
/* Same, for a call on a grid of `nvox` voxels: adds the pair copy when DRRT_FLAG_PAIR_GRID is set and the
 * 512-byte counter block.  Layout: [sort buffers | trace_target state][pair copy][counters].  The one place that
 * draws and computes it, region by region, is the comment above ws_layout() in csrc/drrt_api.hip.    */
DRRT_API size_t drrt_workspace_bytes_grid(size_t n, long long nvox, unsigned flags);

/* Message of the last error on this thread ("" if none). */
DRRT_API const char* drrt_last_error(void);

/* Library / build identification: "drrt_hip <abi> gfx950 src:<12 hex digits>", the digest being that of the sources
 * the library was built from (csrc/Makefile); profiles/ *_pmc.json record it so that a stale profile is detectable. */
DRRT_API const char* drrt_version(void);

/* ---- visit order hand-over (optimisation hint; with a valid permutation results do not depend on it) ---
 * A sorted call (DRRT_FLAG_SORT_RAYS) leaves the permutation it used -- n uint32 ray indices, in
 * visit order -- inside the caller's workspace; drrt_last_order() returns that device pointer
 * (valid until the workspace is overwritten) and its length.
 * drrt_set_order_hint(order, n) makes the NEXT march call on this host thread visit its rays in
 * `order` instead of sorting.  That call consumes the hint as its first action -- also when it then fails
 * validation or ignores the hint -- so a hint never outlives one call.  It is ignored when its ray count
 * differs, by drrt_trace_target_f32 (whose state buffer would overlay an order living in the same workspace)
 * and by the cable calls.  `order` must stay valid and unmodified until the call's kernels have finished;
 * entries are range-checked on the device: an entry >= n leaves that slot's ray unvisited (its outputs
 * unwritten) but is never dereferenced.  With a valid permutation results do not depend on the hint.
 * Intended pairing: the adjoint of a forward march (core/tracer.py:294-335 couples them through
 * ctx.outx/ctx.outv) reuses the forward's order -- rays that entered the grid together stay
 * together through any smooth medium, which keeps each wave inside its LDS gradient window even
 * where the exit rays alone (a focus, a caustic) say nothing about the bundle they came from.   */
DRRT_API const uint32_t* drrt_last_order(size_t* n_out);
DRRT_API void drrt_set_order_hint(const uint32_t* order, size_t n);
/* Length of the hint currently armed on this host thread -- the order hint's, or the step hint's (below) when only
 * that one is armed; 0 = neither: lets a binding assert that no hint survives a call. */
DRRT_API size_t drrt_order_hint_pending(void);
/* ---- step hint (optimisation hint of the same kind; results do not depend on it) ---------------------------------
 * A forward march (drrt_trace_f32 / _f16io / _q16io / drrt_trace_pln_f32 called with a workspace) leaves the number of
 * march iterations of every ray -- n uint32, caller ray order -- in the workspace; drrt_last_steps() returns that
 * device pointer (valid until the workspace is overwritten; NULL when the last forward call on this thread wrote none).
 * drrt_set_step_hint(steps, n) hands them to the NEXT drrt_backtrace_* call on this host thread (consumed at its entry,
 * like the order hint; ignored when n differs): the rays of a wave then start the adjoint on the forward march's clock
 * (a ray that left d iterations before the last one of its wave starts d iterations later, d <= 96), so a bundle that
 * was compact in the forward march is compact in the adjoint too, whatever the exit face.  Only WHEN a lane does its
 * k-th step changes; every ray still gets its max_steps iterations (src/tracer.cpp:417).  Wrong counts cost speed only. */
DRRT_API const uint32_t* drrt_last_steps(size_t* n_out);
DRRT_API void drrt_set_step_hint(const uint32_t* steps, size_t n);

/* Which adjoint kernel ran, and why: a DEVICE pointer to the four counters of the bundle classification of the last
 * drrt_backtrace_* / drrt_backtrace_sdf_f32 call on this host thread that classified its bundles (it lies in that call's
 * workspace: valid while the workspace is, read it after synchronising the stream), or NULL when that call did not (no visit
 * order, a forced kernel, a workspace without the counter block).  Over every 16th block of 64-ray bundles:
 *   [0] bundles whose start cells do not fit the box window, [1] bundles looked at,
 *   [2] lanes whose start cell lies more than 3 cells from their bundle's mean cell, [3] lanes looked at (diagnostic),
 *   [4] lanes whose pair partner (lane ^ 1) starts in the same cell (diagnostic), [5] non-zero when the call pinned the
 *   general instantiation of the ring kernel, [6] bundles whose rays' forward iteration counts (step hint) spread over 12
 *   cells of travel or more (spread * ds / h >= 12: 24 iterations at ds = h / 2; 0 without a hint) (8 ints in all; [7] unused).
 * The ring-window kernel runs when [0] * 100 >= [1] * drrt_ring_threshold_pct() (the library's compile-time threshold, 20 in
 * the product build) or when [6] * 1000 >= [1] * drrt_ring_long_threshold_permille() (75: the box-window kernel does not use
 * the step hint, so rays that left the forward march that far apart run spread along their path beyond its window); its
 * sparse-only instantiation (fixed-point window) unless [5] is set -- the one that hands over per step ("direct") when
 * [4] * 100 < [3] * drrt_ring_direct_threshold_pct() (40: few lanes share a cell), else the one that hands over per cell.
 * Calibration:
 * csrc/drrt_march.h, bundles_want_ring / bundles_long / bundles_want_sparse.  The counters describe the START cells of the
 * bundles (the exit rays as given), not where the step hint's delays put the lanes later on. */
DRRT_API const unsigned* drrt_last_bundle_counters(void);
DRRT_API int drrt_ring_threshold_pct(void);
DRRT_API int drrt_ring_long_threshold_permille(void);   /* ring kernel also when counters [6] * 1000 >= [1] * this */
DRRT_API int drrt_ring_direct_threshold_pct(void);      /* its direct sparse-only instantiation when counters [4] * 100 < [3] * this */

/* ---- 16-bit ray state "q16" (BASELINE.json config 5: "fp16 ray state + fp32 adjoint accumulate") -----------------
 * The reference is fp32-only (include/types.h:36-46).  IEEE half keeps 11 significant bits wherever the value is:
 * a position near 1.0 is rounded to 2^-11 = 1/8 voxel of a 256^3 grid, which changes the adjoint trajectories
 * enough to move the gradient by 26 % rel-L2 (tests/test_baseline_configs.py, round 1).  The q16 formats spend the
 * same 6 bytes per 3-vector where a march needs them:
 *   positions   unsigned 16-bit codes c: p = q_min + c * q_step, over [-E/16, E + E/16] with E = max((res-1)*h);
 *               q_step = 1.125 E / 65535 (= h/228 at 256^3); positions outside the range SATURATE
 *   directions  signed 16-bit fixed point c: v = c * 2^-14 (range [-2, 2): |v| = n < 2); saturating
 *   seeds       dx, dv of the adjoint: IEEE half (relative precision is what a seed needs; scale them into range)
 * drrt_trace_q16io / drrt_backtrace_q16io widen exactly on load, march / accumulate in fp32 and round outputs once:
 *   drrt_trace_q16io(encode(x), encode(v)) == encode(drrt_trace_f32(decode(encode(x)), decode(encode(v)))) bit for bit.
 * drrt_q16_encode / drrt_q16_decode are the device-side conversions (either array may be NULL);
 * drrt_q16_params returns {q_min, q_step, 2^-14} for a grid (host pointers).
 * Tolerance (stated, no reference counterpart; tests/test_baseline_configs.py, 256^3 / 512 steps / 512^2 sensor / 262k
 * rays): the gradient splat of a sample jumps by one voxel when the sample changes cell, and a perturbation of d voxels
 * of the exit state makes a fraction ~d of the samples do so, so two SPARSE gradient grids (a handful of samples per
 * voxel) differ by ~sqrt(d) rel-L2 whatever the storage format: IEEE half (d ~ 1/8) 0.26, q16 (d ~ 2e-3) 0.055 raw and
 * 0.013 after a 3^3 box filter (the scale an optimiser sees); q16 positions with fp32 directions
 * (DRRT_FLAG_Q16_POS_ONLY) 0.050 / 0.012.  Tested bounds: 0.1 raw, 2e-2 filtered.                                      */
DRRT_API int drrt_q16_params(const int res[3], float h, float out[3]);
DRRT_API int drrt_q16_encode(const int res[3], float h, size_t n, const float* pos, const float* vel,
                    void* pos_q, void* vel_q, void* stream);
DRRT_API int drrt_q16_decode(const int res[3], float h, size_t n, const void* pos_q, const void* vel_q,
                    float* pos, float* vel, void* stream);
DRRT_API int drrt_trace_q16io(const float* rif, long long nvox, const int res[3], size_t n,
                     const void* pos_q, const void* vel_q, float h, float ds,
                     void* xt_q, void* vt_q,
                     drrt_stats* stats, void* workspace, size_t workspace_bytes,
                     unsigned flags, void* stream);
DRRT_API int drrt_backtrace_q16io(const float* rif, long long nvox, const int res[3], size_t n,
                         const void* xt_q, const void* vt_q, const void* dx_h, const void* dv_h,
                         float h, float ds, float* grad,
                         drrt_stats* stats, void* workspace, size_t workspace_bytes,
                         unsigned flags, void* stream);

/* ---- forward marches ------------------------------------------------------------------- */

/* Tracer<false,true>::trace  -- src/tracer.cpp:35-100, bound as TracerC.trace (src/drrt.cpp:51) */
DRRT_API int drrt_trace_f32(const float* rif, long long nvox, const int res[3], size_t n,
                   const float* pos, const float* vel, float h, float ds,
                   float* xt, float* vt,
                   drrt_stats* stats, void* workspace, size_t workspace_bytes,
                   unsigned flags, void* stream);

/* fp16 ray-state variant of drrt_trace_f32 (BASELINE.json config 5: "fp16 ray state + fp32 adjoint
 * accumulate"; the reference is fp32-only, include/types.h:36-46).  pos, vel, xt, vt are (n,3) IEEE
 * half; values are widened exactly on load, the march is fp32, outputs are rounded to half once:
 * result == half(drrt_trace_f32(float(pos), float(vel))) bit for bit.                            */
DRRT_API int drrt_trace_f16io(const float* rif, long long nvox, const int res[3], size_t n,
                     const void* pos_h, const void* vel_h, float h, float ds,
                     void* xt_h, void* vt_h,
                     drrt_stats* stats, void* workspace, size_t workspace_bytes,
                     unsigned flags, void* stream);

/* Tracer::trace_plane -- src/tracer.cpp:102-172, bound as TracerC.trace_pln (src/drrt.cpp:52).
 * failmask[i] = 1 for rays that never got flagged escaped (uint8, n entries).                 */
DRRT_API int drrt_trace_pln_f32(const float* rif, long long nvox, const int res[3], size_t n,
                       const float* pos, const float* vel,
                       const float* pln_o, const float* pln_d, float h, float ds,
                       float* xt, float* vt, uint8_t* failmask,
                       drrt_stats* stats, void* workspace, size_t workspace_bytes,
                       unsigned flags, void* stream);

/* Tracer::trace_target -- src/tracer.cpp:174-242, TracerC.trace_target (src/drrt.cpp:54).
 * Records the state at closest approach to target[i]; dist2 = squared distance there.          */
DRRT_API int drrt_trace_target_f32(const float* rif, long long nvox, const int res[3], size_t n,
                          const float* pos, const float* vel, const float* target,
                          float h, float ds, float* xt, float* vt, float* dist2,
                          drrt_stats* stats, void* workspace, size_t workspace_bytes,
                          unsigned flags, void* stream);

/* Tracer::trace_sdf -- src/tracer.cpp:244-310, TracerC.trace_sdf (src/drrt.cpp:53).
 * Always needs a workspace of drrt_workspace_bytes(n, flags) bytes (n flag bytes for the second pass that
 * reproduces the reference's global-loop behaviour of rays leaving the box while still sdf-inside).  */
DRRT_API int drrt_trace_sdf_f32(const float* rif, const float* sdf, long long nvox, const int res[3],
                       size_t n, const float* pos, const float* vel, float h, float ds,
                       float* xt, float* vt,
                       drrt_stats* stats, void* workspace, size_t workspace_bytes,
                       unsigned flags, void* stream);

/* Tracer::trace_cable -- src/tracer.cpp:312-382, TracerC.trace_cable (src/drrt.cpp:55).
 * rif = radial profile fp32[rres] (src/cylinder_volume.cpp).                                    */
DRRT_API int drrt_trace_cable_f32(const float* rif, size_t rres, float radius, float length, size_t n,
                         const float* pos, const float* vel, const float* target, float ds,
                         float* xt, float* vt, float* dist2,
                         drrt_stats* stats, void* workspace, size_t workspace_bytes,
                         unsigned flags, void* stream);

/* ---- adjoint marches: accumulate dL/dn into `grad` --------------------------------------- */

/* Tracer::backtrace -- src/tracer.cpp:384-440, TracerC.backtrace (src/drrt.cpp:56).
 * grad: fp32[nvox]; zeroed by the call unless DRRT_FLAG_NO_ZERO.                                 */
DRRT_API int drrt_backtrace_f32(const float* rif, long long nvox, const int res[3], size_t n,
                       const float* xt, const float* vt, const float* dx, const float* dv,
                       float h, float ds, float* grad,
                       drrt_stats* stats, void* workspace, size_t workspace_bytes,
                       unsigned flags, void* stream);

/* Ray-state adjoint of drrt_trace_f32 (the reference's ADTracerC, core/tracer.py:16-66, through enoki autodiff): dL/dpos and
 * dL/dvel of the rays that went INTO a trace call, from the seeds dx = dL/dxt, dv = dL/dvt on its exit rays.  Not in the
 * reference's C++ Tracer.  Nothing is written to a gradient grid: dL/dn is drrt_backtrace_f32's.
 *   pos, vel    the forward call's inputs; xt, vt its outputs; fwd_steps its per-ray iteration counts K (drrt_last_steps()
 *               right after that call; copy them out of the workspace if anything runs in between), all caller ray order
 *   dpos, dvel  out: (n,3) fp32, caller ray order
 * Contract (the exact derivative of the forward's recurrences): the forward samples n only inside the box
 * (Q4), so a ray entering from outside flies straight for e iterations first (x_e = pos + e ds vel).  The call replays that
 * prefix from (pos, vel) with the forward's own fp32 operations, then runs K - e reverse iterations from (xt, vt), seeded
 * like drrt_backtrace_f32 (lambda = dx, mu = dv + ds dx) -- no backward-escape test, no adjoint step bound -- and writes
 * dpos = lambda, dvel = mu before its last update + e ds lambda.  A ray whose prefix never samples inside (it never
 * entered: xt = pos, vt = vel) gets (dx, dv).  A ray with K >= the forward's max_steps failed (Q5, Q6: vt is the stale
 * vel) and gets a zero gradient and counts in stats->n_failed; a ray that exited on exactly its last allowed iteration is
 * indistinguishable from one and is treated the same.  stats->ray_steps = reverse iterations executed.  The result does
 * not depend on DRRT_FLAG_CORRECTED_H (the 1/h of Q3 scales the grid splat only) nor on the visit order.
 * Flags: DRRT_FLAG_SORT_RAYS, DRRT_FLAG_PAIR_GRID / _PAIR_REUSE and DRRT_FLAG_DISPATCH_IN_ORDER as for drrt_backtrace_f32;
 * the order hint (normally the paired forward's) is consumed like there, the step hint is ignored (fwd_steps is the
 * argument).  fp32 only.                                                                                                 */
DRRT_API int drrt_backtrace_rays_f32(const float* rif, long long nvox, const int res[3], size_t n,
                       const float* pos, const float* vel,
                       const float* xt, const float* vt,
                       const uint32_t* fwd_steps,
                       const float* dx, const float* dv, float h, float ds,
                       float* dpos, float* dvel,
                       drrt_stats* stats, void* workspace, size_t workspace_bytes,
                       unsigned flags, void* stream);

/* ---- optical path length (not in the reference) ------------------------------------------------------------------------
 * The march integrates dx/dsigma = v, dv/dsigma = n grad n, so |v| = n and the optical path length int n dl is
 * int n^2 dsigma.  drrt_trace_opl_f32 is drrt_trace_f32 (xt, vt and the per-ray iteration counts K bit for bit) that also
 * returns  opl = sum_{k<K} ds n_k^2  over the masked samples n_k the march takes at x_k anyway (0 while the ray is not
 * inside the box: free flight adds nothing), accumulated in fp32 as opl = fmaf(ds n_k, n_k, opl) in iteration order from 0.
 * A failed ray (K >= max_steps) returns what it accumulated.
 *   opl        out: fp32[n]
 *   steps_out  out: uint32[n], required: K per ray, caller ray order (what the adjoint takes as fwd_steps).  The call
 *              leaves no drrt_last_steps().
 * Flags: DRRT_FLAG_SORT_RAYS, DRRT_FLAG_PAIR_GRID / _PAIR_REUSE, DRRT_FLAG_DISPATCH_IN_ORDER as for drrt_trace_f32.  fp32 only. */
DRRT_API int drrt_trace_opl_f32(const float* rif, long long nvox, const int res[3], size_t n,
                       const float* pos, const float* vel, float h, float ds,
                       float* xt, float* vt, float* opl, uint32_t* steps_out,
                       drrt_stats* stats, void* workspace, size_t workspace_bytes,
                       unsigned flags, void* stream);

/* Adjoint of drrt_trace_opl_f32: from the seeds dx = dL/dxt, dv = dL/dvt, dopl = dL/dopl (each nullable: read as zeros) ONE
 * reverse march yields dL/dn (grad), dL/dpos and dL/dvel.  The march is drrt_backtrace_rays_f32's, unchanged in structure
 * (replayed free-flight prefix, K - e reverse iterations, the last sampled at the replayed x_e, no backward-escape test;
 * failed rays get zeros, contribute nothing and count in stats->n_failed; never-entered rays get (dx, dv) and contribute
 * nothing).  Each reverse iteration uses  dn = mu . grad n_k + 2 dopl n_k  where that march uses mu . grad n_k, and adds
 * splat_weights(w, dn ds, (n_k ds grad_scale) mu), formed with mu before its update, at the 8 taps of the sampled cell.
 * grad_scale = 1 / h with DRRT_FLAG_CORRECTED_H -- then the result is the exact discrete derivative -- and 1 without, as
 * for drrt_backtrace_f32 (Q3).
 *   grad        out, nullable (no scatter at all): fp32[nvox], zeroed by the call unless DRRT_FLAG_NO_ZERO
 *   dpos, dvel  out, both or neither: (n,3) fp32.  grad, dpos and dvel all null: DRRT_ERR_ARG
 * The scatter is one global fp32 atomic per tap and per run of samples in one cell (a lane sums in registers while it
 * stays in a cell): there is no LDS window here, so rays focused into a few voxels run at the memory-side atomic rate.
 * Flags: DRRT_FLAG_SORT_RAYS, DRRT_FLAG_PAIR_GRID / _PAIR_REUSE, DRRT_FLAG_DISPATCH_IN_ORDER, DRRT_FLAG_CORRECTED_H,
 * DRRT_FLAG_NO_ZERO; other adjoint flags are ignored.  The order hint is consumed, the step hint ignored.  fp32 only.      */
DRRT_API int drrt_backtrace_opl_f32(const float* rif, long long nvox, const int res[3], size_t n,
                       const float* pos, const float* vel,
                       const float* xt, const float* vt,
                       const uint32_t* fwd_steps,
                       const float* dx, const float* dv, const float* dopl, float h, float ds,
                       float* grad, float* dpos, float* dvel,
                       drrt_stats* stats, void* workspace, size_t workspace_bytes,
                       unsigned flags, void* stream);

/* ---- line integral of a second field along the bent ray (not in the reference) -------------------------------------------
 * tau = int a dl of a second voxel field a -- an absorption or emission coefficient, a group index -- along the ray that n
 * bends.  `field` is an fp32 grid of exactly rif's shape and axis convention (res[0] indexes the fastest axis).  |v| = n
 * along the march, so dl = n dsigma: drrt_trace_field_f32 is drrt_trace_f32 (xt, vt and the per-ray iteration counts K bit
 * for bit) that also returns  tau = sum_{k<K} ds n_k a_k,  n_k the masked sample the march takes at x_k anyway (0 while the
 * ray is not inside the box: free flight adds nothing) and a_k the trilinear sample of `field` at the same cell, with the
 * same weights and the same mask, accumulated in fp32 as tau = fmaf(ds n_k, a_k, tau) in iteration order from 0.  With
 * field holding rif's values tau is drrt_trace_opl_f32's opl bit for bit.  A failed ray returns what it accumulated.
 *   tau        out: fp32[n]
 *   steps_out  out: uint32[n], required: K per ray, caller ray order (what the adjoint takes as fwd_steps).  The call
 *              leaves no drrt_last_steps().
 * Flags: DRRT_FLAG_SORT_RAYS, DRRT_FLAG_PAIR_GRID / _PAIR_REUSE (the pair copy is of rif; field is gathered as it is),
 * DRRT_FLAG_DISPATCH_IN_ORDER as for drrt_trace_f32.  fp32 only. */
DRRT_API int drrt_trace_field_f32(const float* rif, const float* field, long long nvox, const int res[3], size_t n,
                       const float* pos, const float* vel, float h, float ds,
                       float* xt, float* vt, float* tau, uint32_t* steps_out,
                       drrt_stats* stats, void* workspace, size_t workspace_bytes,
                       unsigned flags, void* stream);

/* Adjoint of drrt_trace_field_f32: from the seeds dx = dL/dxt, dv = dL/dvt, dtau = dL/dtau (each nullable: read as zeros) ONE
 * reverse march yields dL/drif (grad), dL/dfield (grad_field), dL/dpos and dL/dvel.  The march is drrt_backtrace_opl_f32's,
 * unchanged in structure (failed rays get zeros, contribute nothing and count in stats->n_failed; never-entered rays get
 * (dx, dv) and contribute nothing).  Each reverse iteration samples rif (n_k, grad n_k, mixed partials) and field (a_k,
 * grad a_k, scaled by 1 / h like grad n_k) at the same cell, uses  dn = mu . grad n_k + dtau a_k  where drrt_backtrace_rays_f32
 * uses mu . grad n_k, adds  (dtau ds n_k) grad a_k  to lambda before the recurrences -- the pull of the field's gradient on
 * the sample position -- and adds, with mu before its update, at the 8 taps of the sampled cell
 *   to grad:        splat_weights(w, dn ds, (n_k ds grad_scale) mu),  grad_scale = 1 / h with DRRT_FLAG_CORRECTED_H and 1
 *                   without, as for drrt_backtrace_f32 (Q3);
 *   to grad_field:  the value weights alone, w_c (dtau ds n_k): tau is linear in the field, so there is no gradient splat
 *                   and grad_scale does not enter.
 * With DRRT_FLAG_CORRECTED_H all four outputs are the exact derivative of the discrete forward; grad_field, dpos and dvel
 * are that with either setting.
 *   grad, grad_field  out, each nullable (no scatter into that grid): fp32[nvox], zeroed by the call unless
 *                     DRRT_FLAG_NO_ZERO, which applies to both
 *   dpos, dvel        out, both or neither: (n,3) fp32.  All four outputs null: DRRT_ERR_ARG
 * The scatter is one global fp32 atomic per tap, per grid and per run of samples in one cell, as for drrt_backtrace_opl_f32:
 * no LDS window, so a call that scatters into both grids pays the memory-side atomic rate twice.
 * Flags: DRRT_FLAG_SORT_RAYS, DRRT_FLAG_PAIR_GRID / _PAIR_REUSE, DRRT_FLAG_DISPATCH_IN_ORDER, DRRT_FLAG_CORRECTED_H,
 * DRRT_FLAG_NO_ZERO; other adjoint flags are ignored.  The order hint is consumed, the step hint ignored.  fp32 only.      */
DRRT_API int drrt_backtrace_field_f32(const float* rif, const float* field, long long nvox, const int res[3], size_t n,
                       const float* pos, const float* vel,
                       const float* xt, const float* vt,
                       const uint32_t* fwd_steps,
                       const float* dx, const float* dv, const float* dtau, float h, float ds,
                       float* grad, float* grad_field, float* dpos, float* dvel,
                       drrt_stats* stats, void* workspace, size_t workspace_bytes,
                       unsigned flags, void* stream);

/* ---- emission with self-absorption along the bent ray (not in the reference) ----------------------------------------------
 * rad = int e(s) exp(-int_0^s a) ds, the radiative-transfer line integral: what a camera sees through a medium that emits
 * (e) and absorbs (a) along the ray that n bends.  `emission` and `absorption` are fp32 grids of exactly rif's shape and
 * axis convention.  drrt_trace_emission_f32 is drrt_trace_f32 (xt, vt and the per-ray iteration counts K bit for bit) that
 * also returns rad and tau.  With n_k the masked sample the march takes at x_k anyway (0 while the ray is not inside the
 * box), w_k = ds n_k, and e_k, a_k the trilinear samples of the two fields at the same cell, with the same weights and the
 * same mask, in fp32 and in iteration order from tau_0 = rad_0 = 0:
 *   T_k       = exp_neg(tau_k)                 the transmittance in front of sample k
 *   rad_{k+1} = fmaf(T_k w_k, e_k, rad_k)      emit, then absorb
 *   tau_{k+1} = fmaf(w_k, a_k, tau_k)          drrt_trace_field_f32's tau of the field a, bit for bit
 * exp_neg(t) = exp(-t) is the library's own operation sequence (csrc/drrt_device.h: argument clamped to +-87, relative
 * error 7.9e-8, exp_neg(0) = 1 exactly, NaN in -> NaN out), so with absorption = 0 everywhere rad is
 * drrt_trace_field_f32's tau of the field e bit for bit.  Negative absorption (gain) is legal.  A failed ray returns what
 * it accumulated; a ray that never samples inside returns rad = tau = 0.
 *   rad, tau   out: fp32[n] each
 *   steps_out  out: uint32[n], required: K per ray, caller ray order (what the adjoint takes as fwd_steps).  The call
 *              leaves no drrt_last_steps().
 * Flags: DRRT_FLAG_SORT_RAYS, DRRT_FLAG_PAIR_GRID / _PAIR_REUSE (the pair copy is of rif; the two fields are gathered as
 * they are), DRRT_FLAG_DISPATCH_IN_ORDER as for drrt_trace_f32.  fp32 only. */
DRRT_API int drrt_trace_emission_f32(const float* rif, const float* emission, const float* absorption, long long nvox,
                       const int res[3], size_t n,
                       const float* pos, const float* vel, float h, float ds,
                       float* xt, float* vt, float* rad, float* tau, uint32_t* steps_out,
                       drrt_stats* stats, void* workspace, size_t workspace_bytes,
                       unsigned flags, void* stream);

/* Adjoint of drrt_trace_emission_f32: from the seeds dx = dL/dxt, dv = dL/dvt, drad = dL/drad, dtau = dL/dtau (each
 * nullable: read as zeros) ONE reverse march yields dL/drif (grad), dL/demission (grad_emission), dL/dabsorption
 * (grad_absorption), dL/dpos and dL/dvel.  `tau` is the forward's tau (required when n > 0).  The march is
 * drrt_backtrace_field_f32's, unchanged in structure (failed rays get zeros, contribute nothing and count in
 * stats->n_failed; never-entered rays get (dx, dv) and contribute nothing), with two running scalars: t, from the
 * forward's tau, stepped back by t = fmaf(-w_k, a_k, t) to tau_k, and P, from dtau, the derivative of L w.r.t. the optical
 * depth behind the sample.  Each reverse iteration samples rif, emission and absorption at the same cell and, with
 * ce = drad exp_neg(t), uses  dn = mu . grad n_k + (ce e_k + P a_k)  where drrt_backtrace_rays_f32 uses mu . grad n_k, adds
 * (ce w_k) grad e_k + (P w_k) grad a_k  to lambda before the recurrences, adds, with mu before its update, at the 8 taps
 * of the sampled cell
 *   to grad:             splat_weights(w, dn ds, (n_k ds grad_scale) mu), grad_scale = 1 / h with DRRT_FLAG_CORRECTED_H and
 *                        1 without, as for drrt_backtrace_f32 (Q3);
 *   to grad_emission:    the value weights alone, w_c (ce w_k);
 *   to grad_absorption:  the value weights alone, w_c (P w_k);
 * and then steps P = fmaf(-(ce w_k), e_k, P).  The transmittance is always recovered from tau, never by dividing it, so an
 * opaque ray (exp_neg at its clamp) gets finite gradients.  tau_k is recomputed by subtraction, so the transmittance of the
 * reverse march differs from the forward's by rounding only: grad_emission, grad_absorption, dpos and dvel are the
 * derivative of the discrete forward to fp32 rounding with either setting; grad is the same derivative with
 * DRRT_FLAG_CORRECTED_H.  With drad null or zero this is drrt_backtrace_field_f32 with field = absorption.
 *   grad, grad_emission, grad_absorption  out, each nullable (no scatter into that grid): fp32[nvox], zeroed by the call
 *                        unless DRRT_FLAG_NO_ZERO, which applies to all three
 *   dpos, dvel           out, both or neither: (n,3) fp32.  All five outputs null: DRRT_ERR_ARG
 * The scatter is one global fp32 atomic per tap, per grid and per run of samples in one cell, as for
 * drrt_backtrace_field_f32: no LDS window, so a call pays the memory-side atomic rate once per grid it scatters into.
 * Flags: DRRT_FLAG_SORT_RAYS, DRRT_FLAG_PAIR_GRID / _PAIR_REUSE, DRRT_FLAG_DISPATCH_IN_ORDER, DRRT_FLAG_CORRECTED_H,
 * DRRT_FLAG_NO_ZERO; other adjoint flags are ignored.  The order hint is consumed, the step hint ignored.  fp32 only.      */
DRRT_API int drrt_backtrace_emission_f32(const float* rif, const float* emission, const float* absorption, long long nvox,
                       const int res[3], size_t n,
                       const float* pos, const float* vel,
                       const float* xt, const float* vt,
                       const uint32_t* fwd_steps, const float* tau,
                       const float* dx, const float* dv, const float* drad, const float* dtau, float h, float ds,
                       float* grad, float* grad_emission, float* grad_absorption, float* dpos, float* dvel,
                       drrt_stats* stats, void* workspace, size_t workspace_bytes,
                       unsigned flags, void* stream);

/* ---- line integral of a vector field along the bent ray (not in the reference) --------------------------------------------
 * circ = int u . dl of a vector field u projected on the ray's own direction -- a flow velocity (Doppler and time-of-flight
 * flow tomography), n_e B (Faraday rotation) -- along the ray that n bends.  `vfield` is 3 nvox fp32: three component planes
 * of exactly rif's shape and axis convention, plane c at vfield + c nvox, and plane c = 0, 1, 2 pairs with component c of
 * pos / vel (x, y, z).  drrt_trace_vector_f32 is drrt_trace_f32 (xt, vt and the per-ray iteration counts K bit for bit)
 * that also returns
 *   circ = sum_{k<K} ds (u_k . v_{k+1})  =  sum_k u(x_k) . (x_{k+1} - x_k)
 * u_k the trilinear sample of the three planes at the cell the march samples at x_k anyway, with the same weights and the
 * same mask (0 while the ray is not inside the box: free flight adds nothing), and v_{k+1} the velocity behind the update
 * from sample k, the one that carries the ray from x_k to x_{k+1}; accumulated in fp32 in iteration order from 0 as
 * t = ux vx; t = fmaf(uy, vy, t); t = fmaf(uz, vz, t); circ = fmaf(ds, t, circ).  The sum telescopes: for a uniform u,
 * circ = u . (xt - x_e) with x_e the first in-box sample.  A failed ray returns what it accumulated; a ray that never
 * samples inside returns circ = 0.
 *   circ       out: fp32[n]
 *   steps_out  out: uint32[n], required: K per ray, caller ray order (what the adjoint takes as fwd_steps).  The call
 *              leaves no drrt_last_steps().
 * Flags: DRRT_FLAG_SORT_RAYS, DRRT_FLAG_PAIR_GRID / _PAIR_REUSE (the pair copy is of rif; the three planes are gathered as
 * they are), DRRT_FLAG_DISPATCH_IN_ORDER as for drrt_trace_f32.  fp32 only. */
DRRT_API int drrt_trace_vector_f32(const float* rif, const float* vfield, long long nvox, const int res[3], size_t n,
                       const float* pos, const float* vel, float h, float ds,
                       float* xt, float* vt, float* circ, uint32_t* steps_out,
                       drrt_stats* stats, void* workspace, size_t workspace_bytes,
                       unsigned flags, void* stream);

/* Adjoint of drrt_trace_vector_f32: from the seeds dx = dL/dxt, dv = dL/dvt, dcirc = dL/dcirc (each nullable: read as zeros)
 * ONE reverse march yields dL/drif (grad), dL/du (grad_vfield, three planes laid out as vfield), dL/dpos and dL/dvel.  The
 * march is drrt_backtrace_field_f32's, unchanged in structure (failed rays get zeros, contribute nothing and count in
 * stats->n_failed; never-entered rays get (dx, dv) and contribute nothing).  The summand of sample k holds v_{k+1}, the
 * velocity the reverse march arrives with, so each reverse iteration first samples the three planes (u_k, grad u_k scaled
 * by 1 / h like grad n_k) at the cell of x_k and, with g = dcirc ds, adds  g u_k  to mu -- the seed on v_{k+1} -- BEFORE
 * dn = mu . grad n_k is formed and keeps  w = g v_{k+1};  then it samples rif, and adds, with mu before its update, at the
 * 8 taps of the sampled cell
 *   to grad:                   splat_weights(w, dn ds, (n_k ds grad_scale) mu),  grad_scale = 1 / h with
 *                              DRRT_FLAG_CORRECTED_H and 1 without, as for drrt_backtrace_f32 (Q3);
 *   to plane c of grad_vfield: the value weights alone, w_c-weights of w[c]: circ is linear in u, so there is no gradient
 *                              splat and grad_scale does not enter;
 * and adds  (grad u_k)^T w  to lambda before the recurrences -- the pull of the field's gradient on the sample position.
 * With DRRT_FLAG_CORRECTED_H all outputs are the exact derivative of the discrete forward; grad_vfield, dpos and dvel are
 * that with either setting.
 *   grad         out, nullable (no scatter into dL/drif): fp32[nvox]
 *   grad_vfield  out, nullable (no scatter into dL/du): fp32[3 nvox]; both are zeroed by the call unless DRRT_FLAG_NO_ZERO
 *   dpos, dvel   out, both or neither: (n,3) fp32.  All four outputs null: DRRT_ERR_ARG
 * The scatter is one global fp32 atomic per tap, per grid and per run of samples in one cell, as for
 * drrt_backtrace_field_f32: no LDS window, so a call pays the memory-side atomic rate once per plane it scatters into
 * (three for grad_vfield, four with grad).
 * Flags: DRRT_FLAG_SORT_RAYS, DRRT_FLAG_PAIR_GRID / _PAIR_REUSE, DRRT_FLAG_DISPATCH_IN_ORDER, DRRT_FLAG_CORRECTED_H,
 * DRRT_FLAG_NO_ZERO; other adjoint flags are ignored.  The order hint is consumed, the step hint ignored.  fp32 only.      */
DRRT_API int drrt_backtrace_vector_f32(const float* rif, const float* vfield, long long nvox, const int res[3], size_t n,
                       const float* pos, const float* vel,
                       const float* xt, const float* vt,
                       const uint32_t* fwd_steps,
                       const float* dx, const float* dv, const float* dcirc, float h, float ds,
                       float* grad, float* grad_vfield, float* dpos, float* dvel,
                       drrt_stats* stats, void* workspace, size_t workspace_bytes,
                       unsigned flags, void* stream);

/* ---- ray paths: where every bent ray went (not in the reference) ---------------------------------------------------------
 * drrt_trace_path_f32 is drrt_trace_f32 (xt, vt and the per-ray iteration counts K bit for bit, failed rays included: Q5,
 * Q6) that also returns every stride-th marching position of every ray.  Per ray, with x_k the marching position in front
 * of iteration k (x_0 = pos; fp32, the march's own values), stride >= 1 and samples = M >= 1:
 *   count[i]   = min(M, ceil(K / stride)): the strided samples x_{j stride} with j stride < K that fit
 *   path[j]    = x_{j stride}  for j < count
 *   path[j]    = xt            for count <= j < M (padding): a series that is long enough ends on the exit ray's position.
 *                A ray that never samples inside the box has xt = pos by the march's own convention (Q6), so its padding
 *                is pos; count says where to cut.
 * M stride < K truncates the series: no padding, and no error.  M = ceil(max_steps / stride) + 1 is the smallest M that
 * always ends on xt (max_steps: the forward's bound, (int)(4 h max(res) / ds)).
 *   path       out: fp32 (M, n, 3), sample-major: entry j of ray i at (j n + i) 3.  path[j] is every ray at sample j; a
 *              wave stores one contiguous run per sample when the rays are visited in caller order
 *   count      out: int32[n]
 *   steps_out  out: uint32[n], required, as for drrt_trace_opl_f32
 * DRRT_ERR_ARG: stride < 1, samples < 1, samples n 3 floats overflowing size_t (the kernels' index type), and the checks
 * of drrt_trace_opl_f32 (count is checked with the ray pointers).
 * Flags: as for drrt_trace_opl_f32.  fp32 only.                                                                         */
DRRT_API int drrt_trace_path_f32(const float* rif, long long nvox, const int res[3], size_t n,
                       const float* pos, const float* vel, float h, float ds, int stride, int samples,
                       float* xt, float* vt, float* path, int* count, uint32_t* steps_out,
                       drrt_stats* stats, void* workspace, size_t workspace_bytes,
                       unsigned flags, void* stream);

/* Adjoint of drrt_trace_path_f32: the derivative of the discrete forward with K and count held fixed, from the seeds
 * dx = dL/dxt, dv = dL/dvt ((n,3)) and dpath = dL/dpath ((M, n, 3), path's layout), each nullable: read as zeros.  ONE
 * reverse march yields dL/dn (grad), dL/dpos and dL/dvel.  The march is drrt_backtrace_opl_f32's with dopl null; with dpath
 * null the results are that call's bit for bit.  With e the free-flight prefix of the ray (drrt_backtrace_rays_f32):
 *   * the seed on a sample x_k, k > e, is added to lambda in the reverse iteration that arrives at x_k, before that
 *     iteration's lambda / mu recurrences (mu += ds lambda sees it);
 *   * the seeds on the prefix samples x_k = pos + k ds vel, k <= e, go straight to the result behind the march, in
 *     ascending j:  dpos += g,  dvel = fmaf((float)k * ds, g, dvel)  (the way e ds is formed for dvel);
 *   * the seeds on padded entries are seeds on xt: they are added to dx in ascending j, in fp32, ((dx + g_count) +
 *     g_{count+1}) + ..., before the march is initialised, so mu = dv + ds dx sees them;
 *   * a ray that never sampled inside (e = K) gets (dx, dv) with its padding and prefix seeds as above and contributes
 *     nothing to grad; a failed ray gets zeros, contributes nothing and counts in stats->n_failed.
 * grad is the exact discrete derivative with DRRT_FLAG_CORRECTED_H, as for drrt_backtrace_opl_f32; the ray gradients are
 * exact either way.  stride and samples are the forward's.
 *   grad        out, nullable (no scatter at all): fp32[nvox], zeroed by the call unless DRRT_FLAG_NO_ZERO
 *   dpos, dvel  out, both or neither: (n,3) fp32.  grad, dpos and dvel all null: DRRT_ERR_ARG
 * DRRT_ERR_ARG also for stride < 1, samples < 1 and samples n 3 floats overflowing size_t.
 * Flags and hints: as for drrt_backtrace_opl_f32.  fp32 only.                                                           */
DRRT_API int drrt_backtrace_path_f32(const float* rif, long long nvox, const int res[3], size_t n,
                       const float* pos, const float* vel,
                       const float* xt, const float* vt,
                       const uint32_t* fwd_steps,
                       const float* dx, const float* dv, const float* dpath, float h, float ds,
                       int stride, int samples,
                       float* grad, float* dpos, float* dvel,
                       drrt_stats* stats, void* workspace, size_t workspace_bytes,
                       unsigned flags, void* stream);

/* ---- ray paths with velocities: the march's state at every sample (not in the reference) ------------------------------
 * drrt_trace_phase_f32 is drrt_trace_path_f32 with one more output, vpath: xt, vt, path, count, steps_out and the
 * statistics are that call's bit for bit.  Per ray, with v_k the marching velocity in front of iteration k -- v_0 = vel,
 * and for k >= 1 the velocity that carried the ray from x_{k-1} to x_k: x_k = fmaf(ds, v_k, x_{k-1}), fp32, the march's own
 * values -- and count as there:
 *   vpath[j]   = v_{j stride}  for j < count
 *   vpath[j]   = vt            for count <= j < M (padding, whatever the march's conventions make vt: the stale vel for a
 *                failed ray, Q6, and vel for a ray that never samples inside)
 * so (path[j], vpath[j]) is the march's state at sample j, and a series that is long enough ends on (xt, vt).  |v| = n along
 * the march: |vpath[j]| is the refractive index the ray saw at sample j.  A chord of path, (path[j+1] - path[j]) /
 * (ds stride), is NOT vpath[j] for stride > 1.
 *   vpath      out, required: fp32 (M, n, 3) in path's layout, stored in path's order (one contiguous run per sample and
 *              series from a wave that visits the rays in caller order)
 * Everything else -- arguments, flags, workspace, DRRT_ERR_ARG (the size_t overflow check holds for each series; vpath is
 * checked with the ray pointers) -- is as for drrt_trace_path_f32.  fp32 only.                                            */
DRRT_API int drrt_trace_phase_f32(const float* rif, long long nvox, const int res[3], size_t n,
                       const float* pos, const float* vel, float h, float ds, int stride, int samples,
                       float* xt, float* vt, float* path, float* vpath, int* count, uint32_t* steps_out,
                       drrt_stats* stats, void* workspace, size_t workspace_bytes,
                       unsigned flags, void* stream);

/* Adjoint of drrt_trace_phase_f32: drrt_backtrace_path_f32 with one more seed, dvpath = dL/dvpath ((M, n, 3), nullable:
 * read as zeros), the derivative of the discrete forward with K and count held fixed.  ONE reverse march yields dL/dn
 * (grad), dL/dpos and dL/dvel; with dvpath null every result is drrt_backtrace_path_f32's bit for bit.  The seeds on path
 * are placed as there.  With e the free-flight prefix of the ray:
 *   * the seed on a sample v_k, e < k < K, is a seed on the total adjoint of v_k (v_k enters only through x_k = x_{k-1} +
 *     ds v_k and v_{k+1} = v_k + ...): it is added to mu at the start of the reverse iteration that arrives at x_{k-1}, in
 *     front of that iteration's sample, so that mu . grad n, the contribution to grad and dL/dvel see it.  That is one
 *     reverse iteration behind the position seed on x_k; the sample k = e + 1 is seeded in the entry iteration;
 *   * v_k = vel bit for bit for k <= e: these seeds are added to dvel behind the march (and behind the prefix's position
 *     seeds) in ascending j, and add nothing to dpos;
 *   * the seeds on padded entries are seeds on vt: they are added to dv in ascending j, in fp32, ((dv + g_count) +
 *     g_{count+1}) + ..., before the march is initialised, so mu = dv + ds dx sees them;
 *   * a ray that never sampled inside (e = K) gets drrt_backtrace_path_f32's result with every vpath seed added to dvel;
 *     a failed ray gets zeros (no seed is read), contributes nothing and counts in stats->n_failed.
 * Outputs, flags, hints and DRRT_ERR_ARG: as for drrt_backtrace_path_f32.  fp32 only.                                    */
DRRT_API int drrt_backtrace_phase_f32(const float* rif, long long nvox, const int res[3], size_t n,
                       const float* pos, const float* vel,
                       const float* xt, const float* vt,
                       const uint32_t* fwd_steps,
                       const float* dx, const float* dv, const float* dpath, const float* dvpath, float h, float ds,
                       int stride, int samples,
                       float* grad, float* dpos, float* dvel,
                       drrt_stats* stats, void* workspace, size_t workspace_bytes,
                       unsigned flags, void* stream);

/* fp16 ray-state variant of drrt_backtrace_f32: xt, vt, dx, dv are (n,3) IEEE half, the adjoint
 * recurrences and the accumulation into `grad` stay fp32.                                        */
DRRT_API int drrt_backtrace_f16io(const float* rif, long long nvox, const int res[3], size_t n,
                         const void* xt_h, const void* vt_h, const void* dx_h, const void* dv_h,
                         float h, float ds, float* grad,
                         drrt_stats* stats, void* workspace, size_t workspace_bytes,
                         unsigned flags, void* stream);

/* Tracer::backtrace in depth chunks (not in the reference; for the multi-GPU path): the iterations
 * [it_begin, it_begin + it_count) of the adjoint march's max_steps (drrt_backtrace_max_steps(); it_count < 0 = all that are
 * left), same arguments as drrt_backtrace_f32.  it_begin == 0 starts from (xt, vt, dx, dv) and zeroes `grad` (unless
 * DRRT_FLAG_NO_ZERO) and `stats`; it_begin > 0 continues from `state` (drrt_backtrace_chunk_state_bytes(n) bytes, written
 * by the previous chunk; opaque) and accumulates into `grad` and `stats`.  After the last chunk `grad` holds what
 * drrt_backtrace_f32 computes -- the same per-ray contributions, summed in another order.  Why: with rays that travel on
 * one clock (a plane source) the part of the grid every ray has left behind is FINAL after a chunk, so a rank can start
 * reducing that slab with the other ranks while its next chunk marches (adjointnonlinearraytracing_amd/dist.py).
 *   visit order  every chunk of a march must visit the rays in the SAME order (the state is stored per visit slot): with
 *                DRRT_FLAG_SORT_RAYS hand the order of the first chunk (drrt_last_order(), or the paired forward's) to
 *                every later chunk with drrt_set_order_hint(); a resumed chunk without it is refused.
 *   progress     nullable DEVICE pointer to 20 ints, written by the chunk: where the rays that are still marching stand
 *                and head -- [0..2] min and [3..5] max of their positions (x, y, z: the NEXT sample of each ray), [6..8] min
 *                and [9..11] max of their velocities, as order-preserving keys (key = bits >= 0 ? bits : bits ^ 0x7fffffff;
 *                the map is its own inverse), [12] their number -- and [13..15] min, [16..18] max of the positions of
 *                the samples THIS chunk contributed at (a sample at p touches the voxels floor(p / h) and floor(p / h) + 1
 *                per axis), [19] unused.  The march moves a ray by -ds * v per iteration: a half space that lies behind
 *                every marching ray and that no ray heads back into is final; the sample box of the NEXT chunk tells
 *                afterwards whether that held.
 * Runs the box-window kernel (k_backtrace_flat) whatever the bundles look like; fp32 ray state only.                  */
DRRT_API size_t drrt_backtrace_chunk_state_bytes(size_t n);
DRRT_API int drrt_backtrace_max_steps(const int res[3], float h, float ds);      /* src/tracer.cpp:417 (Q5); < 0: bad arguments */
DRRT_API int drrt_backtrace_chunk_f32(const float* rif, long long nvox, const int res[3], size_t n,
                         const float* xt, const float* vt, const float* dx, const float* dv,
                         float h, float ds, float* grad,
                         drrt_stats* stats, void* workspace, size_t workspace_bytes,
                         unsigned flags, void* stream,
                         void* state, size_t state_bytes, int it_begin, int it_count, int* progress);

/* Tracer::backtrace_sdf -- src/tracer.cpp:443-509, TracerC.backtrace_sdf (src/drrt.cpp:57).     */
DRRT_API int drrt_backtrace_sdf_f32(const float* rif, const float* sdf, long long nvox, const int res[3],
                           size_t n, const float* xt, const float* vt,
                           const float* dx, const float* dv, float h, float ds, float* grad,
                           drrt_stats* stats, void* workspace, size_t workspace_bytes,
                           unsigned flags, void* stream);

/* Tracer::backtrace_cable -- src/tracer.cpp:511-567, TracerC.backtrace_cable (src/drrt.cpp:58).
 * grad: fp32[rres].                                                                             */
DRRT_API int drrt_backtrace_cable_f32(const float* rif, size_t rres, float radius, float length, size_t n,
                             const float* xt, const float* vt, const float* dx, const float* dv,
                             float ds, float* grad,
                             drrt_stats* stats, void* workspace, size_t workspace_bytes,
                             unsigned flags, void* stream);

/* Ray-state adjoint of Tracer::trace_cable: dL/dpos, dL/dvel of the rays that entered drrt_trace_cable_f32 (the reference
 * gets them from enoki autodiff, core/tracer.py:237-291 ADCableTracerC).  No contribution to dL/dn is formed.
 *   pos, vel, target   the forward call's inputs, (n,3) fp32
 *   dx, dv             seeds on its outputs (xt, vt); a seed on dist2 does not enter (as in the reference, :268-272)
 *   dpos, dvel         out: (n,3) fp32
 * Contract: (xt, vt) is the state (x_j, v_j) of the iteration j with the smallest squared distance to the target (first
 * minimum; j = 0 is the input itself).  The forward does not report j, so the call replays the forward march from
 * (pos, vel) with the forward's own fp32 operations and takes j and (xt, vt) from the replay; then it runs j reverse
 * iterations from (xt, vt), seeded like drrt_backtrace_cable_f32 (lambda = dx, mu = dv + ds dx) -- no backward-escape
 * test, no adjoint step bound -- and writes dpos = lambda, dvel = mu before its last update.  j = 0 gives (dx, dv).
 * j is held fixed.  A ray that ran out of steps keeps its record and its gradient: stats->n_failed = 0.
 * stats->ray_steps = replay + reverse iterations.  The workspace and flags are not used.  fp32 only.                */
DRRT_API int drrt_backtrace_cable_rays_f32(const float* rif, size_t rres, float radius, float length, size_t n,
                             const float* pos, const float* vel, const float* target,
                             const float* dx, const float* dv, float ds,
                             float* dpos, float* dvel,
                             drrt_stats* stats, void* workspace, size_t workspace_bytes,
                             unsigned flags, void* stream);

/* drrt_trace_cable_f32 with the optical path length of every ray up to its record, and the record's iteration (not in
 * the reference).  xt, vt, dist2 and the statistics are drrt_trace_cable_f32's bit for bit.
 *   opl        out: fp32[n], sum_{k<j} ds n_k^2 over the iterations in front of the record (x_j, v_j), n_k the march's own
 *              unmasked sample at x_k, accumulated in fp32 in iteration order (fmaf(ds n_k, n_k, acc) from 0) and latched
 *              whenever the record is updated; j = 0 (the record is the input) gives 0.  It is the integral of n along the
 *              path -- the transit time up to the record -- when the rays enter with |v| = n.
 *   rec_steps  out: uint32[n], j: what drrt_backtrace_cable_opl_f32 takes, so that it replays nothing
 * The workspace and flags are not used.  fp32 only.                                                                  */
DRRT_API int drrt_trace_cable_opl_f32(const float* rif, size_t rres, float radius, float length, size_t n,
                             const float* pos, const float* vel, const float* target, float ds,
                             float* xt, float* vt, float* dist2, float* opl, uint32_t* rec_steps,
                             drrt_stats* stats, void* workspace, size_t workspace_bytes,
                             unsigned flags, void* stream);

/* The ONE adjoint of drrt_trace_cable_opl_f32: dL/d(profile), dL/dpos and dL/dvel from seeds on (xt, vt, opl), the exact
 * derivative of the discrete forward with the record's iteration held fixed.
 *   pos                the forward call's input positions, (n,3) fp32
 *   xt, vt, rec_steps  its outputs
 *   dx, dv, dopl       seeds on (xt, vt) ((n,3) fp32) and on opl (fp32[n]); each may be null: zeros
 *   grad               out: fp32[rres], zeroed first unless DRRT_FLAG_NO_ZERO (then added into); null: not computed
 *   dpos, dvel         out: (n,3) fp32; both null: not computed.  grad, or dpos and dvel, must be asked for.
 * A ray makes rec_steps[i] reverse iterations from (xt, vt), run as drrt_backtrace_cable_rays_f32 runs them (lambda = dx,
 * mu = dv + ds dx, no backward-escape test, the last sample at pos itself), with dn = mu . grad n_k + 2 dopl n_k; every
 * iteration adds drrt_backtrace_cable_f32's two contributions for that dn to grad.  rec_steps = 0 gives (dx, dv) bit for
 * bit and no contribution.  Nothing flows to target, radius, length or ds, and dist2 takes no seed.
 * rec_steps is the only loop bound: a ray whose count exceeds the forward's own bound (int)(4 length / ds) -- no forward
 * call returns one -- makes no iterations, gets zero gradients and counts in stats->n_failed.  stats->ray_steps = the
 * reverse iterations.  n = 0 zeroes grad and returns DRRT_OK.  The workspace is not used.  fp32 only.               */
DRRT_API int drrt_backtrace_cable_opl_f32(const float* rif, size_t rres, float radius, float length, size_t n,
                             const float* pos, const float* xt, const float* vt, const uint32_t* rec_steps,
                             const float* dx, const float* dv, const float* dopl, float ds,
                             float* grad, float* dpos, float* dvel,
                             drrt_stats* stats, void* workspace, size_t workspace_bytes,
                             unsigned flags, void* stream);

/* drrt_trace_cable_f32 with the line integral of a second radial profile along every ray up to its record, and the
 * record's iteration (not in the reference): the group delay int N_g dl, an attenuation or gain int alpha dl.  xt, vt,
 * dist2 and the statistics are drrt_trace_cable_f32's bit for bit, rec_steps is drrt_trace_cable_opl_f32's.
 *   field      fp32[rres], the profile a on rif's knots (same radius); it may be rif itself (both are only read)
 *   tau        out: fp32[n], sum_{k<j} ds n_k a_k over the iterations in front of the record (x_j, v_j); n_k is the march's
 *              own unmasked sample at x_k and a_k the same lerp of `field` in the same cell (clamped beyond the radius
 *              like it), accumulated in fp32 in iteration order (fmaf(ds n_k, a_k, acc) from 0) and latched whenever the
 *              record is updated; j = 0 gives 0.  With field = rif it is drrt_trace_cable_opl_f32's opl bit for bit.  It is
 *              the integral of a along the path when the rays enter with |v| = n; rays scaled otherwise get the same sum,
 *              which is not that integral.
 *   rec_steps  out: uint32[n], j: what drrt_backtrace_cable_field_f32 takes, so that it replays nothing
 * The workspace and flags are not used.  fp32 only.                                                                  */
DRRT_API int drrt_trace_cable_field_f32(const float* rif, const float* field, size_t rres, float radius, float length,
                             size_t n, const float* pos, const float* vel, const float* target, float ds,
                             float* xt, float* vt, float* dist2, float* tau, uint32_t* rec_steps,
                             drrt_stats* stats, void* workspace, size_t workspace_bytes,
                             unsigned flags, void* stream);

/* The ONE adjoint of drrt_trace_cable_field_f32: dL/d(profile), dL/d(field), dL/dpos and dL/dvel from seeds on
 * (xt, vt, tau), the exact derivative of the discrete forward with the record's iteration held fixed.
 *   pos                the forward call's input positions, (n,3) fp32
 *   xt, vt, rec_steps  its outputs
 *   dx, dv, dtau       seeds on (xt, vt) ((n,3) fp32) and on tau (fp32[n]); each may be null: zeros
 *   grad, grad_field   out: fp32[rres] each, zeroed first unless DRRT_FLAG_NO_ZERO (then both are added into); null: not
 *                      computed; they must be two arrays
 *   dpos, dvel         out: (n,3) fp32; both null: not computed.  grad, grad_field, or dpos and dvel, must be asked for.
 * A ray makes rec_steps[i] reverse iterations from (xt, vt), run as drrt_backtrace_cable_opl_f32 runs them (lambda = dx,
 * mu = dv + ds dx, no backward-escape test, the last sample at pos itself).  In the cell (i0, i1, w0) of its sample an
 * iteration has dn = mu . grad n_k + dtau a_k and adds drrt_backtrace_cable_f32's two contributions for that dn to grad;
 * with fv = dtau ds n_k it adds fv (1 - w0) to grad_field[i0] and fv w0 to grad_field[i1], and lambda takes
 * fv a'_k rhat, a'_k = (field[i1] - field[i0]) / h, before it is carried into mu (a' is zero where grad n is: within
 * 1e-6 of the axis and beyond the radius).  With dtau null, grad, dpos and dvel are drrt_backtrace_cable_opl_f32's with
 * dopl null and grad_field is zero.  rec_steps = 0 gives (dx, dv) bit for bit and no contribution.  Nothing flows to
 * target, radius, length or ds, and dist2 takes no seed.
 * rec_steps is the only loop bound: a ray whose count exceeds the forward's own bound (int)(4 length / ds) -- no forward
 * call returns one -- makes no iterations, gets zero gradients and counts in stats->n_failed.  stats->ray_steps = the
 * reverse iterations.  n = 0 zeroes the requested gradients and returns DRRT_OK.  The workspace is not used.  fp32 only.
 * Up to 2048 profile samples with both gradients, 3072 with one and 4096 with none the block keeps the profiles and its
 * f64 gradient accumulators in LDS; above, it reads global memory and adds with global atomics.                      */
DRRT_API int drrt_backtrace_cable_field_f32(const float* rif, const float* field, size_t rres, float radius, float length,
                             size_t n, const float* pos, const float* xt, const float* vt, const uint32_t* rec_steps,
                             const float* dx, const float* dv, const float* dtau, float ds,
                             float* grad, float* grad_field, float* dpos, float* dvel,
                             drrt_stats* stats, void* workspace, size_t workspace_bytes,
                             unsigned flags, void* stream);

/* Ray-state adjoints of Tracer::trace_plane and Tracer::trace_sdf: dL/dpos, dL/dvel of the rays that entered
 * drrt_trace_pln_f32 / drrt_trace_sdf_f32 (the reference gets them from enoki autodiff through those marches,
 * core/tracer.py:122-234).  No contribution to dL/dn is formed.
 *   pos, vel       the forward call's inputs, (n,3) fp32;  pln_o, pln_d / sdf: its plane / signed-distance grid
 *   dx, dv         seeds on its outputs (xt, vt)
 *   dpos, dvel     out: (n,3) fp32
 * Contract: (xt, vt) is the state (x_j, v_j) after the LAST iteration j at which the ray went from inside to outside
 * (j = 0: the input itself), and iteration k is refracted only when the forward's `inside` flag m_k was set.  The forward
 * reports neither, so the call replays it from (pos, vel) with the forward's own fp32 operations -- both of its passes: every
 * ray until it is flagged escaped, then the rays whose record can still change over the call's global iteration count (the
 * maximum over its rays), see drrt_trace_pln_f32 -- and then undoes the iterations j-1 .. 0 from (xt, vt), seeded like
 * drrt_backtrace_f32 (lambda = dx, mu = dv + ds dx), with j and every m_k held fixed: a refracted iteration is one reverse
 * iteration of drrt_backtrace_f32 without its backward-escape test and step bound, a masked one is free flight (lambda
 * unchanged, mu += ds lambda).  The first sample of every refracted stretch is taken at the replayed position itself.
 * j = 0 gives (dx, dv) bit for bit.  trace_plane: a ray that never escaped (failmask set: xt is its final position, vt is
 * stale) gets a zero gradient and counts in stats->n_failed.  trace_sdf: a ray that never crosses keeps (xt, vt) = (pos, vel)
 * and gets (dx, dv); stats->n_failed = 0.  stats->ray_steps = replayed forward iterations + reverse iterations;
 * stats->iters = the replayed forward's global iteration count (drrt_trace_*'s own stats->iters).  The result does not
 * depend on DRRT_FLAG_CORRECTED_H nor on the visit order; no gradient flows to the plane, the SDF, h or ds.
 * Workspace: as for drrt_trace_sdf_f32 (n flag bytes behind the sort buffers; drrt_workspace_bytes() covers them).  Without
 * a stats block the library's per-device one carries the iteration count, as in drrt_trace_pln_f32.
 * Flags: DRRT_FLAG_SORT_RAYS (sorts the rays by their entry voxel), DRRT_FLAG_PAIR_GRID / _PAIR_REUSE and
 * DRRT_FLAG_DISPATCH_IN_ORDER as for drrt_trace_f32; the order hint (normally the paired forward's) is consumed like there,
 * the step hint is ignored.  fp32 only.                                                                                  */
DRRT_API int drrt_backtrace_pln_rays_f32(const float* rif, long long nvox, const int res[3], size_t n,
                             const float* pos, const float* vel, const float* pln_o, const float* pln_d,
                             const float* dx, const float* dv, float h, float ds,
                             float* dpos, float* dvel,
                             drrt_stats* stats, void* workspace, size_t workspace_bytes,
                             unsigned flags, void* stream);
DRRT_API int drrt_backtrace_sdf_rays_f32(const float* rif, const float* sdf, long long nvox, const int res[3], size_t n,
                             const float* pos, const float* vel,
                             const float* dx, const float* dv, float h, float ds,
                             float* dpos, float* dvel,
                             drrt_stats* stats, void* workspace, size_t workspace_bytes,
                             unsigned flags, void* stream);

/* Ray-state adjoint of Tracer::trace_target: dL/dpos, dL/dvel of the rays that entered drrt_trace_target_f32, from seeds on
 * all three of its outputs (the reference binds trace_target on its autodiff tracer, src/drrt.cpp:34).  No contribution to
 * dL/dn is formed.
 *   pos, vel, target   the forward call's inputs, (n,3) fp32
 *   dx, dv             seeds on its outputs (xt, vt);  ddist2: seed on dist2, fp32[n], or NULL for zero
 *   dpos, dvel         out: (n,3) fp32
 * Contract: (xt, vt) is the state (x_j, v_j) of the iteration j with the smallest squared distance to the target (first
 * minimum; j = 0 is the input itself) over the call's GLOBAL iteration count -- the maximum, over its rays, of the iterations
 * until a ray is flagged escaped: an escaped ray flies straight on while any ray marches -- and dist2 = |x_j - target|^2.
 * The forward reports neither j nor which iterations were refracted, so the call replays it from (pos, vel) with the
 * forward's own fp32 operations: a first launch for the global iteration count, a second for the replay and the reverse
 * march.  j and the forward's `inside` masks are held fixed.  The effective position seed is gx = dx + 2 ddist2 (x_j - target)
 * (one fmaf per component); j = 0 gives (gx, dv), which is (dx, dv) bit for bit when ddist2 is zero.  Otherwise the
 * iterations j-1 .. 0 are undone from the record, seeded like drrt_backtrace_f32 (lambda = gx, mu = dv + ds gx): a refracted
 * iteration is one reverse iteration of drrt_backtrace_f32 without its backward-escape test and step bound, a masked one --
 * the prefix before the first in-box sample, and everything after the ray was flagged escaped -- is free flight (lambda
 * unchanged, mu += ds lambda).  The first refracted sample is taken at the replayed position itself; a record written after
 * the escape starts the refracted stretch from the replayed state at the escape.  A ray that ran out of steps keeps its
 * record and its gradient; stats->n_failed counts the rays that never got flagged escaped, as drrt_trace_target_f32's.
 * stats->ray_steps = replayed forward iterations (second launch) + reverse iterations; stats->iters = the forward's own
 * stats->iters.  The result does not depend on DRRT_FLAG_CORRECTED_H nor on the visit order; no gradient flows to h or ds.
 * dL/dtarget = -2 ddist2 (xt - target) is a point-wise expression of the forward's outputs: the caller forms it.
 * Workspace: drrt_workspace_bytes() (drrt_workspace_bytes_grid() with DRRT_FLAG_PAIR_GRID); the call keeps no per-ray state
 * in it.  Without a stats block the library's per-device one carries the iteration count, as in drrt_trace_pln_f32.
 * Flags: DRRT_FLAG_SORT_RAYS, DRRT_FLAG_PAIR_GRID / _PAIR_REUSE and DRRT_FLAG_DISPATCH_IN_ORDER as for drrt_trace_f32; the
 * order hint (normally the paired forward's) is consumed like there, the step hint is ignored.  fp32 only.              */
DRRT_API int drrt_backtrace_target_rays_f32(const float* rif, long long nvox, const int res[3], size_t n,
                             const float* pos, const float* vel, const float* target,
                             const float* dx, const float* dv, const float* ddist2 /* nullable = 0 */,
                             float h, float ds, float* dpos, float* dvel,
                             drrt_stats* stats, void* workspace, size_t workspace_bytes,
                             unsigned flags, void* stream);

/* ---- sensor image splat (SURVEY.md 8.8 "next" row 1; the reference does this in torch) ----------
 * Forward: core/sensor.py:5-28 generate_sensor = trace_rays_to_plane (:195-202) + sensor frame
 * (t1 = n x t2, t2; get_tan_vecs :219-231 is evaluated by the caller) + foreshortening |v.n| +
 * Grid.Splat(average=False) with 4x4 tent taps (core/grid.py:37-64,77-81,133-151).
 *   x, v      (n,3) fp32 rays (normally the exit rays of drrt_trace_f32)
 *   e         per-ray energy fp32[n], or NULL to use e_scalar for every ray
 *   plane_p/n, t1, t2   HOST pointers to 3 floats each (one sensor plane per call, as in the reference)
 *   image     fp32[res*res], row-major image[ia*res + ib] with ia along t1; zeroed unless DRRT_FLAG_NO_ZERO
 * Backward: gradient of sum(grad_image * image) w.r.t. (x, v) -- what torch.autograd yields through
 * the reference's generate_sensor; grad_x, grad_v are (n,3) fp32 outputs (the seed of backtrace).  */
DRRT_API int drrt_sensor_splat_f32(size_t n, const float* x, const float* v, const float* e, float e_scalar,
                          const float plane_p[3], const float plane_n[3], const float t1[3], const float t2[3],
                          int res, float span, float* image, unsigned flags, void* stream);
DRRT_API int drrt_sensor_splat_bwd_f32(size_t n, const float* x, const float* v, const float* e, float e_scalar,
                              const float plane_p[3], const float plane_n[3], const float t1[3], const float t2[3],
                              int res, float span, const float* grad_image, float* grad_x, float* grad_v,
                              void* stream);

/* Far-field sensor: core/sensor.py:31-53 generate_inf_sensor (called at core/image_opt.py:116).  The image is a
 * histogram of the NORMALISED ray directions in the sensor frame: coordinates (vhat.t1, vhat.t2) + ang_cut with
 * ang_cut = sin(0.5 * deg2rad(angle_span)) computed by the caller (sensor.py:38), cell size 2*ang_cut/res, weight e
 * (no foreshortening), the same Grid.Splat.  Positions do not enter; the backward writes grad_x = 0.            */
DRRT_API int drrt_sensor_far_splat_f32(size_t n, const float* v, const float* e, float e_scalar, const float t1[3],
                              const float t2[3], int res, float ang_cut, float* image, unsigned flags, void* stream);
DRRT_API int drrt_sensor_far_splat_bwd_f32(size_t n, const float* v, const float* e, float e_scalar, const float t1[3],
                                  const float t2[3], int res, float ang_cut, const float* grad_image,
                                  float* grad_x, float* grad_v, void* stream);

/* core/sensor.py:102-138 get_sdf_vals_near (mode 0) / get_sdf_vals_far (mode 1): Grid(tex, h).Get at the rays' sensor
 * coordinates -- the 4x4 radial-tent interpolant of core/grid.py:100-124, tap indices clipped to the (res, res) texture
 * (edge extrapolation off the texture, as in the reference) -- and its analytic backward w.r.t. the rays.  mode 0: rays ->
 * plane -> sensor frame, cell size span / res; mode 1: coordinates v . T + span / 2 from the direction as it is (pass
 * span = 2 * ang_cut).  tex, f_out, grad_f: device fp32; the plane and the tangents are host float[3].              */
DRRT_API int drrt_sensor_tex_get_f32(size_t n, const float* x, const float* v, const float plane_p[3], const float plane_n[3],
                            const float t1[3], const float t2[3], const float* tex, int res, float span, int mode,
                            float* f_out, void* stream);
DRRT_API int drrt_sensor_tex_get_bwd_f32(size_t n, const float* x, const float* v, const float plane_p[3],
                                const float plane_n[3], const float t1[3], const float t2[3], const float* tex, int res,
                                float span, int mode, const float* grad_f, float* grad_x, float* grad_v, void* stream);

/* The same six sensor operators with the sensor frame in DEVICE memory: frame12 = 12 fp32 values (plane_p, plane_n, t1, t2;
 * the far-field entries read t1, t2 only).  The reference keeps its planes as torch tensors on the device (core/image_opt.py
 * :88-119 slices them from the ray generator's output), so a caller of the host-pointer entries above has to copy them back
 * first -- a device synchronisation per call.  These entries need none; results are identical.                            */
DRRT_API int drrt_sensor_splat_dframe_f32(size_t n, const float* x, const float* v, const float* e, float e_scalar,
                                 const float* frame12, int res, float span, float* image, unsigned flags, void* stream);
DRRT_API int drrt_sensor_splat_dframe_bwd_f32(size_t n, const float* x, const float* v, const float* e, float e_scalar,
                                     const float* frame12, int res, float span, const float* grad_image, float* grad_x,
                                     float* grad_v, void* stream);
DRRT_API int drrt_sensor_far_splat_dframe_f32(size_t n, const float* v, const float* e, float e_scalar, const float* frame12,
                                     int res, float ang_cut, float* image, unsigned flags, void* stream);
DRRT_API int drrt_sensor_far_splat_dframe_bwd_f32(size_t n, const float* v, const float* e, float e_scalar,
                                         const float* frame12, int res, float ang_cut, const float* grad_image,
                                         float* grad_x, float* grad_v, void* stream);
DRRT_API int drrt_sensor_tex_get_dframe_f32(size_t n, const float* x, const float* v, const float* frame12, const float* tex,
                                   int res, float span, int mode, float* f_out, void* stream);
DRRT_API int drrt_sensor_tex_get_dframe_bwd_f32(size_t n, const float* x, const float* v, const float* frame12,
                                       const float* tex, int res, float span, int mode, const float* grad_f,
                                       float* grad_x, float* grad_v, void* stream);

/* Radiance splats: a per-ray, PER-CHANNEL energy rad (n, channels) fp32, 1 <= channels <= 32, splatted onto an image
 * (channels, res, res); channel c is drrt_sensor_splat_f32 / drrt_sensor_far_splat_f32 with e = rad[:, c] (same plane
 * intersection, frame, taps, normalisation over all 16 taps, foreshortening |v.n| in the near field only).  The channels
 * of a ray share its landing point and its 16 weights.  DRRT_FLAG_NO_ZERO holds for all channels*res*res floats.
 * Backward: gradient of sum(grad_image * image), grad_image (channels, res, res), w.r.t. rad (grad_rad, (n, channels)) and
 * the rays (grad_x, grad_v, (n,3)); each of the three outputs may be NULL and is then not computed (all three NULL: nothing
 * is launched).  A ray that misses the image gets zeros.  The far-field entries write zeros to a non-NULL grad_x.
 * `_dframe`: the frame as 12 device floats, as above.                                                                   */
DRRT_API int drrt_sensor_radiance_f32(size_t n, const float* x, const float* v, const float* rad, int channels,
                             const float plane_p[3], const float plane_n[3], const float t1[3], const float t2[3],
                             int res, float span, float* image, unsigned flags, void* stream);
DRRT_API int drrt_sensor_radiance_bwd_f32(size_t n, const float* x, const float* v, const float* rad, int channels,
                                 const float plane_p[3], const float plane_n[3], const float t1[3], const float t2[3],
                                 int res, float span, const float* grad_image, float* grad_rad, float* grad_x,
                                 float* grad_v, void* stream);
DRRT_API int drrt_sensor_radiance_dframe_f32(size_t n, const float* x, const float* v, const float* rad, int channels,
                                    const float* frame12, int res, float span, float* image, unsigned flags, void* stream);
DRRT_API int drrt_sensor_radiance_dframe_bwd_f32(size_t n, const float* x, const float* v, const float* rad, int channels,
                                        const float* frame12, int res, float span, const float* grad_image,
                                        float* grad_rad, float* grad_x, float* grad_v, void* stream);
DRRT_API int drrt_sensor_radiance_far_f32(size_t n, const float* v, const float* rad, int channels, const float t1[3],
                                 const float t2[3], int res, float ang_cut, float* image, unsigned flags, void* stream);
DRRT_API int drrt_sensor_radiance_far_bwd_f32(size_t n, const float* v, const float* rad, int channels, const float t1[3],
                                     const float t2[3], int res, float ang_cut, const float* grad_image,
                                     float* grad_rad, float* grad_x, float* grad_v, void* stream);
DRRT_API int drrt_sensor_radiance_far_dframe_f32(size_t n, const float* v, const float* rad, int channels,
                                        const float* frame12, int res, float ang_cut, float* image, unsigned flags,
                                        void* stream);
DRRT_API int drrt_sensor_radiance_far_dframe_bwd_f32(size_t n, const float* v, const float* rad, int channels,
                                            const float* frame12, int res, float ang_cut, const float* grad_image,
                                            float* grad_rad, float* grad_x, float* grad_v, void* stream);

/* core/sensor.py:195-202 trace_rays_to_plane, the statement right after the march in every experiment: x_out = x + t v with
 * t = n.(p - x) / n.v (v passes through unchanged), and its analytic backward w.r.t. the rays (grad_x, grad_v receive the
 * part of the gradient that flows through x_out).  plane_stride 3 = one (p, n) per ray, 0 = one plane for all rays.
 * All pointers are device pointers to fp32 (n,3) row-major arrays (planes: (n,3) or (1,3)).                        */
DRRT_API int drrt_rays_to_plane_f32(size_t n, const float* x, const float* v, const float* plane_p, const float* plane_n,
                           int plane_stride, float* x_out, void* stream);
DRRT_API int drrt_rays_to_plane_bwd_f32(size_t n, const float* x, const float* v, const float* plane_p, const float* plane_n,
                               int plane_stride, const float* grad_x_out, float* grad_x, float* grad_v, void* stream);

/* ---- multires up-sampling (SURVEY.md 8.8 "next" row 3) --------------------------------------------
 * core/optimizer.py:7-10 upres_scene / core/grid.py:318-330 upres_volume: trilinear resampling of a
 * cubic (R,R,R) fp32 volume at linspace(0,1,S) per axis, evaluated in float64 like the reference and
 * rounded to fp32.  Shapes are HOST pointers to 3 ints in torch order.                            */
DRRT_API int drrt_upres_volume_f32(const float* src, const int src_shape[3], float* dst, const int dst_shape[3],
                          void* stream);

/* core/optimizer.py:57-69, the tail of one multires_opt iteration in ONE pass over the volume: the boundary-gradient
 * mask `n.grad[mask] = 0` (mask = outermost voxel layer, :54-55), `opto.step()` of torch.optim.Adam (amsgrad = maximize
 * = False; formula of torch/optim/adam.py) and `n.clamp_(min=1)`.  All four arrays are DEVICE fp32 arrays of
 * shape[0]*shape[1]*shape[2] elements (torch order, last axis fastest), updated in place (grad: zeroed on the boundary
 * layer, like the reference).  `step` is the step count AFTER this update's increment (1 for the first call); lr, betas,
 * eps, weight_decay are the param group's values.                                                                  */
#define DRRT_ADAM_MASK_BOUNDARY 1u  /* treat the gradient of the outermost voxel layer as 0 (and zero it in `grad`) */
#define DRRT_ADAM_CLAMP_MIN     2u  /* clamp the updated parameter from below at clamp_min                          */
DRRT_API int drrt_adam_step_f32(float* param, float* grad, float* exp_avg, float* exp_avg_sq, const int shape[3],
                       double step, double lr, double beta1, double beta2, double eps, double weight_decay,
                       double clamp_min, unsigned flags, void* stream);

/* ---- ray generation (SURVEY.md 8.8 "next" row 2) ---------------------------------------------------
 * kind 0: core/source.py:54-69 plane_source3_rand + :275-293 rotate_pts_to_source;
 * kind 1: :72-104 point_source3_rand -- for n_views views in one call (what :352-357 rand_rays_in_sphere,
 * :360-365 rand_ptrays_in_sphere and :398-412 rand_rays_cube concatenate), optionally followed by
 * :555-563 random_rotate_ic.  All pointers are DEVICE pointers except ic_rot.
 *   u          fp32[n_views][2*spp][p0][p1] uniforms in [0,1) (the reference's torch.rand draws)
 *   view_rot   fp32[n_views][9] row-major rotate_ray3 matrix of each view (:303-312)
 *   width, sensor_dist, span   python scalars of the reference (doubles, rounded to fp32 where the
 *              reference's tensors are fp32)
 *   circle     keep only points with r < width/2 (order-preserving compaction, :277-280 / :81-92)
 *   independent  kind 0 only: :60-63 instead of the jittered pixel grid
 *   ic_rot     HOST pointer to 9 floats (row-major M) or NULL: x' = M (x - span/2) + span/2 etc.
 *   x, v       fp32[cap][3], planes fp32[cap][3][3] with cap = n_views*spp*p0*p1; kept rays are
 *              written densely in the reference's order (view, sample, pixel row, pixel column)
 *   view_counts  int32[n_views+1]: exclusive prefix of kept rays per view, [n_views] = total
 *   workspace  drrt_gen_workspace_bytes(...) bytes of device scratch                                */
#define DRRT_SOURCE_PLANE 0
#define DRRT_SOURCE_POINT 1
DRRT_API size_t drrt_gen_workspace_bytes(int n_views, int spp, int p0, int p1);
DRRT_API int drrt_gen_rays_f32(int kind, const float* u, const float* view_rot, int n_views, int spp, int p0, int p1,
                      double width, double sensor_dist, int circle, int independent,
                      const float* ic_rot, double span, float* x, float* v, float* planes,
                      int* view_counts, void* workspace, size_t workspace_bytes, void* stream);
/* Cone source: core/source.py:186-203 cone_source3_rand (the fibre experiment's source, core/fiber_opt.py:131) --
 * spp*p0*p1 rays per view from the point R (0, -width/2, 0) + width/2 with directions drawn by hatbox_sample
 * (:531-545) in a cone of full angle cone_angle about R e_y.  `u` holds, per view, the two uniform draws of
 * hatbox_sample: u[view][0][c] for z, u[view][1][c] for theta, c < spp*p0*p1.  cone_cos = cos(cone_angle / 2) as the
 * reference evaluates it (fp32, :533-534).  No disc mask: every candidate is a ray.                              */
DRRT_API int drrt_gen_cone_rays_f32(const float* u, const float* view_rot, int n_views, int spp, int p0, int p1,
                           double width, double sensor_dist, double cone_cos, const float* ic_rot_host, double span,
                           float* x, float* v, float* planes, int* view_counts, void* workspace,
                           size_t workspace_bytes, void* stream);

/* ---- profiling aid (bench.py; no counterpart in the reference) --------------------------------
 * After drrt_profile_begin(capacity) every march call records a HIP event pair on its stream
 * around each kernel it launches (no synchronisation).  drrt_profile_collect() waits for the
 * recorded events, writes up to max_out (kernel id, milliseconds) pairs in launch order, resets
 * the log and returns the count.  Single-threaded use only.                                    */
#define DRRT_PROF_TRACE      1   /* forward march kernel                 */
#define DRRT_PROF_BACKTRACE  2   /* adjoint march kernel                 */
#define DRRT_PROF_SORT       3   /* entry-voxel keys + radix sort        */
#define DRRT_PROF_ZERO       4   /* zero-fill of the gradient grid       */
#define DRRT_PROF_QUAD       5   /* build of the pair copy of the grid   */
#define DRRT_PROF_BACKTRACE_RAYS 6   /* ray-state adjoint (drrt_backtrace_rays_f32) */
#define DRRT_PROF_BACKTRACE_CABLE_RAYS 7   /* ray-state adjoint of the cable march (drrt_backtrace_cable_rays_f32) */
#define DRRT_PROF_BACKTRACE_PLN_RAYS 8   /* ray-state adjoint of trace_plane (drrt_backtrace_pln_rays_f32), both passes */
#define DRRT_PROF_BACKTRACE_SDF_RAYS 9   /* ray-state adjoint of trace_sdf (drrt_backtrace_sdf_rays_f32), both passes */
#define DRRT_PROF_BACKTRACE_TARGET_RAYS 10   /* ray-state adjoint of trace_target (drrt_backtrace_target_rays_f32), both launches */
#define DRRT_PROF_TRACE_OPL 11       /* trace with its optical path length (drrt_trace_opl_f32) */
#define DRRT_PROF_BACKTRACE_OPL 12   /* its adjoint: dL/dn and the ray gradients in one march (drrt_backtrace_opl_f32) */
#define DRRT_PROF_TRACE_FIELD 13     /* trace with the line integral of a second field (drrt_trace_field_f32) */
#define DRRT_PROF_BACKTRACE_FIELD 14 /* its adjoint: dL/dn, dL/dfield and the ray gradients in one march (drrt_backtrace_field_f32) */
#define DRRT_PROF_TRACE_EMISSION 15  /* trace with the emission integral of two further fields (drrt_trace_emission_f32) */
#define DRRT_PROF_BACKTRACE_EMISSION 16 /* its adjoint: dL/dn, dL/de, dL/da and the ray gradients in one march (drrt_backtrace_emission_f32) */
#define DRRT_PROF_TRACE_VECTOR 17    /* trace with the line integral of a vector field (drrt_trace_vector_f32) */
#define DRRT_PROF_BACKTRACE_VECTOR 18 /* its adjoint: dL/dn, dL/du and the ray gradients in one march (drrt_backtrace_vector_f32) */
#define DRRT_PROF_TRACE_CABLE_OPL 19 /* the cable march with its optical path length (drrt_trace_cable_opl_f32) */
#define DRRT_PROF_BACKTRACE_CABLE_OPL 20 /* its adjoint: dL/d(profile) and the ray gradients in one march (drrt_backtrace_cable_opl_f32) */
#define DRRT_PROF_TRACE_CABLE_FIELD 21 /* the cable march with the line integral of a second radial profile (drrt_trace_cable_field_f32) */
#define DRRT_PROF_BACKTRACE_CABLE_FIELD 22 /* its adjoint: dL/d(profile), dL/d(field) and the ray gradients in one march (drrt_backtrace_cable_field_f32) */
#define DRRT_PROF_TRACE_PATH 23      /* trace with every stride-th position of every ray (drrt_trace_path_f32) */
#define DRRT_PROF_BACKTRACE_PATH 24  /* its adjoint: dL/dn and the ray gradients in one march (drrt_backtrace_path_f32) */
#define DRRT_PROF_TRACE_PHASE 25     /* trace with every stride-th position AND velocity of every ray (drrt_trace_phase_f32) */
#define DRRT_PROF_BACKTRACE_PHASE 26 /* its adjoint: dL/dn and the ray gradients in one march (drrt_backtrace_phase_f32) */
DRRT_API int  drrt_profile_begin(int capacity);
DRRT_API int  drrt_profile_collect(int* kernel_ids, float* ms, int max_out);
DRRT_API void drrt_profile_end(void);

#ifdef __cplusplus
}
#endif
#endif /* DRRT_HIP_H */
