// drrt_api.hip -- the C ABI of include/drrt_hip.h: argument checks (the reference's three error messages verbatim,
// src/volume.cpp:28,37,124), workspace layout (ws_layout), visit-order / step hand-over (ThreadState), per-kernel timing,
// and the launches of the kernels in drrt_forward.hip / drrt_adjoint_box.hip / drrt_adjoint_ring.hip /
// drrt_ray_adjoints.hip / drrt_integral.hip / drrt_cable.hip.  Host code, plus the
// four small utility kernels that belong to no march (pair copy of the grid, q16 encode / decode, chunk progress reset).
#include "drrt_host.h"
#include "drrt_march.h"

using namespace drrt;

// from drrt_sort.hip
namespace drrt {
size_t sort_workspace_bytes(size_t n);
hipError_t sort_rays_by_entry_voxel(const Vol& V, float h, size_t n, const void* pos, const void* vel, int io_half,
                                    float dir_sign, void* ws, size_t ws_bytes, const uint32_t** perm_out,
                                    hipStream_t stream, bool chord_key);
}

static thread_local char g_err[512] = "";

int drrt::fail(int code, const char* msg) {
  snprintf(g_err, sizeof(g_err), "%s", msg);
  return code;
}
int drrt::fail_hip(hipError_t e, const char* where) {
  snprintf(g_err, sizeof(g_err), "%s: %s", where, hipGetErrorString(e));
  return DRRT_ERR_HIP;
}

extern "C" const char* drrt_last_error(void) { return g_err; }

// ---- visit-order / step / counter hand-over between paired calls (per host thread) -----------
struct OrderHint { const uint32_t* order; size_t n; const uint32_t* steps; size_t steps_n; };
struct ThreadState {
  const uint32_t* last_order = nullptr;     // order used by the last sorted call (maybe_sort)
  const uint32_t* last_steps = nullptr;     // per-ray iteration counts written by the last forward march
  size_t last_order_n = 0, last_steps_n = 0;
  const unsigned* last_counters = nullptr;  // bundle classification of the last adjoint call (device, in its workspace)
  OrderHint hint{};                         // order and steps for the NEXT march call
  // Every march entry point takes (reads AND clears) the hint as its FIRST statement -- by making its GridCall or calling
  // cable_begin --, so no return path, validation failure included, can leave a stale device pointer armed for a later call.
  OrderHint take_hint() { const OrderHint h = hint; hint = OrderHint{}; return h; }
  // one reset point per kind of call: a forward march forgets the iteration counts of the one before it (trace / trace_pln
  // once they are about to launch, the marches that write none at their entry), a dL/dn adjoint the last classification
  void reset_last_steps() { last_steps = nullptr; last_steps_n = 0; }
  void reset_last_counters() { last_counters = nullptr; }
};
static thread_local ThreadState g_ts;

extern "C" const uint32_t* drrt_last_order(size_t* n_out) {
  if (n_out) *n_out = g_ts.last_order_n;
  return g_ts.last_order;
}
extern "C" void drrt_set_order_hint(const uint32_t* order, size_t n) { g_ts.hint.order = order; g_ts.hint.n = order ? n : 0; }
extern "C" size_t drrt_order_hint_pending(void) { const OrderHint& h = g_ts.hint; return h.order ? h.n : (h.steps ? h.steps_n : 0); }
extern "C" const uint32_t* drrt_last_steps(size_t* n_out) {
  if (n_out) *n_out = g_ts.last_steps_n;
  return g_ts.last_steps;
}
extern "C" void drrt_set_step_hint(const uint32_t* steps, size_t n) { g_ts.hint.steps = steps; g_ts.hint.steps_n = steps ? n : 0; }
extern "C" const unsigned* drrt_last_bundle_counters(void) { return g_ts.last_counters; }
extern "C" int drrt_ring_threshold_pct(void) { return DRRT_RING_MIN_NOFIT_PCT; }
extern "C" int drrt_ring_long_threshold_permille(void) { return DRRT_RING_MIN_LONG_PERMILLE; }
extern "C" int drrt_ring_direct_threshold_pct(void) { return DRRT_RING_DIRECT_MAX_PAIR_PCT; }

// ---- optional per-kernel timing (bench / profiling aid; not thread-safe) --------------------
// Event pairs are recorded on the call's stream right around a kernel launch; nothing
// synchronises until drrt_profile_collect().
struct ProfRec { hipEvent_t a, b; int id; };
static ProfRec* g_prof = nullptr;
static int g_prof_cap = 0, g_prof_n = 0;

struct ProfScope {
  int slot; hipStream_t s;
  ProfScope(int id, hipStream_t st) : slot(-1), s(st) {
    if (g_prof && g_prof_n < g_prof_cap) {
      slot = g_prof_n++;
      g_prof[slot].id = id;
      (void)hipEventRecord(g_prof[slot].a, s);
    }
  }
  ~ProfScope() { if (slot >= 0) (void)hipEventRecord(g_prof[slot].b, s); }
};

extern "C" void drrt_profile_end(void) {
  for (int i = 0; i < g_prof_cap; ++i) { (void)hipEventDestroy(g_prof[i].a); (void)hipEventDestroy(g_prof[i].b); }
  delete[] g_prof; g_prof = nullptr; g_prof_cap = g_prof_n = 0;
}

extern "C" int drrt_profile_begin(int capacity) {
  drrt_profile_end();
  if (capacity <= 0) return DRRT_OK;
  g_prof = new ProfRec[capacity];
  for (int i = 0; i < capacity; ++i) {
    hipError_t e = hipEventCreate(&g_prof[i].a);
    if (e == hipSuccess) e = hipEventCreate(&g_prof[i].b);
    if (e != hipSuccess) { g_prof_cap = i; drrt_profile_end(); return fail_hip(e, "hipEventCreate"); }
  }
  g_prof_cap = capacity; g_prof_n = 0;
  return DRRT_OK;
}

extern "C" int drrt_profile_collect(int* ids, float* ms, int max_out) {
  int n = g_prof_n < max_out ? g_prof_n : max_out;
  for (int i = 0; i < n; ++i) {
    (void)hipEventSynchronize(g_prof[i].b);
    float t = 0.f;
    (void)hipEventElapsedTime(&t, g_prof[i].a, g_prof[i].b);
    ids[i] = g_prof[i].id; ms[i] = t;
  }
  g_prof_n = 0;
  return n;
}
#ifndef DRRT_SRC_ID
#define DRRT_SRC_ID "unknown"
#endif
// "drrt_hip <abi> gfx950 src:<digest of the sources, csrc/Makefile>"
extern "C" const char* drrt_version(void) { return "drrt_hip 0.3 gfx950 src:" DRRT_SRC_ID; }

static inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// ---- the workspace: one caller-owned device buffer, laid out here and nowhere else -------------------------------------
//   every call but trace_target   [ sort buffers | per-ray slot ][ pair copy of the grid ][ counters, 512 B ]
//   trace_target                  [ per-ray slot | sort buffers ][ pair copy of the grid ][ counters, 512 B ]
//                                 |<-- drrt_workspace_bytes() -->|
//                                 |<------------------- drrt_workspace_bytes_grid() ---------------------->|
// sort buffers  keys, indices and the sort's own scratch (split by drrt_sort.hip); the visit order the sort leaves,
//               drrt_last_order(), lies in here.  Padded to 256 B; none without DRRT_FLAG_SORT_RAYS.
// per-ray slot  n * 7 floats padded to 256 B, always counted.  ONE slot with three tenants, one per call: the iteration
//               counts of trace / trace_pln (n uint32, drrt_last_steps(); written where the buffer has room), the
//               second-pass flags of trace_sdf and of the plane / SDF ray adjoints (n bytes), and the phase-A state of
//               trace_target (n * 7 floats).  Safe, because flags and state live and die inside their call, and the one
//               tenant that outlives its call, the iteration counts, is only ever a hint: a forward march forgets the
//               pointer (reset_last_steps) before it writes the slot, and an adjoint handed counts that another call has
//               overwritten since loses speed, never a result (include/drrt_hip.h, "step hint").
// trace_target  keeps its state FIRST and the sort buffers behind it, as it always has: drrt_last_order() after it points
//               behind the slot, and bindings look for it there.
// pair copy     8 B per voxel (k_build_pair) with DRRT_FLAG_PAIR_GRID, at a multiple of 256 B.
// counters      the last 512 B of a drrt_workspace_bytes_grid() buffer; the select counters of the bundle classification
//               (32 B, drrt_last_bundle_counters()) sit 256 B into the block.
// debug counters (DRRT_FLAG_DEBUG_COUNTERS)  512 B that END, 8-aligned, where the caller's buffer ends, whatever its size:
//               in a buffer of exactly drrt_workspace_bytes_grid() bytes they are the counter block.
// A new region is a pair of fields here and a line in ws_layout.
constexpr size_t kCtrBytes = 512;
struct WsLayout {
  size_t sort_off, sort_bytes, sort_need;   // sort_need: what the sort uses of its padded region
  size_t slot_off, slot_bytes;
  size_t ray_bytes;                         // sort + slot: drrt_workspace_bytes()
  size_t pair_off, pair_bytes;
  size_t ctr_off, select_off;               // the counter block, and the select counters in it
  size_t grid_bytes;                        // everything: drrt_workspace_bytes_grid()
  size_t dbg_off;                           // from ws_bytes (0 when that is below kCtrBytes)
};
static WsLayout ws_layout(size_t n, long long nvox, unsigned flags, size_t ws_bytes, bool target_order = false) {
  WsLayout L{};
  if (flags & DRRT_FLAG_SORT_RAYS) { L.sort_need = sort_workspace_bytes(n); L.sort_bytes = align_up(L.sort_need, 256); }
  L.slot_bytes = align_up(n * 7 * sizeof(float), 256);
  L.sort_off = target_order ? L.slot_bytes : 0;
  L.slot_off = target_order ? 0 : L.sort_bytes;
  L.pair_off = L.ray_bytes = L.sort_bytes + L.slot_bytes;
  L.pair_bytes = ((flags & DRRT_FLAG_PAIR_GRID) && nvox > 0) ? (size_t)nvox * 2 * sizeof(float) : 0;
  L.ctr_off = L.pair_off + L.pair_bytes;
  L.select_off = L.ctr_off + 256;
  L.grid_bytes = L.ctr_off + kCtrBytes;
  L.dbg_off = ws_bytes >= kCtrBytes ? ((ws_bytes - kCtrBytes) & ~(size_t)7) : 0;
  return L;
}

extern "C" size_t drrt_workspace_bytes(size_t n, unsigned flags) { return ws_layout(n, 0, flags, 0).ray_bytes; }
extern "C" size_t drrt_workspace_bytes_grid(size_t n, long long nvox, unsigned flags) { return ws_layout(n, nvox, flags, 0).grid_bytes; }

namespace drrt {
// pair[2 i] = n[i], pair[2 i + 1] = n[i + W] (the y-neighbour, clamped at the far y face -- those entries are never
// read: only strictly interior cells use the copy).  One thread per voxel, 4 + 8 B of traffic each.
__global__ void __launch_bounds__(256) k_build_pair(const float* __restrict__ g, float2* __restrict__ q, int W, int H,
                                                    unsigned nvox) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  if (i >= nvox) return;
  const unsigned row = i / (unsigned)W, y = row % (unsigned)H;
  const unsigned y1 = (y + 1u < (unsigned)H) ? (unsigned)W : 0u;
  q[i] = make_float2(g[i], g[i + y1]);
}
}  // namespace drrt

// volume ctor checks: src/volume.cpp:31-38 (size) and :123-124 (width/height >= 2)
static int check_steps(float h, float ds) {
  // the reference divides by ds and truncates to int (src/tracer.cpp:51): a non-positive or non-finite
  // step would make that undefined; refuse it instead
  if (!(h > 0.f) || !(ds > 0.f) || !(h < 3.0e38f) || !(ds < 3.0e38f))
    return fail(DRRT_ERR_ARG, "h and ds must be positive and finite");
  return DRRT_OK;
}

static int make_vol(const float* rif, long long nvox, const int res[3], float h, Vol* V) {
  if (!rif || !res) return fail(DRRT_ERR_ARG, "null rif/res pointer");
  if ((long long)res[0] * res[1] * res[2] != nvox || nvox <= 0)
    return fail(DRRT_ERR_RES_MISMATCH, "Resolution doesn't match data");
  if (!(res[0] == 1 && res[1] == 1 && res[2] == 1) && (res[0] < 2 || res[1] < 2))
    return fail(DRRT_ERR_BAD_RES, "volume: invalid resolution!");
  if (nvox >= (1LL << 29)) return fail(DRRT_ERR_ARG, "grid too large (>= 2^29 voxels) for 32-bit byte offsets");
  if (res[0] >= (1 << 24) || res[1] >= (1 << 24) || res[2] >= (1 << 24) || (long long)res[0] * res[1] >= (1 << 24))
    return fail(DRRT_ERR_ARG, "grid extents too large for 24-bit index arithmetic");
  if (!(h > 0.f) || !(h < 3.0e38f)) return fail(DRRT_ERR_ARG, "h and ds must be positive and finite");
  V->data = rif; V->W = res[0]; V->H = res[1]; V->D = res[2];
  vol_finish(*V, h);
  return DRRT_OK;
}

static inline int max3(const int r[3]) { return r[0] > r[1] ? (r[0] > r[2] ? r[0] : r[2]) : (r[1] > r[2] ? r[1] : r[2]); }

// float expression truncated to int, exactly as written in the reference (Q5)
static inline int steps_fwd(float h, const int res[3], float ds)  { return (int)(4.0f * h * (float)max3(res) / ds); }
static inline int steps_sdf(float h, const int res[3], float ds)  { return (int)(2.0f * h * (float)max3(res) / ds); }
static inline int steps_adj(float h, const int res[3], float ds)  { return (int)(2.0f * h * (float)max3(res) / ds); }

static int zero_stats(drrt_stats* stats, hipStream_t s) {
  if (!stats) return DRRT_OK;
  hipError_t e = hipMemsetAsync(stats, 0, sizeof(drrt_stats), s);
  return e == hipSuccess ? DRRT_OK : fail_hip(e, "hipMemsetAsync(stats)");
}

#define LAUNCH_CHECK(where)                                              \
  do { hipError_t e_ = hipGetLastError(); if (e_ != hipSuccess) return fail_hip(e_, where); } while (0)

// the tail of an entry that launches one kernel family: the launch inside its profile record, then the launch check
template <class Launch>
static int timed_launch(int prof_id, hipStream_t s, const char* where, Launch launch) {
  {
    ProfScope prof(prof_id, s);
    launch();
  }
  LAUNCH_CHECK(where);
  return DRRT_OK;
}

// The second pass of trace_pln / trace_sdf and of their ray-state adjoints needs the global loop count of the first: a
// library-owned stats block, one per device (allocated once), for callers that pass none.  It is shared by every stream of
// that device: callers that run such calls concurrently on several streams of one device must pass their own stats block.
static int private_stats(drrt_stats** stats) {
  constexpr int kMaxDev = 64;
  static drrt_stats* priv[kMaxDev] = {};
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return fail_hip(e, "hipGetDevice");
  if (dev < 0 || dev >= kMaxDev) return fail(DRRT_ERR_ARG, "device ordinal out of range; pass a stats block");
  if (!priv[dev]) { e = hipMalloc((void**)&priv[dev], sizeof(drrt_stats)); if (e != hipSuccess) return fail_hip(e, "hipMalloc(stats)"); }
  *stats = priv[dev];
  return DRRT_OK;
}

// ---- the prologue the grid marches share ------------------------------------------------------------------------------
// An entry point makes its GridCall first (that takes the hint and clears the error message), then runs the shared steps
// in this order, with the checks that are its own in between: open() -- grid and steps --, check_ray_count() after its
// null-pointer checks, place() -- visit order (hint or sort), pair copy, dispatch order: all that touches the workspace.
struct GridCall {
  OrderHint hint = g_ts.take_hint();
  Vol& vol;                       // the argument block's
  hipStream_t s;
  float h = 0.f;
  const uint32_t* perm = nullptr;
  int xcd_order = 0;              // 1: the launch's blocks take the visit order XCD by XCD
  GridCall(Vol& v, void* stream) : vol(v), s((hipStream_t)stream) { g_err[0] = 0; }

  int open(const float* rif, long long nvox, const int res[3], float h_, float ds) {
    h = h_;
    const int rc = make_vol(rif, nvox, res, h, &vol);
    return rc ? rc : check_steps(h, ds);
  }
  // `key_pos`, `key_vel`, `dir_sign`: the rays the sort keys are made from, and which way they head
  int place(long long nvox, size_t n, const void* key_pos, const void* key_vel, float dir_sign, unsigned flags,
            const WsLayout& L, void* ws, size_t ws_bytes, int io_half = 0) {
    // A hint from the caller (normally the paired forward call's order) replaces the sort; it was consumed when this call
    // began whether or not it is usable.  Entries are range-checked on the device (ray_index), so a wrong hint can leave
    // rays unvisited but cannot make a kernel fault.
    if (hint.order && hint.n == n) {
      perm = hint.order;
    } else if ((flags & DRRT_FLAG_SORT_RAYS) && n >= 2) {
      // (a caller whose sort buffers do not start the workspace -- trace_target -- has checked that it reaches them)
      if (!ws || ws_bytes - L.sort_off < L.sort_need) return fail(DRRT_ERR_ARG, "workspace too small for DRRT_FLAG_SORT_RAYS");
      ProfScope prof(DRRT_PROF_SORT, s);
      hipError_t e = sort_rays_by_entry_voxel(vol, h, n, key_pos, key_vel, io_half, dir_sign, (char*)ws + L.sort_off,
                                              ws_bytes - L.sort_off, &perm, s, (flags & DRRT_FLAG_CHORD_KEY) != 0);
      if (e != hipSuccess) return fail_hip(e, "sort_rays_by_entry_voxel");
      g_ts.last_order = perm; g_ts.last_order_n = n;
    }
    xcd_order = (perm != nullptr && !(flags & DRRT_FLAG_DISPATCH_IN_ORDER)) ? 1 : 0;
    // DRRT_FLAG_PAIR_GRID: the pair copy of the grid, built here unless DRRT_FLAG_PAIR_REUSE
    if (!(flags & DRRT_FLAG_PAIR_GRID)) return DRRT_OK;
    if (!ws || ws_bytes < L.grid_bytes) return fail(DRRT_ERR_ARG, "workspace too small for DRRT_FLAG_PAIR_GRID (see drrt_workspace_bytes_grid)");
    if (((uintptr_t)ws + L.pair_off) % 16 != 0) return fail(DRRT_ERR_ARG, "workspace must be 16-byte aligned for DRRT_FLAG_PAIR_GRID");
    float2* q = (float2*)((char*)ws + L.pair_off);
    if (!(flags & DRRT_FLAG_PAIR_REUSE)) {
      ProfScope prof(DRRT_PROF_QUAD, s);
      hipLaunchKernelGGL(drrt::k_build_pair, dim3((unsigned)(((size_t)nvox + 255) / 256)), dim3(256), 0, s, vol.data, q, vol.W,
                         vol.H, (unsigned)nvox);
      LAUNCH_CHECK("k_build_pair");
    }
    vol.pair = (const float*)q;
    return DRRT_OK;
  }
  void drop_order() { perm = nullptr; xcd_order = 0; }
};
static int check_ray_count(size_t n) {
  return n > 0xffffffffULL ? fail(DRRT_ERR_ARG, "too many rays for uint32 permutation") : DRRT_OK;
}

template <int MODE>
static int run_trace(const float* rif, const float* sdf, long long nvox, const int res[3], size_t n,
                     const void* pos, const void* vel, const float* pln_o, const float* pln_d,
                     float h, float ds, void* xt, void* vt, uint8_t* failmask, drrt_stats* stats,
                     void* ws, size_t ws_bytes, unsigned flags, void* stream, int io_half = 0) {
  TraceArgs a{};
  GridCall c(a.vol, stream);
  hipStream_t s = c.s;
  int rc = c.open(rif, nvox, res, h, ds); if (rc) return rc;
  if (n == 0) return zero_stats(stats, s);
  if (!pos || !vel || !xt || !vt) return fail(DRRT_ERR_ARG, "null ray pointer");
  if (MODE == 1 && (!pln_o || !pln_d || !failmask)) return fail(DRRT_ERR_ARG, "null plane/failmask pointer");
  if ((MODE == 1 || MODE == 2) && !stats) { rc = private_stats(&stats); if (rc) return rc; }
  if (MODE == 2 && !sdf) return fail(DRRT_ERR_ARG, "null sdf pointer");
  rc = check_ray_count(n); if (rc) return rc;
  rc = zero_stats(stats, s); if (rc) return rc;
  const WsLayout L = ws_layout(n, nvox, flags, ws_bytes);
  rc = c.place(nvox, n, pos, vel, 1.f, flags, L, ws, ws_bytes, io_half); if (rc) return rc;
  if (MODE == 2) {                      // the second-pass flags: n bytes of the per-ray slot
    if (!ws || ws_bytes < L.slot_off + n) return fail(DRRT_ERR_ARG, "workspace too small for trace_sdf (see drrt_workspace_bytes)");
    a.again = (uint8_t*)ws + L.slot_off;
  }
  g_ts.reset_last_steps();
  if (MODE != 2 && ws && ws_bytes >= L.slot_off + n * sizeof(uint32_t)) {
    // per-ray iteration counts for the paired adjoint (drrt_last_steps): n uint32 of the per-ray slot, where there is room
    a.steps_out = (uint32_t*)((char*)ws + L.slot_off);
    g_ts.last_steps = a.steps_out; g_ts.last_steps_n = n;
  }
  a.io_half = io_half;
  a.sdf = sdf; a.pos = pos; a.vel = vel; a.pln_o = pln_o; a.pln_d = pln_d;
  a.xt = xt; a.vt = vt; a.failmask = failmask; a.stats = stats; a.n = n; a.ds = ds;
  a.max_steps = (MODE == 2) ? steps_sdf(h, res, ds) : steps_fwd(h, res, ds);
  a.perm = c.perm; a.xcd_order = c.xcd_order;
  {
    ProfScope prof(DRRT_PROF_TRACE, s);
    launch_trace(MODE, a, s);
  }
  LAUNCH_CHECK("k_trace");
  if (MODE == 1 || MODE == 2) {
    launch_trace_again(MODE, a, s);
    LAUNCH_CHECK("k_trace_again");
  }
  return DRRT_OK;
}

extern "C" int drrt_trace_f32(const float* rif, long long nvox, const int res[3], size_t n,
                              const float* pos, const float* vel, float h, float ds, float* xt, float* vt,
                              drrt_stats* stats, void* ws, size_t ws_bytes, unsigned flags, void* stream) {
  return run_trace<0>(rif, nullptr, nvox, res, n, pos, vel, nullptr, nullptr, h, ds, xt, vt, nullptr,
                      stats, ws, ws_bytes, flags, stream);
}

extern "C" int drrt_trace_f16io(const float* rif, long long nvox, const int res[3], size_t n,
                                const void* pos, const void* vel, float h, float ds, void* xt, void* vt,
                                drrt_stats* stats, void* ws, size_t ws_bytes, unsigned flags, void* stream) {
  return run_trace<0>(rif, nullptr, nvox, res, n, pos, vel, nullptr, nullptr, h, ds, xt, vt, nullptr,
                      stats, ws, ws_bytes, flags, stream, 1);
}

extern "C" int drrt_trace_q16io(const float* rif, long long nvox, const int res[3], size_t n,
                                const void* pos, const void* vel, float h, float ds, void* xt, void* vt,
                                drrt_stats* stats, void* ws, size_t ws_bytes, unsigned flags, void* stream) {
  return run_trace<0>(rif, nullptr, nvox, res, n, pos, vel, nullptr, nullptr, h, ds, xt, vt, nullptr,
                      stats, ws, ws_bytes, flags, stream, (flags & DRRT_FLAG_Q16_POS_ONLY) ? 3 : 2);
}

// ---- 16-bit ray state: encode / decode on the device (so that every binding rounds exactly as the kernels do) ----
namespace drrt {
__global__ void __launch_bounds__(256) k_q16_encode(Vol V, size_t n3, const float* __restrict__ pos, const float* __restrict__ vel,
                                                    uint16_t* __restrict__ pos_q, int16_t* __restrict__ vel_q) {
  const size_t k = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= n3) return;
  if (pos) pos_q[k] = q16_pos_enc(V, pos[k]);
  if (vel) vel_q[k] = q16_vel_enc(vel[k]);
}
__global__ void __launch_bounds__(256) k_q16_decode(Vol V, size_t n3, const uint16_t* __restrict__ pos_q, const int16_t* __restrict__ vel_q,
                                                    float* __restrict__ pos, float* __restrict__ vel) {
  const size_t k = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= n3) return;
  if (pos_q) pos[k] = q16_pos_dec(V, pos_q[k]);
  if (vel_q) vel[k] = q16_vel_dec(vel_q[k]);
}
}  // namespace drrt

static int q16_vol(const int res[3], float h, Vol* V) {
  if (!res) return fail(DRRT_ERR_ARG, "null res pointer");
  if (res[0] < 1 || res[1] < 1 || res[2] < 1) return fail(DRRT_ERR_BAD_RES, "volume: invalid resolution!");
  if (!(h > 0.f) || !(h < 3.0e38f)) return fail(DRRT_ERR_ARG, "h and ds must be positive and finite");
  V->data = nullptr; V->W = res[0]; V->H = res[1]; V->D = res[2];
  vol_finish(*V, h);
  return DRRT_OK;
}

extern "C" int drrt_q16_params(const int res[3], float h, float out[3]) {
  g_err[0] = 0;
  Vol V; int rc = q16_vol(res, h, &V); if (rc) return rc;
  if (!out) return fail(DRRT_ERR_ARG, "null output pointer");
  out[0] = V.q_min; out[1] = V.q_step; out[2] = kQ16VelStep;
  return DRRT_OK;
}

extern "C" int drrt_q16_encode(const int res[3], float h, size_t n, const float* pos, const float* vel, void* pos_q,
                               void* vel_q, void* stream) {
  g_err[0] = 0;
  Vol V; int rc = q16_vol(res, h, &V); if (rc) return rc;
  if ((pos && !pos_q) || (vel && !vel_q)) return fail(DRRT_ERR_ARG, "null output pointer");
  if (n == 0 || (!pos && !vel)) return DRRT_OK;
  hipLaunchKernelGGL(k_q16_encode, dim3((unsigned)((3 * n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, V, 3 * n, pos, vel,
                     (uint16_t*)pos_q, (int16_t*)vel_q);
  LAUNCH_CHECK("k_q16_encode");
  return DRRT_OK;
}

extern "C" int drrt_q16_decode(const int res[3], float h, size_t n, const void* pos_q, const void* vel_q, float* pos,
                               float* vel, void* stream) {
  g_err[0] = 0;
  Vol V; int rc = q16_vol(res, h, &V); if (rc) return rc;
  if ((pos_q && !pos) || (vel_q && !vel)) return fail(DRRT_ERR_ARG, "null output pointer");
  if (n == 0 || (!pos_q && !vel_q)) return DRRT_OK;
  hipLaunchKernelGGL(k_q16_decode, dim3((unsigned)((3 * n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, V, 3 * n,
                     (const uint16_t*)pos_q, (const int16_t*)vel_q, pos, vel);
  LAUNCH_CHECK("k_q16_decode");
  return DRRT_OK;
}

extern "C" int drrt_trace_pln_f32(const float* rif, long long nvox, const int res[3], size_t n,
                                  const float* pos, const float* vel, const float* pln_o, const float* pln_d,
                                  float h, float ds, float* xt, float* vt, uint8_t* failmask,
                                  drrt_stats* stats, void* ws, size_t ws_bytes, unsigned flags, void* stream) {
  return run_trace<1>(rif, nullptr, nvox, res, n, pos, vel, pln_o, pln_d, h, ds, xt, vt, failmask,
                      stats, ws, ws_bytes, flags, stream);
}

extern "C" int drrt_trace_sdf_f32(const float* rif, const float* sdf, long long nvox, const int res[3],
                                  size_t n, const float* pos, const float* vel, float h, float ds,
                                  float* xt, float* vt, drrt_stats* stats, void* ws, size_t ws_bytes,
                                  unsigned flags, void* stream) {
  return run_trace<2>(rif, sdf, nvox, res, n, pos, vel, nullptr, nullptr, h, ds, xt, vt, nullptr,
                      stats, ws, ws_bytes, flags, stream);
}

extern "C" int drrt_trace_target_f32(const float* rif, long long nvox, const int res[3], size_t n,
                                     const float* pos, const float* vel, const float* target,
                                     float h, float ds, float* xt, float* vt, float* dist2,
                                     drrt_stats* stats, void* ws, size_t ws_bytes, unsigned flags,
                                     void* stream) {
  TargetArgs a{};
  GridCall c(a.vol, stream);
  c.hint = OrderHint{};              // never honoured here: the phase-A state at the start of the workspace would overlay an
                                     // order that lives in the same workspace (drrt_last_order() of an earlier call)
  g_ts.reset_last_steps();           // this forward march writes no iteration counts
  hipStream_t s = c.s;
  int rc = c.open(rif, nvox, res, h, ds); if (rc) return rc;
  if (n == 0) return zero_stats(stats, s);
  if (!pos || !vel || !target || !xt || !vt || !dist2) return fail(DRRT_ERR_ARG, "null ray pointer");
  rc = check_ray_count(n); if (rc) return rc;
  // the global iteration count lives in stats->iters: a stats block is mandatory here
  if (!stats) return fail(DRRT_ERR_ARG, "trace_target needs a stats block (global loop count)");
  const WsLayout L = ws_layout(n, nvox, flags, ws_bytes, /*target_order=*/true);
  if (!ws || ws_bytes < L.ray_bytes) return fail(DRRT_ERR_ARG, "workspace too small for trace_target");
  rc = zero_stats(stats, s); if (rc) return rc;
  rc = c.place(nvox, n, pos, vel, 1.f, flags, L, ws, ws_bytes); if (rc) return rc;
  a.state = (float*)((char*)ws + L.slot_off);
  a.perm = c.perm;
  a.pos = pos; a.vel = vel; a.target = target; a.xt = xt; a.vt = vt; a.dist2 = dist2;
  a.stats = stats; a.n = n; a.ds = ds; a.max_steps = steps_fwd(h, res, ds);
  launch_target(a, s);
  LAUNCH_CHECK("k_target");
  return DRRT_OK;
}

// One chunk of a resumable adjoint march (drrt_backtrace_chunk_f32)
struct ChunkReq { void* state; size_t state_bytes; int it_begin, it_count; int* progress; };

namespace drrt {
__global__ void k_chunk_progress_init(int* p) {
  const int k = threadIdx.x;              // [0..11] mins, maxs, mins, maxs; [12] count; [13..18] mins, maxs; [19] spare
  if (k < 20) p[k] = (k == 12 || k == 19) ? 0 : ((((k < 12 ? k : k - 1) / 3) & 1) ? (int)0x80000000 : 0x7fffffff);
}
}  // namespace drrt

// Which adjoint kernels a call launches; run_backtrace launches them in the order classify, ring, box.
struct BackPlan {
  bool direct = false;        // the one-atomic-per-tap kernel, nothing else
  bool classify = false;      // k_bundle_classify first: the windowed kernels launched after it return unless its counters pick them
  bool ring_general = false;  // k_backtrace_ring, general instantiation (a classified call pins the classification to it)
  int ring_sparse = -1;       // the sparse-only instantiations (launch_backtrace_ring_sparse's `which`), -1: none
  bool box = false;           // k_backtrace_flat
};
static BackPlan plan_backtrace(int mode, unsigned flags, bool chunk, bool dbg, bool classifiable) {
  BackPlan p;
  // DRRT_FLAG_DIRECT_ATOMICS: the kernel every windowed one is cross-checked against
  if (flags & DRRT_FLAG_DIRECT_ATOMICS) { p.direct = true; return p; }
  // DRRT_FLAG_RING_WINDOW forces the ring kernel (A-B; not for chunks): sparse-only with DRRT_FLAG_RING_SPARSE (direct with
  // DRRT_FLAG_RING_DIRECT) where that exists -- backtrace without counters --, general otherwise
  if ((flags & DRRT_FLAG_RING_WINDOW) && !chunk) {
    if ((flags & DRRT_FLAG_RING_SPARSE) && mode == 0 && !dbg) p.ring_sparse = (flags & DRRT_FLAG_RING_DIRECT) ? 1 : 0;
    else p.ring_general = true;
    return p;
  }
  // the box-window kernel (compile-time 9^3 window, for compact bundles) only: DRRT_FLAG_STATIC_WINDOW (A-B), chunks, and
  // calls without a visit order or without the 512-byte counter block at the end of a drrt_workspace_bytes_grid() workspace
  p.box = true;
  if ((flags & DRRT_FLAG_STATIC_WINDOW) || chunk || !classifiable) return p;
  // otherwise the bundles are classified on the device and BOTH windowed kernels are launched (no host round trip); the
  // ring kernel (fitted ring window, step hint) in its sparse-only instantiations unless the call is backtrace_sdf, the
  // debug-counter build or DRRT_FLAG_RING_GENERAL (A-B), which only the general one serves
  p.classify = true;
  if (mode == 0 && !dbg && !(flags & DRRT_FLAG_RING_GENERAL)) p.ring_sparse = 2;
  else p.ring_general = true;
  return p;
}

template <int MODE>
static int run_backtrace(const float* rif, const float* sdf, long long nvox, const int res[3], size_t n,
                         const void* xt, const void* vt, const void* dx, const void* dv,
                         float h, float ds, float* grad, drrt_stats* stats, void* ws, size_t ws_bytes,
                         unsigned flags, void* stream, int io_half = 0, const ChunkReq* ck = nullptr) {
  BackArgs a{};
  GridCall c(a.vol, stream);
  g_ts.reset_last_counters();             // set again below when this call classifies its bundles
  hipStream_t s = c.s;
  int rc = c.open(rif, nvox, res, h, ds); if (rc) return rc;
  if (!grad) return fail(DRRT_ERR_ARG, "null grad pointer");
  if (MODE == 1 && !sdf) return fail(DRRT_ERR_ARG, "null sdf pointer");
  const unsigned ablation = (flags >> 8) & 0xffu;
  if (ablation > 1u) return fail(DRRT_ERR_ARG, "flags: bits 8..15 must be 0, or 1 (no adjoint launch)");
  const bool first_chunk = ck == nullptr || ck->it_begin == 0;
  if (ck != nullptr) {
    if (ck->it_begin < 0) return fail(DRRT_ERR_ARG, "chunk: it_begin must be >= 0");
    if (flags & DRRT_FLAG_DIRECT_ATOMICS) return fail(DRRT_ERR_ARG, "chunk: not available with DRRT_FLAG_DIRECT_ATOMICS");
    if (!ck->state || ck->state_bytes < drrt_backtrace_chunk_state_bytes(n))
      return fail(DRRT_ERR_ARG, "chunk: state buffer too small (see drrt_backtrace_chunk_state_bytes)");
    if (!first_chunk && (flags & DRRT_FLAG_SORT_RAYS) && !(c.hint.order && c.hint.n == n))
      return fail(DRRT_ERR_ARG, "chunk: a resumed chunk needs the visit order of its first chunk (drrt_set_order_hint)");
  }
  if (!(flags & DRRT_FLAG_NO_ZERO) && first_chunk) {                         // src/tracer.cpp:401-403
    ProfScope prof(DRRT_PROF_ZERO, s);
    hipError_t e = hipMemsetAsync(grad, 0, (size_t)nvox * sizeof(float), s);
    if (e != hipSuccess) return fail_hip(e, "hipMemsetAsync(grad)");
  }
  if (first_chunk) { rc = zero_stats(stats, s); if (rc) return rc; }
  if (n == 0) return DRRT_OK;
  if (!xt || !vt || !dx || !dv) return fail(DRRT_ERR_ARG, "null ray pointer");
  rc = check_ray_count(n); if (rc) return rc;
  if (ablation == 1u) return DRRT_OK;       // the gradient stays zero: bench.py's parity check must fail on it
  const WsLayout L = ws_layout(n, nvox, flags, ws_bytes);
  rc = c.place(nvox, n, xt, vt, -1.f, flags, L, ws, ws_bytes, io_half); if (rc) return rc;
  a.perm = c.perm; a.xcd_order = c.xcd_order;
  a.io_half = io_half;
  a.sdf = sdf; a.xt = xt; a.vt = vt; a.dx = dx; a.dv = dv; a.grad = grad; a.stats = stats;
  a.n = n; a.ds = ds; a.max_steps = steps_adj(h, res, ds);
  if (ck != nullptr) {                      // the iterations [it_begin, it_begin + it_count) of the march's max_steps
    const int left = a.max_steps - ck->it_begin;
    a.max_steps = ck->it_count < 0 ? left : (ck->it_count < left ? ck->it_count : left);
    if (a.max_steps < 0) a.max_steps = 0;
    a.chunk_state = (float*)ck->state; a.chunk_stride = (size_t)adj_grid_for(n) * kAdjBlock;
    a.chunk_resume = first_chunk ? 0 : 1; a.chunk_progress = ck->progress;
    if (ck->progress) { hipLaunchKernelGGL(drrt::k_chunk_progress_init, dim3(1), dim3(64), 0, s, ck->progress); LAUNCH_CHECK("k_chunk_progress_init"); }
  }
  a.grad_scale = (flags & DRRT_FLAG_CORRECTED_H) ? a.vol.inv_h : 1.0f;
  a.fsteps = (c.hint.steps && c.hint.steps_n == n) ? c.hint.steps : nullptr;
  a.dbg = nullptr;
  if (flags & DRRT_FLAG_DEBUG_COUNTERS) {        // the 512 bytes at the end of the caller's buffer
    if (!ws || ws_bytes < kCtrBytes) return fail(DRRT_ERR_ARG, "workspace too small for DRRT_FLAG_DEBUG_COUNTERS");
    a.dbg = (unsigned long long*)((char*)ws + L.dbg_off);
    hipError_t e = hipMemsetAsync(a.dbg, 0, kCtrBytes, s);
    if (e != hipSuccess) return fail_hip(e, "hipMemsetAsync(dbg)");
  }
  const bool dbg = a.dbg != nullptr;
  const BackPlan p = plan_backtrace(MODE, flags, ck != nullptr, dbg, a.perm != nullptr && ws && ws_bytes >= L.grid_bytes);
  {
    ProfScope prof(DRRT_PROF_BACKTRACE, s);
    if (p.direct) launch_backtrace_direct(MODE, a, s);
    if (p.classify) {
      a.select = (unsigned*)((char*)ws + L.select_off);
      g_ts.last_counters = a.select;
      hipError_t e = hipMemsetAsync(a.select, 0, 32, s);
      if (e != hipSuccess) return fail_hip(e, "hipMemsetAsync(select)");
      if (p.ring_general) {        // [5] != 0: the classification picks the general ring instantiation, never a sparse-only one
        e = hipMemsetAsync((char*)a.select + 20, 1, 1, s);
        if (e != hipSuccess) return fail_hip(e, "hipMemsetAsync(select)");
      }
      launch_bundle_classify(a, s);
    }
    if (p.ring_general) launch_backtrace_ring(MODE, dbg, a, s);
    if (p.ring_sparse >= 0) launch_backtrace_ring_sparse(a, s, p.ring_sparse);
    if (p.box) launch_backtrace_box(MODE, dbg, a, s);
  }
  LAUNCH_CHECK("k_backtrace");
  return DRRT_OK;
}

extern "C" int drrt_backtrace_f32(const float* rif, long long nvox, const int res[3], size_t n,
                                  const float* xt, const float* vt, const float* dx, const float* dv,
                                  float h, float ds, float* grad, drrt_stats* stats, void* ws,
                                  size_t ws_bytes, unsigned flags, void* stream) {
  return run_backtrace<0>(rif, nullptr, nvox, res, n, xt, vt, dx, dv, h, ds, grad, stats, ws, ws_bytes, flags, stream);
}

extern "C" int drrt_backtrace_rays_f32(const float* rif, long long nvox, const int res[3], size_t n,
                                       const float* pos, const float* vel, const float* xt, const float* vt,
                                       const uint32_t* fwd_steps, const float* dx, const float* dv, float h, float ds,
                                       float* dpos, float* dvel, drrt_stats* stats, void* ws, size_t ws_bytes,
                                       unsigned flags, void* stream) {
  RayGradArgs a{};
  GridCall c(a.vol, stream);
  hipStream_t s = c.s;
  int rc = c.open(rif, nvox, res, h, ds); if (rc) return rc;
  rc = zero_stats(stats, s); if (rc) return rc;
  if (n == 0) return DRRT_OK;
  if (!pos || !vel || !xt || !vt || !dx || !dv) return fail(DRRT_ERR_ARG, "null ray pointer");
  if (!fwd_steps) return fail(DRRT_ERR_ARG, "null fwd_steps pointer (the forward's drrt_last_steps())");
  if (!dpos || !dvel) return fail(DRRT_ERR_ARG, "null dpos/dvel pointer");
  rc = check_ray_count(n); if (rc) return rc;
  rc = c.place(nvox, n, xt, vt, -1.f, flags, ws_layout(n, nvox, flags, ws_bytes), ws, ws_bytes); if (rc) return rc;
  a.pos = pos; a.vel = vel; a.xt = xt; a.vt = vt; a.fsteps = fwd_steps; a.dx = dx; a.dv = dv;
  a.dpos = dpos; a.dvel = dvel; a.stats = stats; a.n = n; a.ds = ds;
  a.max_steps = steps_fwd(h, res, ds);      // the forward's bound: a ray that used all of it failed
  a.perm = c.perm; a.xcd_order = c.xcd_order;
  return timed_launch(DRRT_PROF_BACKTRACE_RAYS, s, "k_backtrace_rays", [&] { launch_backtrace_rays(a, s); });
}

// ray-state adjoints of trace_plane (MODE 1) and trace_sdf (MODE 2): drrt_ray_adjoints.hip
template <int MODE>
static int run_backtrace_stop_rays(const float* rif, const float* sdf, long long nvox, const int res[3], size_t n,
                                   const float* pos, const float* vel, const float* pln_o, const float* pln_d,
                                   const float* dx, const float* dv, float h, float ds, float* dpos, float* dvel,
                                   drrt_stats* stats, void* ws, size_t ws_bytes, unsigned flags, void* stream) {
  StopRayGradArgs a{};
  GridCall c(a.vol, stream);
  hipStream_t s = c.s;
  int rc = c.open(rif, nvox, res, h, ds); if (rc) return rc;
  if (MODE == 2 && !sdf) return fail(DRRT_ERR_ARG, "null sdf pointer");
  if (n == 0) return zero_stats(stats, s);
  if (!pos || !vel || !dx || !dv) return fail(DRRT_ERR_ARG, "null ray pointer");
  if (MODE == 1 && (!pln_o || !pln_d)) return fail(DRRT_ERR_ARG, "null plane pointer");
  if (!dpos || !dvel) return fail(DRRT_ERR_ARG, "null dpos/dvel pointer");
  rc = check_ray_count(n); if (rc) return rc;
  const WsLayout L = ws_layout(n, nvox, flags, ws_bytes);
  if (!ws || ws_bytes < L.slot_off + n) return fail(DRRT_ERR_ARG, "workspace too small for the second-pass flags (see drrt_workspace_bytes)");
  if (!stats) { rc = private_stats(&stats); if (rc) return rc; }
  rc = zero_stats(stats, s); if (rc) return rc;
  rc = c.place(nvox, n, pos, vel, 1.f, flags, L, ws, ws_bytes); if (rc) return rc;
  a.again = (uint8_t*)ws + L.slot_off;      // the second-pass flags: n bytes of the per-ray slot, as trace_sdf's
  if (c.perm != nullptr) {
    // An order that lives where the flags go is not used: slower, never wrong.  Only a hinted order can (one this call
    // sorted lies in its own sort buffers, beside the slot), and a hint is an address, not a region of L -- it may come
    // from a call that laid this workspace out for other flags -- so the test stays on addresses.
    const char* o = (const char*)c.perm;
    const char* f = (const char*)a.again;
    if (o < f + n && f < o + n * sizeof(uint32_t)) c.drop_order();
  }
  a.sdf = sdf; a.pos = pos; a.vel = vel; a.pln_o = pln_o; a.pln_d = pln_d; a.dx = dx; a.dv = dv;
  a.dpos = dpos; a.dvel = dvel; a.stats = stats; a.n = n; a.ds = ds;
  a.max_steps = (MODE == 2) ? steps_sdf(h, res, ds) : steps_fwd(h, res, ds);      // the forward's bound
  a.perm = c.perm; a.xcd_order = c.xcd_order;
  return timed_launch(MODE == 1 ? DRRT_PROF_BACKTRACE_PLN_RAYS : DRRT_PROF_BACKTRACE_SDF_RAYS, s, "k_backtrace_stop_rays",
                      [&] { launch_backtrace_stop_rays(MODE, a, s); });
}

extern "C" int drrt_backtrace_pln_rays_f32(const float* rif, long long nvox, const int res[3], size_t n,
                                           const float* pos, const float* vel, const float* pln_o, const float* pln_d,
                                           const float* dx, const float* dv, float h, float ds, float* dpos, float* dvel,
                                           drrt_stats* stats, void* ws, size_t ws_bytes, unsigned flags, void* stream) {
  return run_backtrace_stop_rays<1>(rif, nullptr, nvox, res, n, pos, vel, pln_o, pln_d, dx, dv, h, ds, dpos, dvel, stats,
                                    ws, ws_bytes, flags, stream);
}

extern "C" int drrt_backtrace_sdf_rays_f32(const float* rif, const float* sdf, long long nvox, const int res[3], size_t n,
                                           const float* pos, const float* vel, const float* dx, const float* dv, float h,
                                           float ds, float* dpos, float* dvel, drrt_stats* stats, void* ws,
                                           size_t ws_bytes, unsigned flags, void* stream) {
  return run_backtrace_stop_rays<2>(rif, sdf, nvox, res, n, pos, vel, nullptr, nullptr, dx, dv, h, ds, dpos, dvel, stats,
                                    ws, ws_bytes, flags, stream);
}

// ray-state adjoint of trace_target: drrt_ray_adjoints.hip.  Keeps nothing per ray between its two launches, so the per-ray
// slot of the workspace stays untouched and an order hint is used wherever it lives.
extern "C" int drrt_backtrace_target_rays_f32(const float* rif, long long nvox, const int res[3], size_t n,
                                              const float* pos, const float* vel, const float* target,
                                              const float* dx, const float* dv, const float* ddist2, float h, float ds,
                                              float* dpos, float* dvel, drrt_stats* stats, void* ws, size_t ws_bytes,
                                              unsigned flags, void* stream) {
  TargetRayGradArgs a{};
  GridCall c(a.vol, stream);
  hipStream_t s = c.s;
  int rc = c.open(rif, nvox, res, h, ds); if (rc) return rc;
  if (n == 0) return zero_stats(stats, s);
  if (!pos || !vel || !target || !dx || !dv) return fail(DRRT_ERR_ARG, "null ray pointer");
  if (!dpos || !dvel) return fail(DRRT_ERR_ARG, "null dpos/dvel pointer");
  rc = check_ray_count(n); if (rc) return rc;
  const WsLayout L = ws_layout(n, nvox, flags, ws_bytes);
  if (!ws || ws_bytes < L.ray_bytes) return fail(DRRT_ERR_ARG, "workspace too small for backtrace_target_rays (see drrt_workspace_bytes)");
  if (!stats) { rc = private_stats(&stats); if (rc) return rc; }
  rc = zero_stats(stats, s); if (rc) return rc;
  rc = c.place(nvox, n, pos, vel, 1.f, flags, L, ws, ws_bytes); if (rc) return rc;
  a.pos = pos; a.vel = vel; a.target = target; a.dx = dx; a.dv = dv; a.dd2 = ddist2;
  a.dpos = dpos; a.dvel = dvel; a.stats = stats; a.n = n; a.ds = ds;
  a.max_steps = steps_fwd(h, res, ds);      // the forward's bound
  a.perm = c.perm; a.xcd_order = c.xcd_order;
  return timed_launch(DRRT_PROF_BACKTRACE_TARGET_RAYS, s, "k_backtrace_target_rays", [&] { launch_backtrace_target_rays(a, s); });
}

// ---- the integral operators (optical path length, line integral of a second field, emission with self-absorption, line
// integral of a vector field): drrt_integral.hip ------------------------------------------------------------------------
// The eight entry points share one forward and one backward prologue.  An entry point fills the fields of its argument block
// that are its own (further grids, per-ray inputs and outputs, gradient grids) and names them for the checks.
struct IntegralCall {              // the arguments every one of the eight has
  const float* rif; long long nvox; const int* res; size_t n;
  const float* pos; const float* vel;
  float h, ds;
  drrt_stats* stats; void* ws; size_t ws_bytes; unsigned flags; void* stream;
};
struct Needed { const void* p; const char* error; };      // a pointer that must not be null, and the message when it is

// `grids`: the further input grids; `outs`: the operator's per-ray outputs (checked with the rays)
template <typename Args>
static int run_trace_integral(Args& a, const IntegralCall& k, std::initializer_list<Needed> grids,
                              std::initializer_list<const float*> outs, float* xt, float* vt, uint32_t* steps_out,
                              int prof_id, const char* where, void (*launch)(const Args&, hipStream_t)) {
  GridCall c(a.vol, k.stream);
  g_ts.reset_last_steps();              // this forward march writes its iteration counts to the caller, none to the workspace
  hipStream_t s = c.s;
  int rc = c.open(k.rif, k.nvox, k.res, k.h, k.ds); if (rc) return rc;
  for (const Needed& g : grids) if (!g.p) return fail(DRRT_ERR_ARG, g.error);
  if (k.n == 0) return zero_stats(k.stats, s);
  bool rays = k.pos && k.vel && xt && vt;
  for (const float* o : outs) rays = rays && o;
  if (!rays) return fail(DRRT_ERR_ARG, "null ray pointer");
  if (!steps_out) return fail(DRRT_ERR_ARG, "null steps_out pointer (the adjoint needs the iteration counts)");
  rc = check_ray_count(k.n); if (rc) return rc;
  rc = zero_stats(k.stats, s); if (rc) return rc;
  rc = c.place(k.nvox, k.n, k.pos, k.vel, 1.f, k.flags, ws_layout(k.n, k.nvox, k.flags, k.ws_bytes), k.ws, k.ws_bytes);
  if (rc) return rc;
  a.pos = k.pos; a.vel = k.vel; a.xt = xt; a.vt = vt; a.steps_out = steps_out; a.stats = k.stats; a.n = k.n; a.ds = k.ds;
  a.max_steps = steps_fwd(k.h, k.res, k.ds);
  a.perm = c.perm; a.xcd_order = c.xcd_order;
  return timed_launch(prof_id, s, where, [&] { launch(a, s); });
}

// `grids`: the further input grids; `per_ray`: the operator's per-ray inputs that must be there (checked behind fwd_steps);
// `grads`: the gradient grids (each nullable, zeroed here unless DRRT_FLAG_NO_ZERO); `no_outputs`: the message when they,
// dpos and dvel are all null
template <typename Args>
static int run_backtrace_integral(Args& a, const IntegralCall& k, std::initializer_list<Needed> grids,
                                  std::initializer_list<Needed> per_ray, std::initializer_list<float*> grads,
                                  const char* no_outputs, const float* xt, const float* vt, const uint32_t* fwd_steps,
                                  const float* dx, const float* dv, float* dpos, float* dvel, int prof_id, const char* where,
                                  void (*launch)(const Args&, hipStream_t)) {
  GridCall c(a.vol, k.stream);
  hipStream_t s = c.s;
  int rc = c.open(k.rif, k.nvox, k.res, k.h, k.ds); if (rc) return rc;
  for (const Needed& g : grids) if (!g.p) return fail(DRRT_ERR_ARG, g.error);
  bool any = dpos || dvel;
  for (float* g : grads) any = any || g;
  if (!any) return fail(DRRT_ERR_ARG, no_outputs);
  if (!dpos != !dvel) return fail(DRRT_ERR_ARG, "dpos and dvel go together");
  if (k.n > 0) {
    if (!k.pos || !k.vel || !xt || !vt) return fail(DRRT_ERR_ARG, "null ray pointer");
    if (!fwd_steps) return fail(DRRT_ERR_ARG, "null fwd_steps pointer (the forward's steps_out)");
    for (const Needed& p : per_ray) if (!p.p) return fail(DRRT_ERR_ARG, p.error);
    rc = check_ray_count(k.n); if (rc) return rc;
  }
  if (!(k.flags & DRRT_FLAG_NO_ZERO)) {
    for (float* g : grads) {
      if (!g) continue;
      ProfScope prof(DRRT_PROF_ZERO, s);
      hipError_t e = hipMemsetAsync(g, 0, (size_t)k.nvox * sizeof(float), s);
      if (e != hipSuccess) return fail_hip(e, "hipMemsetAsync(grad)");
    }
  }
  rc = zero_stats(k.stats, s); if (rc) return rc;
  if (k.n == 0) return DRRT_OK;
  rc = c.place(k.nvox, k.n, xt, vt, -1.f, k.flags, ws_layout(k.n, k.nvox, k.flags, k.ws_bytes), k.ws, k.ws_bytes);
  if (rc) return rc;
  a.pos = k.pos; a.vel = k.vel; a.xt = xt; a.vt = vt; a.fsteps = fwd_steps; a.dx = dx; a.dv = dv;
  a.dpos = dpos; a.dvel = dvel; a.stats = k.stats; a.n = k.n; a.ds = k.ds;
  a.grad_scale = (k.flags & DRRT_FLAG_CORRECTED_H) ? a.vol.inv_h : 1.0f;
  a.max_steps = steps_fwd(k.h, k.res, k.ds);      // the forward's bound: a ray that used all of it failed
  a.perm = c.perm; a.xcd_order = c.xcd_order;
  return timed_launch(prof_id, s, where, [&] { launch(a, s); });
}

extern "C" int drrt_trace_opl_f32(const float* rif, long long nvox, const int res[3], size_t n,
                                  const float* pos, const float* vel, float h, float ds, float* xt, float* vt,
                                  float* opl, uint32_t* steps_out, drrt_stats* stats, void* ws, size_t ws_bytes,
                                  unsigned flags, void* stream) {
  OplTraceArgs a{};
  a.opl = opl;
  return run_trace_integral(a, {rif, nvox, res, n, pos, vel, h, ds, stats, ws, ws_bytes, flags, stream}, {}, {opl}, xt, vt,
                            steps_out, DRRT_PROF_TRACE_OPL, "k_trace_opl", launch_trace_opl);
}

extern "C" int drrt_backtrace_opl_f32(const float* rif, long long nvox, const int res[3], size_t n,
                                      const float* pos, const float* vel, const float* xt, const float* vt,
                                      const uint32_t* fwd_steps, const float* dx, const float* dv, const float* dopl,
                                      float h, float ds, float* grad, float* dpos, float* dvel, drrt_stats* stats,
                                      void* ws, size_t ws_bytes, unsigned flags, void* stream) {
  OplBackArgs a{};
  a.dopl = dopl; a.grad = grad;
  return run_backtrace_integral(a, {rif, nvox, res, n, pos, vel, h, ds, stats, ws, ws_bytes, flags, stream}, {}, {}, {grad},
                                "null output pointers: grad, or dpos and dvel, or all three", xt, vt, fwd_steps, dx, dv,
                                dpos, dvel, DRRT_PROF_BACKTRACE_OPL, "k_backtrace_opl", launch_backtrace_opl);
}

extern "C" int drrt_trace_field_f32(const float* rif, const float* field, long long nvox, const int res[3], size_t n,
                                    const float* pos, const float* vel, float h, float ds, float* xt, float* vt,
                                    float* tau, uint32_t* steps_out, drrt_stats* stats, void* ws, size_t ws_bytes,
                                    unsigned flags, void* stream) {
  FieldTraceArgs a{};
  a.field = field; a.tau = tau;
  return run_trace_integral(a, {rif, nvox, res, n, pos, vel, h, ds, stats, ws, ws_bytes, flags, stream},
                            {{field, "null field pointer"}}, {tau}, xt, vt, steps_out, DRRT_PROF_TRACE_FIELD, "k_trace_field",
                            launch_trace_field);
}

extern "C" int drrt_backtrace_field_f32(const float* rif, const float* field, long long nvox, const int res[3], size_t n,
                                        const float* pos, const float* vel, const float* xt, const float* vt,
                                        const uint32_t* fwd_steps, const float* dx, const float* dv, const float* dtau,
                                        float h, float ds, float* grad, float* grad_field, float* dpos, float* dvel,
                                        drrt_stats* stats, void* ws, size_t ws_bytes, unsigned flags, void* stream) {
  FieldBackArgs a{};
  a.field = field; a.dtau = dtau; a.grad = grad; a.grad_field = grad_field;
  return run_backtrace_integral(a, {rif, nvox, res, n, pos, vel, h, ds, stats, ws, ws_bytes, flags, stream},
                                {{field, "null field pointer"}}, {}, {grad, grad_field},
                                "null output pointers: grad, grad_field, or dpos and dvel, or any of these together", xt, vt,
                                fwd_steps, dx, dv, dpos, dvel, DRRT_PROF_BACKTRACE_FIELD, "k_backtrace_field",
                                launch_backtrace_field);
}

extern "C" int drrt_trace_emission_f32(const float* rif, const float* emission, const float* absorption, long long nvox,
                                       const int res[3], size_t n, const float* pos, const float* vel, float h, float ds,
                                       float* xt, float* vt, float* rad, float* tau, uint32_t* steps_out, drrt_stats* stats,
                                       void* ws, size_t ws_bytes, unsigned flags, void* stream) {
  EmissionTraceArgs a{};
  a.emission = emission; a.absorption = absorption; a.rad = rad; a.tau = tau;
  return run_trace_integral(a, {rif, nvox, res, n, pos, vel, h, ds, stats, ws, ws_bytes, flags, stream},
                            {{emission, "null emission pointer"}, {absorption, "null absorption pointer"}}, {rad, tau}, xt,
                            vt, steps_out, DRRT_PROF_TRACE_EMISSION, "k_trace_emission", launch_trace_emission);
}

extern "C" int drrt_backtrace_emission_f32(const float* rif, const float* emission, const float* absorption, long long nvox,
                                           const int res[3], size_t n, const float* pos, const float* vel, const float* xt,
                                           const float* vt, const uint32_t* fwd_steps, const float* tau, const float* dx,
                                           const float* dv, const float* drad, const float* dtau, float h, float ds,
                                           float* grad, float* grad_emission, float* grad_absorption, float* dpos,
                                           float* dvel, drrt_stats* stats, void* ws, size_t ws_bytes, unsigned flags,
                                           void* stream) {
  EmissionBackArgs a{};
  a.emission = emission; a.absorption = absorption; a.tau = tau; a.drad = drad; a.dtau = dtau;
  a.grad = grad; a.grad_emission = grad_emission; a.grad_absorption = grad_absorption;
  return run_backtrace_integral(
      a, {rif, nvox, res, n, pos, vel, h, ds, stats, ws, ws_bytes, flags, stream},
      {{emission, "null emission pointer"}, {absorption, "null absorption pointer"}},
      {{tau, "null tau pointer (the forward's tau)"}}, {grad, grad_emission, grad_absorption},
      "null output pointers: grad, grad_emission, grad_absorption, or dpos and dvel, or any of these together", xt, vt,
      fwd_steps, dx, dv, dpos, dvel, DRRT_PROF_BACKTRACE_EMISSION, "k_backtrace_emission", launch_backtrace_emission);
}

extern "C" int drrt_trace_vector_f32(const float* rif, const float* vfield, long long nvox, const int res[3], size_t n,
                                     const float* pos, const float* vel, float h, float ds, float* xt, float* vt,
                                     float* circ, uint32_t* steps_out, drrt_stats* stats, void* ws, size_t ws_bytes,
                                     unsigned flags, void* stream) {
  VectorTraceArgs a{};
  a.vfield = vfield; a.circ = circ;
  return run_trace_integral(a, {rif, nvox, res, n, pos, vel, h, ds, stats, ws, ws_bytes, flags, stream},
                            {{vfield, "null vfield pointer"}}, {circ}, xt, vt, steps_out, DRRT_PROF_TRACE_VECTOR,
                            "k_trace_vector", launch_trace_vector);
}

extern "C" int drrt_backtrace_vector_f32(const float* rif, const float* vfield, long long nvox, const int res[3], size_t n,
                                         const float* pos, const float* vel, const float* xt, const float* vt,
                                         const uint32_t* fwd_steps, const float* dx, const float* dv, const float* dcirc,
                                         float h, float ds, float* grad, float* grad_vfield, float* dpos, float* dvel,
                                         drrt_stats* stats, void* ws, size_t ws_bytes, unsigned flags, void* stream) {
  VectorBackArgs a{};
  a.vfield = vfield; a.dcirc = dcirc; a.grad = grad; a.grad_vfield = grad_vfield;
  // the three planes of grad_vfield are three gradient grids of nvox floats to the prologue, which zeroes each
  float* const gy = grad_vfield && nvox > 0 ? grad_vfield + nvox : nullptr;
  float* const gz = grad_vfield && nvox > 0 ? grad_vfield + 2 * nvox : nullptr;
  return run_backtrace_integral(a, {rif, nvox, res, n, pos, vel, h, ds, stats, ws, ws_bytes, flags, stream},
                                {{vfield, "null vfield pointer"}}, {}, {grad, grad_vfield, gy, gz},
                                "null output pointers: grad, grad_vfield, or dpos and dvel, or any of these together", xt, vt,
                                fwd_steps, dx, dv, dpos, dvel, DRRT_PROF_BACKTRACE_VECTOR, "k_backtrace_vector",
                                launch_backtrace_vector);
}

// the checks of the two path entries that are their own, in front of the family's prologue
static int check_path_series(int stride, int samples, size_t n) {
  if (stride < 1) return fail(DRRT_ERR_ARG, "stride must be at least 1");
  if (samples < 1) return fail(DRRT_ERR_ARG, "samples must be at least 1");
  // the kernels index path with size_t: (j n + i) 3 floats, j < samples
  if (n > 0 && (size_t)samples > SIZE_MAX / (3 * sizeof(float)) / n)
    return fail(DRRT_ERR_ARG, "samples * n * 3 floats overflow size_t");
  return DRRT_OK;
}

extern "C" int drrt_trace_path_f32(const float* rif, long long nvox, const int res[3], size_t n,
                                   const float* pos, const float* vel, float h, float ds, int stride, int samples,
                                   float* xt, float* vt, float* path, int* count, uint32_t* steps_out, drrt_stats* stats,
                                   void* ws, size_t ws_bytes, unsigned flags, void* stream) {
  int rc = check_path_series(stride, samples, n); if (rc) return rc;
  PathTraceArgs a{};
  a.path = path; a.count = count; a.stride = (unsigned)stride; a.samples = (unsigned)samples;
  // count rides with the ray pointers: one check, one message
  return run_trace_integral(a, {rif, nvox, res, n, pos, vel, h, ds, stats, ws, ws_bytes, flags, stream}, {},
                            {path, (const float*)count}, xt, vt, steps_out, DRRT_PROF_TRACE_PATH, "k_trace_path",
                            launch_trace_path);
}

extern "C" int drrt_backtrace_path_f32(const float* rif, long long nvox, const int res[3], size_t n,
                                       const float* pos, const float* vel, const float* xt, const float* vt,
                                       const uint32_t* fwd_steps, const float* dx, const float* dv, const float* dpath,
                                       float h, float ds, int stride, int samples, float* grad, float* dpos, float* dvel,
                                       drrt_stats* stats, void* ws, size_t ws_bytes, unsigned flags, void* stream) {
  int rc = check_path_series(stride, samples, n); if (rc) return rc;
  PathBackArgs a{};
  a.dpath = dpath; a.grad = grad; a.stride = (unsigned)stride; a.samples = (unsigned)samples;
  return run_backtrace_integral(a, {rif, nvox, res, n, pos, vel, h, ds, stats, ws, ws_bytes, flags, stream}, {}, {}, {grad},
                                "null output pointers: grad, or dpos and dvel, or all three", xt, vt, fwd_steps, dx, dv,
                                dpos, dvel, DRRT_PROF_BACKTRACE_PATH, "k_backtrace_path", launch_backtrace_path);
}

// the two series of the phase entries have one extent (samples, n, 3): check_path_series covers each
extern "C" int drrt_trace_phase_f32(const float* rif, long long nvox, const int res[3], size_t n,
                                    const float* pos, const float* vel, float h, float ds, int stride, int samples,
                                    float* xt, float* vt, float* path, float* vpath, int* count, uint32_t* steps_out,
                                    drrt_stats* stats, void* ws, size_t ws_bytes, unsigned flags, void* stream) {
  int rc = check_path_series(stride, samples, n); if (rc) return rc;
  PhaseTraceArgs a{};
  a.path = path; a.vpath = vpath; a.count = count; a.stride = (unsigned)stride; a.samples = (unsigned)samples;
  return run_trace_integral(a, {rif, nvox, res, n, pos, vel, h, ds, stats, ws, ws_bytes, flags, stream}, {},
                            {path, vpath, (const float*)count}, xt, vt, steps_out, DRRT_PROF_TRACE_PHASE, "k_trace_phase",
                            launch_trace_phase);
}

extern "C" int drrt_backtrace_phase_f32(const float* rif, long long nvox, const int res[3], size_t n,
                                        const float* pos, const float* vel, const float* xt, const float* vt,
                                        const uint32_t* fwd_steps, const float* dx, const float* dv, const float* dpath,
                                        const float* dvpath, float h, float ds, int stride, int samples, float* grad,
                                        float* dpos, float* dvel, drrt_stats* stats, void* ws, size_t ws_bytes,
                                        unsigned flags, void* stream) {
  int rc = check_path_series(stride, samples, n); if (rc) return rc;
  PhaseBackArgs a{};
  a.dpath = dpath; a.dvpath = dvpath; a.grad = grad; a.stride = (unsigned)stride; a.samples = (unsigned)samples;
  return run_backtrace_integral(a, {rif, nvox, res, n, pos, vel, h, ds, stats, ws, ws_bytes, flags, stream}, {}, {}, {grad},
                                "null output pointers: grad, or dpos and dvel, or all three", xt, vt, fwd_steps, dx, dv,
                                dpos, dvel, DRRT_PROF_BACKTRACE_PHASE, "k_backtrace_phase", launch_backtrace_phase);
}

extern "C" size_t drrt_backtrace_chunk_state_bytes(size_t n) { return (size_t)adj_grid_for(n) * kAdjBlock * 13 * sizeof(float); }
extern "C" int drrt_backtrace_max_steps(const int res[3], float h, float ds) {
  if (!res || !(h > 0.f) || !(ds > 0.f)) return -1;
  return steps_adj(h, res, ds);
}
extern "C" int drrt_backtrace_chunk_f32(const float* rif, long long nvox, const int res[3], size_t n,
                                        const float* xt, const float* vt, const float* dx, const float* dv,
                                        float h, float ds, float* grad, drrt_stats* stats, void* ws,
                                        size_t ws_bytes, unsigned flags, void* stream, void* state, size_t state_bytes,
                                        int it_begin, int it_count, int* progress) {
  const ChunkReq ck{state, state_bytes, it_begin, it_count, progress};
  return run_backtrace<0>(rif, nullptr, nvox, res, n, xt, vt, dx, dv, h, ds, grad, stats, ws, ws_bytes, flags, stream, 0, &ck);
}

extern "C" int drrt_backtrace_f16io(const float* rif, long long nvox, const int res[3], size_t n,
                                    const void* xt, const void* vt, const void* dx, const void* dv,
                                    float h, float ds, float* grad, drrt_stats* stats, void* ws,
                                    size_t ws_bytes, unsigned flags, void* stream) {
  return run_backtrace<0>(rif, nullptr, nvox, res, n, xt, vt, dx, dv, h, ds, grad, stats, ws, ws_bytes, flags, stream, 1);
}

extern "C" int drrt_backtrace_q16io(const float* rif, long long nvox, const int res[3], size_t n,
                                    const void* xt, const void* vt, const void* dx, const void* dv,
                                    float h, float ds, float* grad, drrt_stats* stats, void* ws,
                                    size_t ws_bytes, unsigned flags, void* stream) {
  return run_backtrace<0>(rif, nullptr, nvox, res, n, xt, vt, dx, dv, h, ds, grad, stats, ws, ws_bytes, flags, stream,
                          (flags & DRRT_FLAG_Q16_POS_ONLY) ? 3 : 2);
}

extern "C" int drrt_backtrace_sdf_f32(const float* rif, const float* sdf, long long nvox, const int res[3],
                                      size_t n, const float* xt, const float* vt, const float* dx,
                                      const float* dv, float h, float ds, float* grad, drrt_stats* stats,
                                      void* ws, size_t ws_bytes, unsigned flags, void* stream) {
  return run_backtrace<1>(rif, sdf, nvox, res, n, xt, vt, dx, dv, h, ds, grad, stats, ws, ws_bytes, flags, stream);
}

// ---- the prologue the seven cable entries share, in their common order: the hint (taken, never honoured: the cable kernels
// visit rays in caller order), the profile and step checks, the adjoint's zero fill of `zero_grad` (nullable), the stats,
// and the head of the argument block.  `null_msg` (nullable) is the entry's complaint about its own grid pointers.
template <class Args>
static int cable_begin(Args& a, const char* null_msg, const float* rif, size_t rres, float radius, float length, float ds,
                       float* zero_grad, drrt_stats* stats, size_t n, hipStream_t s) {
  (void)g_ts.take_hint();
  g_err[0] = 0;
  if (null_msg) return fail(DRRT_ERR_ARG, null_msg);
  if (rres < 2 || rres > 0x7fffffffULL) return fail(DRRT_ERR_BAD_RES, "volume: invalid resolution!");
  if (!(radius > 0.f) || !(length > 0.f) || !(ds > 0.f) || !(ds < 3.0e38f))
    return fail(DRRT_ERR_ARG, "radius, length and ds must be positive and finite");
  if (zero_grad) {                                                           // src/tracer.cpp:528-530
    hipError_t e = hipMemsetAsync(zero_grad, 0, rres * sizeof(float), s);
    if (e != hipSuccess) return fail_hip(e, "hipMemsetAsync(grad)");
  }
  a.rif = rif; a.rres = (int)rres; a.radius = radius; a.length = length; a.ds = ds;
  a.max_steps = (int)(4.0f * length / ds);                                   // src/tracer.cpp:332, :544
  a.stats = stats; a.n = n;
  return zero_stats(stats, s);
}

extern "C" int drrt_trace_cable_f32(const float* rif, size_t rres, float radius, float length, size_t n,
                                    const float* pos, const float* vel, const float* target, float ds,
                                    float* xt, float* vt, float* dist2, drrt_stats* stats, void* ws,
                                    size_t ws_bytes, unsigned flags, void* stream) {
  (void)ws; (void)ws_bytes; (void)flags;
  hipStream_t s = (hipStream_t)stream;
  CableArgs a{};
  const int rc = cable_begin(a, rif ? nullptr : "null rif pointer", rif, rres, radius, length, ds, nullptr, stats, n, s);
  g_ts.reset_last_steps();              // this forward march writes no iteration counts, refused or not
  if (rc || n == 0) return rc;
  if (!pos || !vel || !target || !xt || !vt || !dist2) return fail(DRRT_ERR_ARG, "null ray pointer");
  a.pos = pos; a.vel = vel; a.target = target; a.xt = xt; a.vt = vt; a.dist2 = dist2;
  return timed_launch(DRRT_PROF_TRACE, s, "k_trace_cable", [&] { launch_trace_cable(a, s); });
}

extern "C" int drrt_backtrace_cable_f32(const float* rif, size_t rres, float radius, float length, size_t n,
                                        const float* xt, const float* vt, const float* dx, const float* dv,
                                        float ds, float* grad, drrt_stats* stats, void* ws, size_t ws_bytes,
                                        unsigned flags, void* stream) {
  (void)ws; (void)ws_bytes;
  hipStream_t s = (hipStream_t)stream;
  CableArgs a{};
  const int rc = cable_begin(a, rif && grad ? nullptr : "null rif/grad pointer", rif, rres, radius, length, ds,
                             (flags & DRRT_FLAG_NO_ZERO) ? nullptr : grad, stats, n, s);
  if (rc || n == 0) return rc;
  if (!xt || !vt || !dx || !dv) return fail(DRRT_ERR_ARG, "null ray pointer");
  a.pos = xt; a.vel = vt; a.dx = dx; a.dv = dv; a.grad = grad;
  return timed_launch(DRRT_PROF_BACKTRACE, s, "k_backtrace_cable", [&] { launch_backtrace_cable(a, s); });
}

extern "C" int drrt_backtrace_cable_rays_f32(const float* rif, size_t rres, float radius, float length, size_t n,
                                             const float* pos, const float* vel, const float* target,
                                             const float* dx, const float* dv, float ds, float* dpos, float* dvel,
                                             drrt_stats* stats, void* ws, size_t ws_bytes, unsigned flags,
                                             void* stream) {
  (void)ws; (void)ws_bytes; (void)flags;
  hipStream_t s = (hipStream_t)stream;
  CableRayGradArgs a{};
  const int rc = cable_begin(a, rif ? nullptr : "null rif pointer", rif, rres, radius, length, ds, nullptr, stats, n, s);
  if (rc || n == 0) return rc;
  if (!pos || !vel || !target || !dx || !dv) return fail(DRRT_ERR_ARG, "null ray pointer");
  if (!dpos || !dvel) return fail(DRRT_ERR_ARG, "null dpos/dvel pointer");
  a.pos = pos; a.vel = vel; a.target = target; a.dx = dx; a.dv = dv; a.dpos = dpos; a.dvel = dvel;
  return timed_launch(DRRT_PROF_BACKTRACE_CABLE_RAYS, s, "k_backtrace_cable_rays", [&] { launch_backtrace_cable_rays(a, s); });
}

extern "C" int drrt_trace_cable_opl_f32(const float* rif, size_t rres, float radius, float length, size_t n,
                                        const float* pos, const float* vel, const float* target, float ds,
                                        float* xt, float* vt, float* dist2, float* opl, uint32_t* rec_steps,
                                        drrt_stats* stats, void* ws, size_t ws_bytes, unsigned flags, void* stream) {
  (void)ws; (void)ws_bytes; (void)flags;
  hipStream_t s = (hipStream_t)stream;
  CableOplTraceArgs a{};
  const int rc = cable_begin(a, rif ? nullptr : "null rif pointer", rif, rres, radius, length, ds, nullptr, stats, n, s);
  g_ts.reset_last_steps();              // rec_steps is the caller's: no iteration counts are left in the workspace
  if (rc || n == 0) return rc;
  if (!pos || !vel || !target || !xt || !vt || !dist2) return fail(DRRT_ERR_ARG, "null ray pointer");
  if (!opl || !rec_steps) return fail(DRRT_ERR_ARG, "null opl/rec_steps pointer");
  a.pos = pos; a.vel = vel; a.target = target; a.xt = xt; a.vt = vt; a.dist2 = dist2; a.opl = opl; a.rec_steps = rec_steps;
  return timed_launch(DRRT_PROF_TRACE_CABLE_OPL, s, "k_trace_cable_opl", [&] { launch_trace_cable_opl(a, s); });
}

extern "C" int drrt_backtrace_cable_opl_f32(const float* rif, size_t rres, float radius, float length, size_t n,
                                            const float* pos, const float* xt, const float* vt, const uint32_t* rec_steps,
                                            const float* dx, const float* dv, const float* dopl, float ds, float* grad,
                                            float* dpos, float* dvel, drrt_stats* stats, void* ws, size_t ws_bytes,
                                            unsigned flags, void* stream) {
  (void)ws; (void)ws_bytes;
  hipStream_t s = (hipStream_t)stream;
  CableOplBackArgs a{};
  const char* refusal = !rif ? "null rif pointer"
                      : !(grad || dpos || dvel) ? "nothing to compute: grad, dpos and dvel are all null"
                      : !dpos != !dvel ? "dpos and dvel go together" : nullptr;
  const int rc = cable_begin(a, refusal, rif, rres, radius, length, ds, (flags & DRRT_FLAG_NO_ZERO) ? nullptr : grad, stats,
                             n, s);
  if (rc || n == 0) return rc;
  if (!pos || !xt || !vt) return fail(DRRT_ERR_ARG, "null ray pointer");
  if (!rec_steps) return fail(DRRT_ERR_ARG, "null rec_steps pointer (the forward's rec_steps)");
  a.pos = pos; a.xt = xt; a.vt = vt; a.rec_steps = rec_steps; a.dx = dx; a.dv = dv; a.dopl = dopl;
  a.grad = grad; a.dpos = dpos; a.dvel = dvel;
  return timed_launch(DRRT_PROF_BACKTRACE_CABLE_OPL, s, "k_backtrace_cable_opl", [&] { launch_backtrace_cable_opl(a, s); });
}

extern "C" int drrt_trace_cable_field_f32(const float* rif, const float* field, size_t rres, float radius, float length,
                                          size_t n, const float* pos, const float* vel, const float* target, float ds,
                                          float* xt, float* vt, float* dist2, float* tau, uint32_t* rec_steps,
                                          drrt_stats* stats, void* ws, size_t ws_bytes, unsigned flags, void* stream) {
  (void)ws; (void)ws_bytes; (void)flags;
  hipStream_t s = (hipStream_t)stream;
  CableFieldTraceArgs a{};
  const int rc = cable_begin(a, !rif ? "null rif pointer" : !field ? "null field pointer" : nullptr, rif, rres, radius, length,
                             ds, nullptr, stats, n, s);
  g_ts.reset_last_steps();              // rec_steps is the caller's: no iteration counts are left in the workspace
  if (rc || n == 0) return rc;
  if (!pos || !vel || !target || !xt || !vt || !dist2) return fail(DRRT_ERR_ARG, "null ray pointer");
  if (!tau || !rec_steps) return fail(DRRT_ERR_ARG, "null tau/rec_steps pointer");
  a.field = field;
  a.pos = pos; a.vel = vel; a.target = target; a.xt = xt; a.vt = vt; a.dist2 = dist2; a.tau = tau; a.rec_steps = rec_steps;
  return timed_launch(DRRT_PROF_TRACE_CABLE_FIELD, s, "k_trace_cable_field", [&] { launch_trace_cable_field(a, s); });
}

extern "C" int drrt_backtrace_cable_field_f32(const float* rif, const float* field, size_t rres, float radius, float length,
                                              size_t n, const float* pos, const float* xt, const float* vt,
                                              const uint32_t* rec_steps, const float* dx, const float* dv, const float* dtau,
                                              float ds, float* grad, float* grad_field, float* dpos, float* dvel,
                                              drrt_stats* stats, void* ws, size_t ws_bytes, unsigned flags, void* stream) {
  (void)ws; (void)ws_bytes;
  hipStream_t s = (hipStream_t)stream;
  CableFieldBackArgs a{};
  const char* refusal = !rif ? "null rif pointer"
                      : !field ? "null field pointer"
                      : !(grad || grad_field || dpos || dvel) ? "nothing to compute: grad, grad_field, dpos and dvel are all null"
                      : !dpos != !dvel ? "dpos and dvel go together"
                      : grad && grad == grad_field ? "grad and grad_field must be two arrays" : nullptr;
  const bool zero = !(flags & DRRT_FLAG_NO_ZERO);
  const int rc = cable_begin(a, refusal, rif, rres, radius, length, ds, zero ? grad : nullptr, stats, n, s);
  if (rc) return rc;
  if (zero && grad_field) {
    hipError_t e = hipMemsetAsync(grad_field, 0, rres * sizeof(float), s);
    if (e != hipSuccess) return fail_hip(e, "hipMemsetAsync(grad_field)");
  }
  if (n == 0) return rc;
  if (!pos || !xt || !vt) return fail(DRRT_ERR_ARG, "null ray pointer");
  if (!rec_steps) return fail(DRRT_ERR_ARG, "null rec_steps pointer (the forward's rec_steps)");
  a.field = field;
  a.pos = pos; a.xt = xt; a.vt = vt; a.rec_steps = rec_steps; a.dx = dx; a.dv = dv; a.dtau = dtau;
  a.grad = grad; a.grad_field = grad_field; a.dpos = dpos; a.dvel = dvel;
  return timed_launch(DRRT_PROF_BACKTRACE_CABLE_FIELD, s, "k_backtrace_cable_field", [&] { launch_backtrace_cable_field(a, s); });
}
