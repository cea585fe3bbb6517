// api_internal.h — what two or more of the api_*.cpp files (the C ABI of libm3d.so, include/m3d.h)
// share, and nothing else: a helper with one user lives in an anonymous namespace of that file.
// Host only; included by the api_*.cpp files alone, never by a .hip file or by m3d_internal.h.
//
// Where an entry point's device scratch comes from.  Five sources, each with its own rule:
//
//  1. Arena over ctx->scratch (with the RANSAC loop state ctx->rstate).  A bump allocator over one
//     context-owned buffer; growing it synchronises the device.  Every call on the context shares
//     it and each call only enqueues work on its caller's stream: a call on another stream than the
//     previous user first waits (device-side, ctx->scratch_ev) for that user's work and records its
//     own completion when it is done enqueueing, so calls on several streams are serialised on the
//     device and never race.  The one source an ASYNCHRONOUS call may draw from: it may return
//     without synchronising.  Users: m3d_kabsch3_batch / _one, m3d_ransac_score / _score_one,
//     m3d_ransac_run_async, m3d_plane_score, m3d_segment_plane.
//  2. ctx->tmp (m3d_internal.h TmpArena).  Temporaries of setup work — cloud packing, grid sorts and
//     occupancy, Morton copies, MFMA tiles, the k-NN ladder's grids — and of m3d_corr_pairs and
//     m3d_evaluate_registration.  Context-owned, grown on demand; an outgrown buffer is retired,
//     never freed under work in flight.  Consecutive users on ONE stream reuse it in stream order
//     without a host sync; nothing orders users on different streams, so a user either runs on the
//     null stream (icp_create's setup, synchronised before the loop object is handed out) or
//     synchronises its stream before it returns.
//  3. ctx->run (TmpArena).  The arrays of a loop object that dies inside the call — icp_create with
//     run_arena (m3d_icp_run, m3d_nn1, m3d_evaluate_registration, every side-terms call) and the
//     mesh ICP loop — instead of a hipMalloc / hipFree pair per call (≈ 0.2 ms: the free waits for the
//     device and unmaps).  Context-owned, kept between calls.  Only for a SYNCHRONOUS call: its
//     stream is idle when it returns, on every path.
//  4. prep_buffer over ctx->prep.  Neighbour lists and kernel scratch of the synchronous
//     preprocessing calls (a 180k-point cloud's lists at k = 30 take 65 MB, whose hipMalloc +
//     hipFree cost more than the normals kernel).  Context-owned, grown and never shrunk; growing
//     frees the old buffer.  Safe to reuse because those calls synchronise their stream before
//     returning and a context serves one host thread (m3d.h).  Users: voxel down-sampling, normals,
//     FPFH, k-NN, the outlier filters, DBSCAN, ISS and model resolution, thinning, and the grid
//     paths of m3d_mesh_closest and the ray casts.
//  5. DevTmp, an allocation of the call's own, freed on scope exit (hipFree waits for the device).
//     For a synchronous call whose scratch size follows its arguments and that must leave the
//     arena and the buffers above to the calls it makes: m3d_ransac_on_correspondences and the
//     m3d_fgr_* calls (the evaluation at the end of FGR uses ctx->tmp and ctx->run).
//
// Objects that outlive a call (clouds, grids, meshes, loop objects, a side-terms call's arrays) are
// none of these: they are blocks of the block cache (m3d_internal.h block_alloc, api_ctx.cpp).
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "m3d_internal.h"

#define CHECK_ARG(ctx, cond, msg) \
  do {                            \
    if (!(cond)) return m3d_fail((ctx), M3D_ERR_INVALID, (msg)); \
  } while (0)

#define HIPX(ctx, expr) M3D_HIP_CHECK(ctx, expr)

namespace m3d {
namespace api {

inline hipStream_t S(void* s) { return reinterpret_cast<hipStream_t>(s); }

constexpr float kFar = 1.0e18f;

inline int64_t round_up(int64_t v, int64_t m) { return (v + m - 1) / m * m; }

// (what, hipError_t, why) as the context's error: "what: why", or the HIP error's text (api_ctx.cpp)
int hip_fail(m3d_ctx* ctx, const char* what, hipError_t e, const std::string& why);

template <class T>
int dev_alloc(m3d_ctx* ctx, T** p, int64_t count) {
  *p = nullptr;
  if (count <= 0) return M3D_OK;
  hipError_t e = dev_malloc(reinterpret_cast<void**>(p), sizeof(T) * (size_t)count);
  if (e != hipSuccess) {
    *p = nullptr;
    return m3d_fail(ctx, M3D_ERR_OOM, std::string("hipMalloc: ") + hipGetErrorString(e));
  }
  return M3D_OK;
}

// device scratch released on scope exit (after the synchronous entry point has synchronised):
// source 5 above
template <class T>
struct DevTmp {
  T* p = nullptr;
  ~DevTmp() { hipFree(p); }
};

// Bump allocator over the context scratch arena: source 1 above.
struct Arena {
  m3d_ctx* ctx;
  hipStream_t st;
  size_t off = 0;
  Arena(m3d_ctx* c, hipStream_t s) : ctx(c), st(s) {
    if (ctx->scratch_ev != nullptr && ctx->scratch_used && ctx->scratch_stream != st)
      (void)hipStreamWaitEvent(st, ctx->scratch_ev, 0);
  }
  ~Arena() {
    if (ctx->scratch_ev != nullptr && hipEventRecord(ctx->scratch_ev, st) == hipSuccess) {
      ctx->scratch_used = true;
      ctx->scratch_stream = st;
    }
  }
  size_t take(size_t bytes) {
    size_t o = (off + 255) & ~size_t(255);
    off = o + bytes;
    return o;
  }
  int commit();  // api_ctx.cpp
  template <class T>
  T* at(size_t o) const {
    return reinterpret_cast<T*>(static_cast<char*>(ctx->scratch) + o);
  }
};

// mapped pinned memory of the context (api_ctx.cpp pin_ensure): kernels write their few results into
// it and the host reads them after one stream sync — no device-to-host copy (a pageable copy is a
// staging blit plus its own wait: ≈ 20 µs per readback on the cold path).  [0, kPinRead): the
// one-hypothesis results of api_ransac.cpp; from kPinRead on, pin_read's.
int pin_ensure(m3d_ctx* ctx);
constexpr size_t kPinRead = 2048;  // the cold path's readbacks: cloud summary, grid occupancy
template <class T>
T* pin_read(const m3d_ctx* ctx, bool dev) {
  return reinterpret_cast<T*>(static_cast<char*>(dev ? ctx->pin_dev : ctx->pin) + kPinRead);
}

// the context's preprocessing buffer with at least `need` bytes (grown, never shrunk): source 4
// above (api_ctx.cpp)
int prep_buffer(m3d_ctx* ctx, size_t need, char** out);

// api_cloud.cpp: a cloud's grid at cell size `cell`, and its copy in Morton slot order with that
// copy's query grid; both built once and cached on the cloud
int ensure_grid(m3d_ctx* ctx, const m3d_cloud* c, double cell, hipStream_t st, const Grid** out);
int ensure_morton_source(m3d_ctx* ctx, const m3d_cloud* c, double cell, const m3d_cloud** out, const Grid** gout);

// api_prep.cpp: the grids of a hybrid search
int search_grids(m3d_ctx* ctx, const m3d_cloud* c, double radius, int k, hipStream_t st, const Grid** g,
                 const Grid** gf, double* hf);

// api_terms.cpp: a caller's robust kernel is a known kind with a usable k
int robust_check(m3d_ctx* ctx, const m3d_robust_kernel* kernel);

// api_icp.cpp: the loop object and the pieces of a one-shot call around it
int icp_create(m3d_ctx* ctx, const m3d_cloud* src, const m3d_cloud* tgt, double max_dist,
               const m3d_icp_params* params, m3d_icp** out, bool run_arena);
hipError_t enqueue_nn(m3d_icp* s, int64_t off, hipStream_t st, bool self_seed = false, int64_t q0 = 0,
                      int64_t q1 = -1, bool with_terms = false);
bool apply_init_of(const double* T, bool open3d_init);
int icp_reset(m3d_icp* s, const double* init, bool open3d_init, void* stream);
int defer_fault(m3d_ctx* ctx, uint32_t count, bool fault);
int read_result(m3d_ctx* ctx, const char* what, const IcpState* state, const uint32_t* hcnt, m3d_icp_result* out,
                hipStream_t st);
int finish_run(m3d_icp* s, m3d_icp_result* out, int32_t* corr_idx, hipStream_t st);
int fill_unmatched(m3d_ctx* ctx, int64_t ns, int32_t* corr_idx, double* d2, hipStream_t st);

inline constexpr double kIdentity16[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};

// the parameters of a loop object that only searches (one evaluation, no iteration)
inline m3d_icp_params probe_params(int32_t estimation, int32_t nn_method) {
  return m3d_icp_params{1e-6, 1e-6, 0, estimation, nn_method, 0};
}

// the throw-away loop of one call: destroyed when the call returns, on every path
struct ScopedLoop {
  m3d_icp* s = nullptr;
  ~ScopedLoop() { m3d_icp_destroy(s); }
  m3d_icp* operator->() const { return s; }
  operator m3d_icp*() const { return s; }
};

// `total` evaluations, step(k) enqueueing the next k of them, in growing chunks (4, 8, 16, …)
// with a look at the state's `done` between chunks — a converged loop (often after a handful of
// evaluations) then does not enqueue the remaining ~2 launches per evaluation that would only
// read `done` and return.  The evaluations that run are the same; only the early-exit launches
// are skipped.
template <class Step>
int run_chunked(m3d_ctx* ctx, const IcpState* state, int32_t total, Step step, hipStream_t st) {
  int32_t left = total, chunk = 4;
  while (left > 0) {
    const int32_t k = std::min(chunk, left);
    const int rc = step(k);
    left -= k;
    chunk *= 2;
    if (rc || left == 0) return rc;
    int32_t done = 0;
    hipError_t e = hipMemcpyAsync(&done, &state->done, sizeof(done), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return m3d_fail(ctx, M3D_ERR_HIP, hipGetErrorString(e));
    if (done) break;
  }
  return M3D_OK;
}
template <class Step>
int run_chunked(m3d_icp* s, int32_t total, Step step, hipStream_t st) {
  return run_chunked(s->ctx, s->state, total, step, st);
}

// One evaluation at the transform T: reset, NN scan, the caller's pass over the scan, the
// correspondences in the caller's source order (corr_idx null: none), one stream sync.
// n > 0: pass(out) leaves n doubles in `out`, the context's mapped pinned memory, the last two the
// grid scan's deferral count and fault word (launch_reduce) — the sums and the fault word land
// together, one stream sync brings both back with no device-to-host copy — copied into sums
// unless the fault word is set.  n = 0: pass(nullptr), nothing read back.
template <class Pass>
int one_evaluation(m3d_icp* s, const double* T, bool open3d_init, Pass pass, int32_t* corr_idx, int n,
                   double* sums, hipStream_t st) {
  m3d_ctx* ctx = s->ctx;
  int rc = n > 0 ? pin_ensure(ctx) : M3D_OK;
  if (!rc) rc = icp_reset(s, T, open3d_init, st);
  if (rc) return rc;
  hipError_t e = enqueue_nn(s, 0, st);
  s->points_moved = true;  // the pass is a terms pass
  if (e == hipSuccess) e = pass(n > 0 ? pin_read<double>(ctx, true) : nullptr);
  if (e == hipSuccess && corr_idx != nullptr) e = launch_scatter_i32(s->corr, s->src->slot, s->src->n, corr_idx, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return m3d_fail(ctx, M3D_ERR_HIP, hipGetErrorString(e));
  if (n == 0) return M3D_OK;
  const volatile double* h = pin_read<double>(ctx, false);
  for (int k = 0; k < n; ++k) sums[k] = h[k];
  return defer_fault(ctx, (uint32_t)sums[n - 2], sums[n - 1] != 0.0);
}

}  // namespace api
}  // namespace m3d
