// api_icp.cpp — the ICP loop object of the C ABI (include/m3d.h): create / destroy / reset, the step and its
// graph capture, the shard entries, solve and result read; the synchronous one-shot calls around a
// throw-away loop (m3d_icp_run, m3d_nn1, m3d_evaluate_registration); the loop's test hooks.  The
// per-step host path (m3d_icp_step(s), capture_steps, enqueue_nn, fused_tail, the shard entries) is
// all in this translation unit.
#include <string.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "api_internal.h"

using namespace m3d;
using namespace m3d::api;

namespace {
// Dense target cells (a cell at ≈ r holding ≥ kHeavyCell points — e.g. the vertex fan at a
// UV-sphere pole, ~30× the mean density): queries with more than kHeavyCand candidates are
// deferred to grid_nn_heavy_kernel (one block per query) so that the few waves of such queries
// do not set the launch time (cfg4: up to 250 µs per evaluation).  M3D_GRID_HEAVY=0: never,
// =N: always, with cap N (tests).  Off on evenly dense clouds (cfg1's largest cell ≈ 20).
int32_t heavy_cap(const m3d_icp_params* params, int64_t coarse_max_occ) {
  constexpr int64_t kHeavyCell = 256;
  constexpr int32_t kHeavyCand = 256;
  static const int heavy_env = [] {
    const char* e = getenv("M3D_GRID_HEAVY");
    return e ? std::max(0, atoi(e)) : -1;
  }();
  if (params->nn_method != M3D_NN_GRID) return 0;
  return heavy_env > 0 ? heavy_env : (heavy_env < 0 && coarse_max_occ >= kHeavyCell ? kHeavyCand : 0);
}

// Eigen's Matrix4d::isIdentity() (dummy precision 1e-12), as RegistrationICP tests its init:
// |a_ii − 1| ≤ 1e-12·min(|a_ii|, 1), |a_ij| ≤ 1e-12
bool eigen_is_identity(const double* T) {
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) {
      const double a = T[4 * i + j];
      if (i == j ? !(std::fabs(a - 1.0) <= 1e-12 * std::min(std::fabs(a), 1.0)) : !(std::fabs(a) <= 1e-12))
        return false;
    }
  return true;
}

// Whether an iteration's tail runs as ONE launch (terms + last-block reduce [+ solve]).  The
// fused last block reduces every block partial alone, with 256 threads: past ~256 blocks the
// separate 1024-thread reduce_kernel is faster (1M sources, grid loop: fused 60.7 µs against
// terms 33.1 + reduce 8.8 + solve 6.5 µs, rocprof).  Where the fused tail hands the keys back
// (brute force: the next scan then seeds itself, no keyinit launch) it stays fused.  Both forms
// sum in the same fixed order: the same bits.
bool fused_tail(const m3d_icp* s, bool keys_back) {
  static const bool env = [] {
    const char* e = getenv("M3D_ICP_FUSED");
    return !(e && atoi(e) == 0);
  }();
  return env && (keys_back || s->nblocks <= 256);
}

// M3D_NN_TERMS=0 in the environment: the terms pass never runs inside the NN launch
bool nn_terms_env() {
  static const bool on = [] {
    const char* e = getenv("M3D_NN_TERMS");
    return !(e && atoi(e) == 0);
  }();
  return on;
}

// m3d_icp_step's view of a loop for nn_terms_selected (it passes no claim)
NnTermsSel nn_terms_sel(const m3d_icp* s, bool fused, bool reset) {
  NnTermsSel c;
  c.planned = s->params.nn_method == M3D_NN_BRUTE && s->nn_targs != nullptr && icp_nn_planned(s);
  c.fused = fused;
  c.reset = reset;
  c.p2plane = s->params.estimation == M3D_EST_POINT_TO_PLANE;
  c.rec64 = s->tgt->rec64 != nullptr;
  c.seed = s->seed != nullptr;
  c.claim = false;
  c.one_device = s->ns_total == 0;
  c.on = nn_terms_env() && !s->nn_terms_off;
  return c;
}

// n steps as ONE graph launch: the sequence (NN scan [+ keyinit] + fused tail per step, 2–3
// kernels each) is captured on a loop-owned stream the second time the same (n, keys_clean on
// entry) is requested — a one-shot run never pays the capture — and then replayed on the
// caller's stream — the per-kernel host enqueues and the stream's per-dispatch
// gaps become one graph launch.  Every kernel argument is a device pointer into the loop's state,
// so a replay computes exactly what the enqueued steps would (tests: test_gpu_icp graph cases).
// Not used while kernel profiling records events, or after a failed capture (plain enqueues).
bool icp_graphs_on() {
  static const bool on = [] {
    const char* e = getenv("M3D_ICP_GRAPH");
    return !(e && atoi(e) == 0);
  }();
  return on;
}

int capture_steps(m3d_icp* s, int32_t n) {
  if (s->cap_stream == nullptr &&
      hipStreamCreateWithFlags(&s->cap_stream, hipStreamNonBlocking) != hipSuccess) {
    s->cap_stream = nullptr;
    return M3D_ERR_HIP;
  }
  const bool kc0 = s->keys_clean, pm0 = s->points_moved;
  const int slot = kc0 ? 1 : 0;
  if (hipStreamBeginCapture(s->cap_stream, hipStreamCaptureModeThreadLocal) != hipSuccess)
    return M3D_ERR_HIP;
  int rc = M3D_OK;
  for (int32_t k = 0; k < n && rc == M3D_OK; ++k) rc = m3d_icp_step(s, s->cap_stream);
  hipGraph_t g = nullptr;
  const hipError_t ee = hipStreamEndCapture(s->cap_stream, &g);
  const bool kc1 = s->keys_clean;
  s->keys_clean = kc0;  // nothing ran yet
  s->points_moved = pm0;
  hipGraphExec_t ex = nullptr;
  if (rc == M3D_OK && ee == hipSuccess && g != nullptr &&
      hipGraphInstantiate(&ex, g, nullptr, nullptr, 0) == hipSuccess) {
    if (s->graph[slot] != nullptr) hipGraphExecDestroy(s->graph[slot]);
    s->graph[slot] = ex;
    s->graph_n[slot] = n;
    s->graph_kc_out[slot] = kc1;
  } else {
    rc = rc ? rc : M3D_ERR_HIP;
  }
  if (g != nullptr) hipGraphDestroy(g);
  (void)hipGetLastError();
  return rc;
}

// GᵀG of the rows G₁ = (0, z, −y, 1, 0, 0), G₂ = (−z, 0, x, 0, 1, 0), G₃ = (y, −x, 0, 0, 0, 1) over
// the matched target points, from eval.hip's sums m = (count, Σd², Σx Σy Σz, Σx² Σy² Σz², Σxy Σxz Σyz)
void eval_information(const double* m, double* G) {
  const double n = m[0], x = m[2], y = m[3], z = m[4], xx = m[5], yy = m[6], zz = m[7], xy = m[8],
               xz = m[9], yz = m[10];
  const double U[6][6] = {{yy + zz, 0.0 - xy, 0.0 - xz, 0.0, 0.0 - z, y},
                          {0.0, xx + zz, 0.0 - yz, z, 0.0, 0.0 - x},
                          {0.0, 0.0, xx + yy, 0.0 - y, x, 0.0},
                          {0.0, 0.0, 0.0, n, 0.0, 0.0},
                          {0.0, 0.0, 0.0, 0.0, n, 0.0},
                          {0.0, 0.0, 0.0, 0.0, 0.0, n}};
  for (int a = 0; a < 6; ++a)
    for (int b = 0; b < 6; ++b) G[6 * a + b] = a <= b ? U[a][b] : U[b][a];
}
}  // namespace

namespace m3d {
namespace api {
// NN evaluation for the current transform → s->keys (brute: keyinit + scan; grid: one kernel).
// self_seed (m3d_icp_step's fused loop): when the previous fused tail left every key at
// kKeyNone (s->keys_clean), the brute-force scan seeds itself and the keyinit launch is skipped.
// [q0, q1): a slot range of the sources (q1 < 0: all), see icp_nn_splits.
// with_terms: the NN kernel that also runs the terms pass (m3d_icp_step, nn_terms_selected).
hipError_t enqueue_nn(m3d_icp* s, int64_t off, hipStream_t st, bool self_seed, int64_t q0, int64_t q1,
                      bool with_terms) {
  m3d_ctx* ctx = s->ctx;
  const bool whole = q0 == 0 && (q1 < 0 || q1 == s->src->n);
  const bool seeded = self_seed && s->keys_clean && off == 0 && whole;
  s->keys_clean = false;
  if (s->params.nn_method == M3D_NN_GRID) {
    KTimer kt(ctx, M3D_KERNEL_NN, st);
    return launch_grid_nn(s->src->xyz32, s->src->n, s->sgrid, s->tgrid, off, s->state, s->keys,
                          s->near2, s->corr, s->dprev, s->tgt->xyz32, s->tgt->n, st, q0, q1,
                          s->hlist, s->hcnt, s->cand_cap, s->pcd64, s->tgt->xyz64, s->hcap, s->scan_xchunk);
  }
  if (!seeded) {
    hipError_t e = launch_icp_keyinit(s, off, st, q0, q1);
    if (e != hipSuccess) return e;
  }
  KTimer kt(ctx, M3D_KERNEL_NN, st);
  return launch_icp_nn(s, off, seeded, st, q0, q1, with_terms);
}

// run_arena: the loop's arrays come from the context's run arena instead of their own block — for the
// synchronous one-shot entry points, whose loop object dies inside the call (api_internal.h, source 3)
int icp_create(m3d_ctx* ctx, const m3d_cloud* src, const m3d_cloud* tgt, double max_dist,
               const m3d_icp_params* params, m3d_icp** out, bool run_arena) {
  if (!ctx) return M3D_ERR_INVALID;
  CHECK_ARG(ctx, src && tgt && params && out, "invalid arguments");
  CHECK_ARG(ctx, max_dist > 0.0, "Invalid max_correspondence_distance.");
  CHECK_ARG(ctx, params->estimation == M3D_EST_POINT_TO_PLANE ||
                     params->estimation == M3D_EST_POINT_TO_POINT,
            "unknown estimation");
  CHECK_ARG(ctx, params->estimation != M3D_EST_POINT_TO_PLANE || tgt->nrm64 != nullptr || tgt->n == 0,
            "TransformationEstimationPointToPlane requires pre-computed normal vectors for target "
            "PointCloud.");
  CHECK_ARG(ctx, params->max_iteration >= 0, "max_iteration must be >= 0");
  CHECK_ARG(ctx, params->nn_method == M3D_NN_BRUTE || params->nn_method == M3D_NN_GRID,
            "unknown nn_method");
  hipSetDevice(ctx->device);
  const Grid *tg = nullptr, *sg = nullptr;
  const m3d_cloud* src_m = nullptr;
  int64_t coarse_max_occ = 0;  // most target points in one cell at cell ≈ r (grid NN)
  int32_t cand_cap = 0;
  m3d_icp* s = new m3d_icp();
  {
    // Grid NN: cell ≈ the search radius, a query visits 3 cells per axis.  Brute force: the
    // same grids only ORDER the points (targets and queries in cell order make the MFMA
    // screen's 32-target sub-tiles and 64-query waves spatially compact, and let the box cull of
    // nn_mfma_kernel skip the tiles a query block cannot reach); every pair is still screened or
    // excluded by a proven box bound.
    const double cell = max_dist * 1.001;
    int grc = ensure_grid(ctx, tgt, cell, nullptr, &tg);
    // the loop runs on the source in Morton slot order (sg: the copy's query grid)
    const m3d_cloud* ms = nullptr;
    if (!grc) grc = ensure_morton_source(ctx, src, cell, &ms, &sg);
    if (!grc) src_m = ms;
    if (!grc) {
      hipError_t e = ensure_target_rec(tgt, nullptr);
      if (e != hipSuccess) grc = m3d_fail(ctx, M3D_ERR_HIP, std::string("target records: ") + hipGetErrorString(e));
    }
    // (after the source grid, Morton copy and target records are enqueued: the occupancy's one
    // sync then also covers them instead of stalling the queue in between)
    // Grid NN on a dense target: a seeded query's box is ~1–2 cells per axis, so the candidates
    // it scans grow with the points per cell.  Shrink the target cell by div = ⌊√(m / 3.5)⌋
    // (m = points per occupied cell at cell ≈ r; any cell size gives the same keys, grid.hip):
    // measured (tools/grid_cell_sweep.sh) 1M × 1M (m ≈ 33) 206 → 128 µs per scan at div 3;
    // cfg1 (m ≈ 3.9) and the 1M × 125k shard (m ≈ 4.7) are fastest at div 1.
    if (!grc && params->nn_method == M3D_NN_GRID) {
      hipError_t e = pin_ensure(ctx) == M3D_OK ? hipSuccess : hipErrorOutOfMemory;
      if (e == hipSuccess)  // one sync, once per grid
        e = grid_occupancy(const_cast<Grid*>(tg), &ctx->tmp, nullptr, pin_read<unsigned long long>(ctx, true),
                           pin_read<unsigned long long>(ctx, false));
      if (e != hipSuccess) grc = m3d_fail(ctx, M3D_ERR_HIP, std::string("grid occupancy: ") + hipGetErrorString(e));
    }
    if (!grc && params->nn_method == M3D_NN_GRID && tg->n_occ > 0) {
      coarse_max_occ = tg->max_occ;
      const double m = (double)tg->n_pts / (double)tg->n_occ;
      const int div = std::min(4, std::max(1, (int)std::floor(std::sqrt(m / 3.5))));
      if (div > 1) grc = ensure_grid(ctx, tgt, cell / div, nullptr, &tg);
    }
    if (!grc) {  // the terms pass's fp64 walk for ambiguous queries (nnkey.h resolve_wave)
      hipError_t e = build_grid_pts64(tgt, const_cast<Grid*>(tg), nullptr);
      if (e != hipSuccess) grc = m3d_fail(ctx, M3D_ERR_HIP, std::string("grid fp64 points: ") + hipGetErrorString(e));
    }
    if (!grc && params->nn_method == M3D_NN_BRUTE && tg->mf16 == nullptr) {
      hipError_t e = build_mfma_tiles(tgt, const_cast<Grid*>(tg), &ctx->tmp, nullptr);
      if (e != hipSuccess) grc = m3d_fail(ctx, M3D_ERR_HIP, std::string("mfma tiles: ") + hipGetErrorString(e));
    }
    // the loop's arrays in ONE block (from the block cache: a reused block's release mark is
    // waited for on the null stream, and so covered by the sync below)
    if (!grc) {
      cand_cap = heavy_cap(params, coarse_max_occ);
      const size_t n1 = (size_t)std::max<int64_t>(src->n, 1);
      Carve cv;
      cv.add(&s->state, 1);
      if (params->nn_method == M3D_NN_BRUTE) nn_plan_shape(src->n, &s->nn_qblocks, &s->nn_budget);
      if (s->nn_qblocks > 0) {  // the brute-force NN's slice plan (nn_plan.h), on the state's page: the fused
                                // tail's last block reads both
        cv.add(&s->nn_cnt, 2 * (size_t)s->nn_qblocks);  // and nn_tix behind it
        cv.add(&s->nn_targs, (nn_terms_dev_bytes() + 7) / 8);
        cv.add(&s->nn_seen, (size_t)s->nn_qblocks);
        cv.add(&s->nn_table, (size_t)s->nn_budget);
      }
      cv.add(&s->keys, n1);
      cv.add(&s->near2, n1);
      cv.add(&s->dprev, n1);
      cv.add(&s->ld64, n1);
      cv.add(&s->lidx, n1);
      cv.add(&s->corr, n1);
      if (params->nn_method == M3D_NN_BRUTE) cv.add(&s->seed, n1);
      cv.add(&s->partials, (size_t)(terms_blocks(src->n) * kTermSlots + kTermSlots));  // + the sums
      if (cand_cap > 0) {  // the deferral list and its header (count, ticket, fault)
        cv.add(&s->hlist, n1);
        cv.add(&s->hcnt, kDeferWords);
        s->hcap = (int32_t)n1;
      }
      cv.add(&s->pcd64, 3 * n1);
      size_t tot = 0;
      hipError_t e = run_arena ? ctx->run.reserve(cv.bytes()) : cv.alloc(&s->block, &tot, nullptr);
      if (e != hipSuccess) grc = m3d_fail(ctx, M3D_ERR_OOM, "device allocation failed (ICP loop arrays)");
      if (!grc && run_arena) cv.place(ctx->run.base);
    }
    // the deferral list's count / ticket / fault word start at zero BEFORE the sync below: a block
    // from the cache may hold any bytes of its previous owner (e.g. 0xFF fills), and a memset left
    // queued on the null stream is not ordered before a caller's non-blocking stream
    // (grid_nn_heavy_kernel re-zeroes count + ticket, icp_reset all)
    if (!grc && s->hcnt != nullptr &&
        hipMemsetAsync(s->hcnt, 0, kDeferWords * sizeof(uint32_t), nullptr) != hipSuccess)
      grc = m3d_fail(ctx, M3D_ERR_HIP, "loop arrays: deferral counter");
    // likewise the NN plan's tile counters (the planner re-zeroes them, and every reset of the loop's
    // state: launch_icp_reset, launch_icp_set_T)
    if (!grc && s->nn_cnt != nullptr &&
        hipMemsetAsync(s->nn_cnt, 0, 2 * (size_t)s->nn_qblocks * sizeof(uint32_t), nullptr) != hipSuccess)
      grc = m3d_fail(ctx, M3D_ERR_HIP, "loop arrays: NN plan counters");
    // the terms arguments nn_mfma_terms_kernel reads from device memory: constants of the loop
    if (!grc && s->nn_cnt != nullptr) {
      s->nn_tix = s->nn_cnt + s->nn_qblocks;
      s->src = src_m;
      s->tgt = tgt;
      s->tgrid = tg;
      s->params = *params;
      if (launch_nn_terms_setup(s, nullptr) != hipSuccess)
        grc = m3d_fail(ctx, M3D_ERR_HIP, "loop arrays: NN terms arguments");
    }
    // the setup above ran asynchronously on the null stream: finish it before the loop object is
    // used on the caller's streams
    if (!grc) {
      hipError_t e = hipStreamSynchronize(nullptr);
      if (e != hipSuccess) grc = m3d_fail(ctx, M3D_ERR_HIP, std::string("loop setup: ") + hipGetErrorString(e));
    }
    if (grc) {
      block_release(s->block);
      delete s;
      return grc;
    }
  }
  s->ctx = ctx;
  s->ctx_id = ctx->id;
  s->src = src_m;
  src_m->refs += 1;  // the Morton copy stays cached while this loop runs on it
  s->user_src = src;
  s->tgt = tgt;
  s->params = *params;
  s->max_dist = max_dist;
  s->nblocks = terms_blocks(src->n);
  s->tgrid = tg;
  // brute-force query order: the Morton slots themselves (compact 64-query waves, contiguous
  // slot ranges for the split exchange of the target-shard loop)
  s->sgrid = sg;
  s->cand_cap = cand_cap;
  // a target whose extent along some axis is under half the source's (a spatial shard, m3d.dist
  // spatial_shards): the scan's real work concentrates in the Morton ranges near the target, so its
  // blocks go to the XCDs in chunks of 8 (tools/xchunk_sweep.sh: 8 slabs of 1M × 1M, per-shard
  // scan 39.8 → 32.6 µs; a whole-extent target keeps one contiguous eighth per XCD)
  if (src->has_bounds && tgt->has_bounds)
    for (int k = 0; k < 3; ++k)
      if ((double)(tgt->hi[k] - tgt->lo[k]) * 2.0 < (double)(src->hi[k] - src->lo[k])) s->scan_xchunk = 8;
  s->sums = s->partials + s->nblocks * kTermSlots;
  *out = s;
  return M3D_OK;
}

// RegistrationICP (Registration.cpp): pcd = source; if (!init.isIdentity()) pcd.Transform(init) —
// whether a loop's points start as init·p, decided here for the cloud loops and the mesh loop alike
// (open3d_init false: always)
bool apply_init_of(const double* T, bool open3d_init) { return !(open3d_init && eigen_is_identity(T)); }

int icp_reset(m3d_icp* s, const double* init, bool open3d_init, void* stream) {
  if (!s) return M3D_ERR_INVALID;
  Touch tch{s->ctx, S(stream)};
  m3d_ctx* ctx = s->ctx;
  const double* T = init ? init : kIdentity16;
  hipSetDevice(ctx->device);
  hipStream_t st = S(stream);
  HIPX(ctx, hipMemsetAsync(s->corr, 0xFF, sizeof(int32_t) * std::max<int64_t>(s->src->n, 1), st));
  // all-ones bits = a NaN distance: no bound seed until a target-shard exchange wrote dprev
  HIPX(ctx, hipMemsetAsync(s->dprev, 0xFF, sizeof(int64_t) * std::max<int64_t>(s->src->n, 1), st));
  // the deferral list's count, ticket and fault word start at zero on the caller's stream (the
  // heavy kernel re-zeroes count and ticket after each scan; a reset also clears a fault)
  if (s->hcnt != nullptr) HIPX(ctx, hipMemsetAsync(s->hcnt, 0, kDeferWords * sizeof(uint32_t), st));
  HIPX(ctx, launch_icp_reset(s, T, apply_init_of(T, open3d_init), st));
  s->keys_clean = false;
  s->points_moved = false;
  return M3D_OK;
}

// the grid scan's deferral list overflowed (a count the scan found larger than the list — the
// loop's own writes were dropped, never out of bounds): the keys of this run are not trustworthy.
// count / fault: the list header's words (m3d_icp::hcnt), however they reached the host
int defer_fault(m3d_ctx* ctx, uint32_t count, bool fault) {
  if (!fault) return M3D_OK;
  return m3d_fail(ctx, M3D_ERR_HIP,
                  "grid NN deferral list overflow (count " + std::to_string(count) +
                      "): results since the last m3d_icp_reset are invalid");
}

// The result of a loop: its state and — hcnt given — the grid scan's deferral header copied back on
// st, one stream sync (on every path: the stream is idle when this returns), the deferral fault,
// then the fields.  what: the caller's name in a HIP error's text.
int read_result(m3d_ctx* ctx, const char* what, const IcpState* state, const uint32_t* hcnt, m3d_icp_result* out,
                hipStream_t st) {
  IcpState h;
  uint32_t defer[kDeferWords] = {0, 0, 0, 0};
  hipError_t e = hipMemcpyAsync(&h, state, sizeof(h), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && hcnt != nullptr) e = hipMemcpyAsync(defer, hcnt, sizeof(defer), hipMemcpyDeviceToHost, st);
  const hipError_t es = hipStreamSynchronize(st);
  if (e == hipSuccess) e = es;
  if (e != hipSuccess) return m3d_fail(ctx, M3D_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
  if (const int rc = defer_fault(ctx, defer[0], defer[kDeferFault] != 0)) return rc;
  for (int k = 0; k < 16; ++k) {
    out->T[k] = h.T[k];
    out->update[k] = h.last_upd[k];
  }
  out->fitness = h.fitness;
  out->inlier_rmse = h.rmse;
  out->num_correspondences = h.count;
  out->iterations = h.iters;
  out->converged = h.converged;
  return M3D_OK;
}

// after the evaluations: the result, and the correspondences in the caller's source order
int finish_run(m3d_icp* s, m3d_icp_result* out, int32_t* corr_idx, hipStream_t st) {
  const int rc = m3d_icp_result_get(s, out, st);
  if (rc || !corr_idx || s->src->n == 0) return rc;
  hipError_t e = launch_scatter_i32(s->corr, s->src->slot, s->src->n, corr_idx, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  return e == hipSuccess ? M3D_OK : m3d_fail(s->ctx, M3D_ERR_HIP, hipGetErrorString(e));
}

// nothing to search (an empty source or target): every source (if any) is unmatched — corr_idx and
// d2 (non-null) filled —, one stream sync
int fill_unmatched(m3d_ctx* ctx, int64_t ns, int32_t* corr_idx, double* d2, hipStream_t st) {
  hipSetDevice(ctx->device);
  hipError_t e = launch_eval_fill(ns, corr_idx, d2, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return m3d_fail(ctx, M3D_ERR_HIP, hipGetErrorString(e));
  return M3D_OK;
}
}  // namespace api
}  // namespace m3d

int m3d::icp_shard_nn_range(m3d_icp* s, int64_t off, int64_t q0, int64_t q1, int64_t* dkeys, hipStream_t st) {
  hipError_t e = enqueue_nn(s, off, st, false, q0, q1);
  if (e == hipSuccess) e = launch_shard_winner(s, off, dkeys, st, q0, q1);
  if (e != hipSuccess) return m3d_fail(s->ctx, M3D_ERR_HIP, std::string("shard NN: ") + hipGetErrorString(e));
  return M3D_OK;
}

extern "C" {

// ------------------------------------------------------------------------------- ICP
int m3d_icp_create(m3d_ctx* ctx, const m3d_cloud* src, const m3d_cloud* tgt, double max_dist,
                   const m3d_icp_params* params, m3d_icp** out) {
  return icp_create(ctx, src, tgt, max_dist, params, out, false);
}

void m3d_icp_destroy(m3d_icp* s) {
  if (!s) return;
  for (hipGraphExec_t g : s->graph)
    if (g != nullptr) hipGraphExecDestroy(g);
  if (s->cap_stream != nullptr) hipStreamDestroy(s->cap_stream);
  if (s->src != nullptr) {
    m3d_cloud* ms = const_cast<m3d_cloud*>(s->src);
    if (--ms->refs == 0 && ms->orphan) m3d_cloud_destroy(ms);  // its parent cloud is gone
  }
  {
    ReleaseScope rs(s->ctx, s->ctx_id);  // back to the block cache, marked after the loop's work
    block_release(s->block);             // state, keys, near2, dprev, ld64, lidx, corr, partials, sums
  }
  hipFree(s->xdk);
  hipFree(s->xcl);
  hipFree(s->xsums);
  delete s;
}

int m3d_icp_reset(m3d_icp* s, const double* init, void* stream) { return icp_reset(s, init, true, stream); }

int m3d_icp_copy_points(const m3d_icp* s, double* dst, void* stream) {
  if (!s || (!dst && s->src->n > 0)) return M3D_ERR_INVALID;
  Touch tch{s->ctx, S(stream)};
  HIPX(s->ctx, launch_copy_points(s, dst, S(stream)));
  return M3D_OK;
}

int m3d_icp_step(m3d_icp* s, void* stream) {
  if (!s) return M3D_ERR_INVALID;
  Touch tch{s->ctx, S(stream)};
  m3d_ctx* ctx = s->ctx;
  hipStream_t st = S(stream);
  // brute force: the fused tail hands the keys back as kKeyNone, the next NN seeds itself
  const bool reset = s->params.nn_method != M3D_NN_GRID && s->src->n > 0;
  const bool fused = fused_tail(s, reset);
  s->points_moved = true;  // every path below enqueues a terms pass
  if (nn_terms_selected(nn_terms_sel(s, fused, reset))) {
    // the terms pass runs inside the NN launch, query block by query block; what is left is one
    // block: reduce, solve, plan (the M3D_KERNEL_TERMS events then time that block alone)
    HIPX(ctx, enqueue_nn(s, 0, st, true, 0, -1, true));
    KTimer kt(ctx, M3D_KERNEL_TERMS, st);
    HIPX(ctx, launch_icp_reduce_solve_block(s, st));
    s->keys_clean = true;
    return M3D_OK;
  }
  HIPX(ctx, enqueue_nn(s, 0, st, fused));
  if (fused) {
    KTimer kt(ctx, M3D_KERNEL_TERMS, st);
    HIPX(ctx, launch_icp_terms_solve(s, reset, st));
    s->keys_clean = reset;
    return M3D_OK;
  }
  { KTimer kt(ctx, M3D_KERNEL_TERMS, st); HIPX(ctx, launch_icp_terms_mode(s, 0, nullptr, nullptr, st)); }
  HIPX(ctx, launch_icp_reduce_solve(s, st));
  return M3D_OK;
}

int m3d_icp_prepare_steps(m3d_icp* s, int32_t n) {
  if (!s) return M3D_ERR_INVALID;
  CHECK_ARG(s->ctx, n >= 0, "n must be >= 0");
  if (n < 2 || !icp_graphs_on() || s->graph_off) return M3D_OK;  // plain enqueues then
  hipSetDevice(s->ctx->device);
  if (capture_steps(s, n) != M3D_OK) {
    s->graph_off = true;
    (void)hipGetLastError();
  }
  return M3D_OK;
}

int m3d_icp_steps(m3d_icp* s, int32_t n, void* stream) {
  if (!s) return M3D_ERR_INVALID;
  Touch tch{s->ctx, S(stream)};
  CHECK_ARG(s->ctx, n >= 0, "n must be >= 0");
  if (n >= 2 && icp_graphs_on() && !s->graph_off && !s->ctx->profiling) {
    const int slot = s->keys_clean ? 1 : 0;
    const bool have = s->graph[slot] != nullptr && s->graph_n[slot] == n;
    const bool again = s->seen_n[slot] == n;
    s->seen_n[slot] = n;
    if (!have && again) {
      hipSetDevice(s->ctx->device);
      if (capture_steps(s, n) != M3D_OK) s->graph_off = true;
    }
    if ((have || again) && !s->graph_off) {
      HIPX(s->ctx, hipGraphLaunch(s->graph[slot], S(stream)));
      s->keys_clean = s->graph_kc_out[slot];
      s->points_moved = true;
      return M3D_OK;
    }
  }
  for (int32_t k = 0; k < n; ++k) {
    const int rc = m3d_icp_step(s, stream);
    if (rc) return rc;
  }
  return M3D_OK;
}

int m3d_icp_shard_nn(m3d_icp* s, int64_t off, int64_t* dkeys, void* stream) {
  if (!s) return M3D_ERR_INVALID;
  Touch tch{s->ctx, S(stream)};
  m3d_ctx* ctx = s->ctx;
  CHECK_ARG(ctx, off >= 0, "negative shard offset");
  CHECK_ARG(ctx, dkeys != nullptr || off == 0, "a target shard (offset > 0) needs the dkeys exchange buffer");
  hipStream_t st = S(stream);
  // dkeys == NULL: source-sharded protocol, the keys stay inside and the keyinit-free scan may
  // run; else target shard: this shard's fp64 winners → the MIN exchange buffer
  HIPX(ctx, enqueue_nn(s, off, st, dkeys == nullptr));
  if (dkeys != nullptr) HIPX(ctx, launch_shard_winner(s, off, dkeys, st));
  return M3D_OK;
}

int m3d_icp_shard_nn_range(m3d_icp* s, int64_t off, int64_t q0, int64_t q1, int64_t* dkeys, void* stream) {
  if (!s) return M3D_ERR_INVALID;
  Touch tch{s->ctx, S(stream)};
  m3d_ctx* ctx = s->ctx;
  CHECK_ARG(ctx, off >= 0, "negative shard offset");
  CHECK_ARG(ctx, dkeys != nullptr, "null dkeys");
  CHECK_ARG(ctx, 0 <= q0 && q0 <= q1 && q1 <= s->src->n, "slot range outside [0, ns]");
  CHECK_ARG(ctx, icp_nn_range_ok(s), "this loop's NN cannot run on a slot range (grid search without a Morton query grid)");
  return icp_shard_nn_range(s, off, q0, q1, dkeys, S(stream));
}

int m3d_icp_shard_claim(m3d_icp* s, const int64_t* dmin, int32_t* claim, void* stream) {
  if (!s) return M3D_ERR_INVALID;
  Touch tch{s->ctx, S(stream)};  // reads the loop's block: its release mark must cover this launch
  CHECK_ARG(s->ctx, dmin != nullptr && claim != nullptr, "null exchange buffer");
  HIPX(s->ctx, launch_shard_claim(s, dmin, claim, S(stream)));
  return M3D_OK;
}

int m3d_icp_shard_terms(m3d_icp* s, int64_t off, const int64_t* dmin, const int32_t* claim,
                        double* sums, void* stream) {
  if (!s) return M3D_ERR_INVALID;
  Touch tch{s->ctx, S(stream)};
  m3d_ctx* ctx = s->ctx;
  CHECK_ARG(ctx, sums != nullptr, "null sums");
  CHECK_ARG(ctx, (dmin == nullptr) == (claim == nullptr), "dmin and claim go together");
  CHECK_ARG(ctx, claim != nullptr || off == 0, "a target shard (offset > 0) needs dmin and claim");
  hipStream_t st = S(stream);
  s->keys_clean = false;
  s->points_moved = true;
  // keys kept inside (source shard): the fused tail hands them back as kKeyNone like m3d_icp_step
  const bool reset = claim == nullptr && s->src->n > 0 && s->params.nn_method != M3D_NN_GRID;
  if (fused_tail(s, reset)) {  // terms + fixed-order reduce in one launch (same bits as the two kernels)
    KTimer kt(ctx, M3D_KERNEL_TERMS, st);
    HIPX(ctx, launch_icp_terms_reduce(s, off, claim, dmin, sums, reset, st));
    s->keys_clean = reset;
    return M3D_OK;
  }
  { KTimer kt(ctx, M3D_KERNEL_TERMS, st); HIPX(ctx, launch_icp_terms_mode(s, off, claim, dmin, st)); }
  HIPX(ctx, launch_icp_reduce(s, sums, st));
  return M3D_OK;
}

int m3d_icp_solve(m3d_icp* s, const double* sums, void* stream) {
  if (!s) return M3D_ERR_INVALID;
  Touch tch{s->ctx, S(stream)};  // writes IcpState (the loop's block)
  HIPX(s->ctx, launch_icp_solve(s, sums ? sums : s->sums, S(stream)));
  return M3D_OK;
}

int m3d_icp_set_source_total(m3d_icp* s, int64_t ns_total) {
  if (!s) return M3D_ERR_INVALID;
  CHECK_ARG(s->ctx, ns_total >= 0 && (ns_total == 0 || ns_total >= s->src->n),
            "source total must be 0 or at least the shard's source count");
  s->ns_total = ns_total;
  s->graph_n[0] = s->graph_n[1] = -1;  // the captured solve carries the fitness denominator
  return M3D_OK;
}

int m3d_icp_result_get(m3d_icp* s, m3d_icp_result* out, void* stream) {
  if (!s || !out) return M3D_ERR_INVALID;
  Touch tch{s->ctx, S(stream)};
  return read_result(s->ctx, "m3d_icp_result_get", s->state, s->hcnt, out, S(stream));
}

int m3d_corr_pairs(m3d_ctx* ctx, const int32_t* corr_idx, int64_t n, int32_t* pairs_out, int64_t* count,
                   void* stream) {
  if (!ctx) return M3D_ERR_INVALID;
  CHECK_ARG(ctx, count != nullptr && n >= 0 && n < (int64_t)1 << 31, "invalid arguments");
  CHECK_ARG(ctx, n == 0 || (corr_idx != nullptr && pairs_out != nullptr), "null array");
  *count = 0;
  if (n == 0) return M3D_OK;
  hipSetDevice(ctx->device);
  hipStream_t st = S(stream);
  const int64_t nb = (n + 1023) / 1024;
  const size_t o_p = tmp_align(sizeof(int32_t) * (size_t)(nb + 1));
  if (ctx->tmp.reserve(o_p + sizeof(int32_t) * 2 * (size_t)n) != hipSuccess)
    return m3d_fail(ctx, M3D_ERR_OOM, "correspondence pairs scratch");
  int32_t* cnt = reinterpret_cast<int32_t*>(ctx->tmp.base);
  int32_t* pairs = reinterpret_cast<int32_t*>(ctx->tmp.base + o_p);
  int32_t m = 0;
  hipError_t e = launch_corr_pairs(corr_idx, n, cnt, pairs, st);
  if (e == hipSuccess) e = hipMemcpyAsync(&m, cnt + nb, sizeof(m), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e == hipSuccess && m > 0) {
    e = hipMemcpyAsync(pairs_out, pairs, sizeof(int32_t) * 2 * (size_t)m, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
  }
  if (e != hipSuccess) return m3d_fail(ctx, M3D_ERR_HIP, hipGetErrorString(e));
  *count = m;
  return M3D_OK;
}

const int32_t* m3d_icp_corr(const m3d_icp* s) { return s ? s->corr : nullptr; }

int m3d_icp_copy_corr(const m3d_icp* s, int32_t* dst, void* stream) {
  if (!s || !dst) return M3D_ERR_INVALID;
  Touch tch{s->ctx, S(stream)};
  if (s->src->n == 0) return M3D_OK;
  HIPX(s->ctx, launch_scatter_i32(s->corr, s->src->slot, s->src->n, dst, S(stream)));
  return M3D_OK;
}

int m3d_icp_copy_slots(const m3d_icp* s, int32_t* dst, void* stream) {
  if (!s || !dst) return M3D_ERR_INVALID;
  Touch tch{s->ctx, S(stream)};
  if (s->src->n == 0) return M3D_OK;
  HIPX(s->ctx, hipMemcpyAsync(dst, s->src->slot, sizeof(int32_t) * s->src->n, hipMemcpyDeviceToDevice,
                              S(stream)));
  return M3D_OK;
}

// ------------------------------------------------------------------------------- one-shot loops
// The synchronous entry points that make a loop object, use it once and drop it.
int m3d_icp_run(m3d_ctx* ctx, const m3d_cloud* src, const m3d_cloud* tgt, const double* init,
                double max_dist, const m3d_icp_params* params, m3d_icp_result* out,
                int32_t* corr_idx, void* stream) {
  if (!ctx) return M3D_ERR_INVALID;
  Touch tch{ctx, S(stream)};
  CHECK_ARG(ctx, out != nullptr, "null output");
  ScopedLoop s;
  int rc = icp_create(ctx, src, tgt, max_dist, params, &s.s, true);
  if (rc) return rc;
  rc = m3d_icp_reset(s, init, stream);
  s->graph_off = true;  // a one-shot loop: no HIP graph capture (two equal chunks would trigger one)
  // max_iteration + 1 evaluations
  if (!rc) rc = run_chunked(s, params->max_iteration + 1, [&](int32_t k) { return m3d_icp_steps(s, k, stream); }, S(stream));
  return rc ? rc : finish_run(s, out, corr_idx, S(stream));
}

int m3d_nn1(m3d_ctx* ctx, const m3d_cloud* src, const m3d_cloud* tgt, const double* T_host,
            double max_dist, int32_t nn_method, int32_t* idx, double* d2, void* stream) {
  if (!ctx) return M3D_ERR_INVALID;
  Touch tch{ctx, S(stream)};
  CHECK_ARG(ctx, src && tgt && (idx || src->n == 0), "invalid arguments");
  CHECK_ARG(ctx, max_dist > 0.0, "max_dist must be > 0");
  const m3d_icp_params p = probe_params(M3D_EST_POINT_TO_POINT, nn_method);
  ScopedLoop s;
  const int rc = icp_create(ctx, src, tgt, max_dist, &p, &s.s, true);
  if (rc) return rc;
  hipStream_t st = S(stream);
  // the 1-NN of T·src for any T (no isIdentity() rule); the winners go straight to idx / d2
  return one_evaluation(s, T_host, false, [&](double*) { return launch_nn_finalize(s, idx, d2, st); }, nullptr, 0,
                        nullptr, st);
}

int m3d_evaluate_registration(m3d_ctx* ctx, const m3d_cloud* src, const m3d_cloud* tgt,
                              const double* T_host, double max_dist, int32_t nn_method, int32_t flags,
                              m3d_eval_result* out, int32_t* corr_idx, double* d2, void* stream) {
  if (!ctx) return M3D_ERR_INVALID;
  Touch tch{ctx, S(stream)};
  CHECK_ARG(ctx, src && tgt && out, "invalid arguments");
  CHECK_ARG(ctx, max_dist > 0.0, "max_dist must be > 0");
  CHECK_ARG(ctx, nn_method == M3D_NN_BRUTE || nn_method == M3D_NN_GRID, "unknown nn_method");
  memset(out, 0, sizeof(*out));
  hipStream_t st = S(stream);
  const int64_t ns = src->n, nt = tgt->n;
  if (ns == 0 || nt == 0) return fill_unmatched(ctx, ns, corr_idx, d2, st);
  const m3d_icp_params p = probe_params(M3D_EST_POINT_TO_POINT, nn_method);
  ScopedLoop s;
  int rc = icp_create(ctx, src, tgt, max_dist, &p, &s.s, true);
  if (rc) return rc;
  // (after icp_create: its setup used the same arena and has been synchronised)
  if (ctx->tmp.reserve(eval_scratch_bytes(ns)) != hipSuccess)
    return m3d_fail(ctx, M3D_ERR_OOM, "evaluation scratch");
  double sums[16] = {};
  // EvaluateRegistration: pcd = source; if (!T.isIdentity()) pcd.Transform(T).  The pass writes
  // idx / d² in the caller's order itself: no scatter
  rc = one_evaluation(s, T_host, true, [&](double* pin) {
    return launch_eval(s, (flags & M3D_EVAL_INFORMATION) != 0, corr_idx, d2,
                       reinterpret_cast<double*>(ctx->tmp.base), pin, st);
  }, nullptr, 16, sums, st);
  if (rc) return rc;
  const int64_t matched = (int64_t)sums[0];
  out->num_correspondences = matched;
  out->fitness = (double)matched / (double)ns;
  out->inlier_rmse = matched > 0 ? std::sqrt(sums[1] / (double)matched) : 0.0;
  if ((flags & M3D_EVAL_INFORMATION) != 0) eval_information(sums, out->information);
  return M3D_OK;
}

// ------------------------------------------------------------------------------- test hooks
int m3d_debug_icp_defer_count(m3d_icp* s, uint32_t count, void* stream) {
  if (!s) return M3D_ERR_INVALID;
  CHECK_ARG(s->ctx, s->hcnt != nullptr, "this loop has no deferral list (grid NN with a candidate cap only)");
  Touch tch{s->ctx, S(stream)};
  HIPX(s->ctx, hipMemcpyAsync(s->hcnt, &count, sizeof(count), hipMemcpyHostToDevice, S(stream)));
  HIPX(s->ctx, hipStreamSynchronize(S(stream)));
  return M3D_OK;
}

int m3d_debug_icp_nn_plan(m3d_icp* s, const int32_t* S_, int64_t n, void* stream) {
  if (!s || !S_) return M3D_ERR_INVALID;
  CHECK_ARG(s->ctx, s->nn_qblocks > 0 && nn_plan_on(), "this loop's NN launch takes no plan");
  CHECK_ARG(s->ctx, n == s->nn_qblocks, "one S per query block of 512 sources");
  const int64_t ntiles = s->tgrid->mf_npad / 1024;  // nn_brute.hip: tiles of 1024 targets
  std::vector<uint32_t> Sv((size_t)n), table((size_t)s->nn_budget);
  int64_t sum = 0;
  for (int64_t x = 0; x < n; ++x) {
    CHECK_ARG(s->ctx, S_[x] >= 1 && S_[x] <= ntiles && S_[x] <= 255, "S out of range [1, min(ntiles, 255)]");
    Sv[(size_t)x] = (uint32_t)S_[x];
    sum += S_[x];
  }
  CHECK_ARG(s->ctx, sum <= s->nn_budget, "more slices than resident block slots");
  plan_table_of(Sv.data(), n, s->nn_budget, table.data());
  Touch tch{s->ctx, S(stream)};
  const int32_t forced = 2;
  HIPX(s->ctx, hipMemcpyAsync(s->nn_table, table.data(), sizeof(uint32_t) * table.size(), hipMemcpyHostToDevice, S(stream)));
  HIPX(s->ctx, hipMemcpyAsync(&s->state->plan_ok, &forced, sizeof(forced), hipMemcpyHostToDevice, S(stream)));
  HIPX(s->ctx, hipStreamSynchronize(S(stream)));
  return M3D_OK;
}

int m3d_debug_icp_nn_plan_read(m3d_icp* s, uint32_t* counts, uint32_t* table, int32_t* shape3, void* stream) {
  if (!s || !shape3) return M3D_ERR_INVALID;
  shape3[0] = s->nn_qblocks;
  shape3[1] = s->nn_budget;
  shape3[2] = 0;
  if (s->nn_qblocks <= 0) return M3D_OK;
  Touch tch{s->ctx, S(stream)};
  if (counts)
    HIPX(s->ctx, hipMemcpyAsync(counts, s->nn_seen, sizeof(uint32_t) * (size_t)s->nn_qblocks, hipMemcpyDeviceToHost, S(stream)));
  if (table)
    HIPX(s->ctx, hipMemcpyAsync(table, s->nn_table, sizeof(uint32_t) * (size_t)s->nn_budget, hipMemcpyDeviceToHost, S(stream)));
  HIPX(s->ctx, hipMemcpyAsync(&shape3[2], &s->state->plan_ok, sizeof(int32_t), hipMemcpyDeviceToHost, S(stream)));
  HIPX(s->ctx, hipStreamSynchronize(S(stream)));
  return M3D_OK;
}

int m3d_debug_icp_seed_read(m3d_icp* s, float* seed, int32_t* corr, float* tgt32, int32_t* info2, void* stream) {
  if (!s || !info2) return M3D_ERR_INVALID;
  CHECK_ARG(s->ctx, s->seed != nullptr && s->tgt->rec64 != nullptr,
            "this loop keeps no seed records (brute-force NN on a non-empty target only)");
  info2[0] = s->keys_clean ? 1 : 0;
  Touch tch{s->ctx, S(stream)};
  HIPX(s->ctx, hipMemcpyAsync(&info2[1], &s->state->mfma_ok, sizeof(int32_t), hipMemcpyDeviceToHost, S(stream)));
  const size_t ns = (size_t)s->src->n, nt = (size_t)s->tgt->n;
  if (seed && ns > 0)
    HIPX(s->ctx, hipMemcpyAsync(seed, s->seed, sizeof(float4) * ns, hipMemcpyDeviceToHost, S(stream)));
  if (corr && ns > 0)
    HIPX(s->ctx, hipMemcpyAsync(corr, s->corr, sizeof(int32_t) * ns, hipMemcpyDeviceToHost, S(stream)));
  if (tgt32)
    HIPX(s->ctx, hipMemcpyAsync(tgt32, s->tgt->xyz32, sizeof(float4) * nt, hipMemcpyDeviceToHost, S(stream)));
  HIPX(s->ctx, hipStreamSynchronize(S(stream)));
  return M3D_OK;
}

int m3d_debug_icp_nn_terms(m3d_icp* s, int on) {
  if (!s) return M3D_ERR_INVALID;
  s->nn_terms_off = on == 0;
  // a captured step sequence holds the other iteration's kernels
  for (int k = 0; k < 2; ++k) {
    if (s->graph[k] != nullptr) hipGraphExecDestroy(s->graph[k]);
    s->graph[k] = nullptr;
    s->graph_n[k] = s->seen_n[k] = -1;
  }
  const bool reset = s->params.nn_method != M3D_NN_GRID && s->src->n > 0;
  return nn_terms_selected(nn_terms_sel(s, fused_tail(s, reset), reset)) ? 1 : 0;
}

int m3d_debug_icp_nn_terms_read(m3d_icp* s, uint32_t* tickets, uint32_t* counts, void* stream) {
  if (!s) return M3D_ERR_INVALID;
  if (s->nn_tix == nullptr) return 0;
  Touch tch{s->ctx, S(stream)};
  const size_t bytes = sizeof(uint32_t) * (size_t)s->nn_qblocks;
  if (tickets) HIPX(s->ctx, hipMemcpyAsync(tickets, s->nn_tix, bytes, hipMemcpyDeviceToHost, S(stream)));
  if (counts) HIPX(s->ctx, hipMemcpyAsync(counts, s->nn_cnt, bytes, hipMemcpyDeviceToHost, S(stream)));
  HIPX(s->ctx, hipStreamSynchronize(S(stream)));
  return s->nn_qblocks;
}

int m3d_debug_nn_terms_select(uint32_t bits) {
  NnTermsSel c;
  c.planned = bits & 1u;
  c.fused = bits & 2u;
  c.reset = bits & 4u;
  c.p2plane = bits & 8u;
  c.rec64 = bits & 16u;
  c.seed = bits & 32u;
  c.claim = bits & 64u;
  c.one_device = bits & 128u;
  c.on = bits & 256u;
  return nn_terms_selected(c) ? 1 : 0;
}

}  // extern "C"
