// api_terms.cpp — the entry points of the C ABI (include/m3d.h) whose loop runs a terms pass of its own:
// Generalized ICP, the robust kernels, Colored ICP (with m3d_color_gradients).
#include <cmath>
#include <string>

#include "api_internal.h"

using namespace m3d;
using namespace m3d::api;

// ------------------------------------------------------------------------------- side terms calls
// The entry points whose loop runs a terms pass of its own (terms_pass.h): Generalized ICP, the
// robust kernels, Colored ICP.  Two shapes — one evaluation (side_terms_once) and the whole
// registration (side_terms_run) — around what an estimator adds: a call object with
//   before(ctx, src, tgt, max_dist, st)   work enqueued before the loop object exists
//   setup(loop, st)                       its arrays allocated and filled
//   pass(loop, sums, with_defer, st)      its terms pass and the reduce
namespace {
// The arrays of one side-terms call beside its loop object, one block from the block cache: the
// estimator's own (its call object adds them to the Carve) and the terms pass's block partials
struct TermArrays {
  void* block = nullptr;
  double* partials = nullptr;  // side_terms_blocks(ns) × kTermSlots
  m3d_ctx* ctx = nullptr;
  hipStream_t st = nullptr;
  // back to the block cache, marked after the work this call enqueued on its stream
  ~TermArrays() {
    if (block == nullptr) return;
    ctx_touch(ctx, st);
    ReleaseScope rs(ctx, ctx->id);
    block_release(block);
  }
  int alloc(m3d_ctx* c, hipStream_t s, Carve& cc, int64_t ns, const char* what) {
    ctx = c;
    st = s;
    cc.add(&partials, (size_t)kTermSlots * (size_t)std::max<int64_t>(side_terms_blocks(ns), 1));
    size_t bytes = 0;
    if (cc.alloc(&block, &bytes, st) != hipSuccess)
      return m3d_fail(ctx, M3D_ERR_OOM, std::string("device allocation failed (") + what + ")");
    return M3D_OK;
  }
  int before(m3d_ctx*, const m3d_cloud*, const m3d_cloud*, double, hipStream_t) { return M3D_OK; }
};

// the loop object of a side-terms call: created with p's estimation, then switched to the
// point-to-plane estimator, whose state and solve the pass's sums feed (same slot layout)
int side_loop_create(m3d_ctx* ctx, const m3d_cloud* src, const m3d_cloud* tgt, double max_dist,
                     const m3d_icp_params& p, m3d_icp** out) {
  const int rc = icp_create(ctx, src, tgt, max_dist, &p, out, true);
  if (!rc) (*out)->params.estimation = M3D_EST_POINT_TO_PLANE;
  return rc;
}

// One evaluation at T_host: sums_out[0 .. 30) (non-null: the entry point's check) and the
// correspondences.  pcd = source; if (!T.isIdentity()) pcd.Transform(T) — points and whatever
// the estimator moves with them
template <class Call>
int side_terms_once(m3d_ctx* ctx, const m3d_cloud* src, const m3d_cloud* tgt, const double* T_host, double max_dist,
                    int32_t estimation, int32_t nn_method, Call& call, double* sums_out, int32_t* corr_idx,
                    hipStream_t st) {
  for (int k = 0; k < kTermSlots; ++k) sums_out[k] = 0.0;
  if (src->n == 0 || tgt->n == 0) return fill_unmatched(ctx, src->n, corr_idx, nullptr, st);  // and no sums
  int rc = call.before(ctx, src, tgt, max_dist, st);
  if (rc) return rc;
  ScopedLoop s;
  rc = side_loop_create(ctx, src, tgt, max_dist, probe_params(estimation, nn_method), &s.s);
  if (!rc) rc = call.setup(s, st);
  if (rc) return rc;
  double sums[kTermSlots] = {};
  rc = one_evaluation(s, T_host, true, [&](double* pin) {
    KTimer kt(ctx, M3D_KERNEL_TERMS, st);
    return call.pass(s, pin, true, st);
  }, corr_idx, kTermSlots, sums, st);
  if (rc) return rc;
  for (int k = 0; k < 30; ++k) sums_out[k] = sums[k];
  return M3D_OK;
}

// The evaluations of a one-shot loop whose terms pass is not the fused tail's: max_iteration + 1
// times NN scan, terms(sums) (the pass and its reduce) and the point-to-plane solve, enqueued in
// growing chunks with a look at `done` in between, as m3d_icp_run; evaluations after convergence
// are device no-ops.  Then the result.  The loop has been reset.
template <class Terms>
int run_terms_loop(m3d_icp* s, int32_t max_iteration, Terms terms, m3d_icp_result* out, int32_t* corr_idx,
                   hipStream_t st) {
  m3d_ctx* ctx = s->ctx;
  const bool search = s->src->n > 0 && s->tgt->n > 0;  // else: no scan, zero sums, every source unmatched
  auto step = [&](int32_t k) {
    hipError_t e = hipSuccess;
    if (k > 0) s->points_moved = true;
    for (int32_t it = 0; it < k && e == hipSuccess; ++it) {
      if (search) e = enqueue_nn(s, 0, st);
      if (e == hipSuccess) {
        KTimer kt(ctx, M3D_KERNEL_TERMS, st);
        e = terms(s->sums);
      }
      if (e == hipSuccess) {
        KTimer kt(ctx, M3D_KERNEL_LOOP, st);
        e = launch_icp_solve(s, s->sums, st);
      }
    }
    return e == hipSuccess ? M3D_OK : m3d_fail(ctx, M3D_ERR_HIP, std::string("terms loop step: ") + hipGetErrorString(e));
  };
  int rc = run_chunked(s, max_iteration + 1, step, st);
  if (!rc) rc = finish_run(s, out, corr_idx, st);
  return rc;
}

// The whole registration from init: p = the loop's parameters (its estimation: side_loop_create)
template <class Call>
int side_terms_run(m3d_ctx* ctx, const m3d_cloud* src, const m3d_cloud* tgt, const double* init, double max_dist,
                   const m3d_icp_params& p, Call& call, m3d_icp_result* out, int32_t* corr_idx, void* stream) {
  hipStream_t st = S(stream);
  int rc = call.before(ctx, src, tgt, max_dist, st);
  if (rc) return rc;
  ScopedLoop s;
  rc = side_loop_create(ctx, src, tgt, max_dist, p, &s.s);
  if (!rc) rc = call.setup(s, st);
  if (!rc) rc = m3d_icp_reset(s, init, stream);
  if (!rc)
    rc = run_terms_loop(s, p.max_iteration, [&](double* sums) { return call.pass(s, sums, false, st); }, out,
                        corr_idx, st);
  if (rc) (void)hipStreamSynchronize(st);  // the arrays go back to the block cache idle
  return rc;
}

// a kernel that changes nothing (null or L2): the call is the one without a kernel
const m3d_robust_kernel* non_l2(const m3d_robust_kernel* kernel) {
  return kernel != nullptr && kernel->kind != M3D_KERNEL_L2 ? kernel : nullptr;
}

// ------------------------------------------------------------------------------- Generalized ICP
// gicp.hip.  The loop object is created as a point-to-point loop: no demand on the target's
// normals — the covariances may be the caller's.
int gicp_check(m3d_ctx* ctx, const m3d_cloud* src, const m3d_cloud* tgt, const double* src_cov,
               const double* tgt_cov, double max_dist, int32_t nn_method, double epsilon) {
  CHECK_ARG(ctx, src && tgt, "invalid arguments");
  CHECK_ARG(ctx, max_dist > 0.0, "Invalid max_correspondence_distance.");
  CHECK_ARG(ctx, nn_method == M3D_NN_BRUTE || nn_method == M3D_NN_GRID, "unknown nn_method");
  CHECK_ARG(ctx, epsilon > 0.0, "epsilon must be > 0");
  CHECK_ARG(ctx, src_cov != nullptr || src->nrm64 != nullptr || src->n == 0,
            "Generalized ICP: the source has neither covariances nor normals");
  CHECK_ARG(ctx, tgt_cov != nullptr || tgt->nrm64 != nullptr || tgt->n == 0,
            "Generalized ICP: the target has neither covariances nor normals");
  return M3D_OK;
}

// The covariance arrays of one Generalized-ICP call, 6 doubles per point: the source's in the
// loop's Morton slot order (rotated in place by every evaluation), the target's in target index
// order.  kernel null: the plane-to-plane terms of gicp.hip, else robust.hip's with that (checked)
// kernel
struct GicpCall : TermArrays {
  const double *src_cov, *tgt_cov;
  double epsilon;
  const m3d_robust_kernel* kernel;
  double* cov_s = nullptr;
  double* cov_t = nullptr;
  GicpCall(const double* sc, const double* tc, double eps, const m3d_robust_kernel* k)
      : src_cov(sc), tgt_cov(tc), epsilon(eps), kernel(k) {}
  // allocate the arrays and initialise the covariances: the caller's (its order → slot order for
  // the source), else from the normals — the Morton copy's are in slot order already
  int setup(m3d_icp* s, hipStream_t st) {
    const int64_t ns = s->src->n, nt = s->tgt->n;
    Carve cc;
    cc.add(&cov_s, 6 * (size_t)ns);
    cc.add(&cov_t, 6 * (size_t)nt);
    const int rc = alloc(s->ctx, st, cc, ns, "Generalized ICP covariances");
    if (rc) return rc;
    HIPX(ctx, src_cov != nullptr ? launch_cov_pack(src_cov, s->src->slot, ns, cov_s, st)
                                 : launch_cov_from_normals(s->src->nrm64, ns, epsilon, cov_s, 6, st));
    HIPX(ctx, tgt_cov != nullptr ? launch_cov_pack(tgt_cov, nullptr, nt, cov_t, st)
                                 : launch_cov_from_normals(s->tgt->nrm64, nt, epsilon, cov_t, 6, st));
    return M3D_OK;
  }
  hipError_t pass(const m3d_icp* s, double* sums, bool with_defer, hipStream_t st) const {
    return kernel == nullptr
               ? launch_gicp_terms(s, cov_s, cov_t, partials, sums, with_defer, st)
               : launch_robust_terms(s, kernel->kind, kernel->k, cov_s, cov_t, partials, sums, with_defer, st);
  }
};

int gicp_terms(m3d_ctx* ctx, const m3d_cloud* src, const m3d_cloud* tgt, const double* src_cov,
               const double* tgt_cov, const double* T_host, double max_dist, int32_t nn_method, double epsilon,
               const m3d_robust_kernel* kernel, double* sums_out, int32_t* corr_idx, hipStream_t st) {
  CHECK_ARG(ctx, sums_out != nullptr, "null output");
  const int rc = gicp_check(ctx, src, tgt, src_cov, tgt_cov, max_dist, nn_method, epsilon);
  if (rc) return rc;
  GicpCall call(src_cov, tgt_cov, epsilon, kernel);
  return side_terms_once(ctx, src, tgt, T_host, max_dist, M3D_EST_POINT_TO_POINT, nn_method, call, sums_out,
                         corr_idx, st);
}

int gicp_run(m3d_ctx* ctx, const m3d_cloud* src, const m3d_cloud* tgt, const double* src_cov,
             const double* tgt_cov, const double* init, double max_dist, const m3d_gicp_params* params,
             const m3d_robust_kernel* kernel, m3d_icp_result* out, int32_t* corr_idx, void* stream) {
  CHECK_ARG(ctx, out != nullptr && params != nullptr, "null output or parameters");
  const int rc = gicp_check(ctx, src, tgt, src_cov, tgt_cov, max_dist, params->nn_method, params->epsilon);
  if (rc) return rc;
  GicpCall call(src_cov, tgt_cov, params->epsilon, kernel);
  const m3d_icp_params p{params->relative_fitness, params->relative_rmse, params->max_iteration,
                         M3D_EST_POINT_TO_POINT,   params->nn_method,     0};
  return side_terms_run(ctx, src, tgt, init, max_dist, p, call, out, corr_idx, stream);
}

// robust point-to-plane (robust.hip): the block partials are all it needs
struct RobustPlaneCall : TermArrays {
  const m3d_robust_kernel* kernel;
  explicit RobustPlaneCall(const m3d_robust_kernel* k) : kernel(k) {}
  int setup(m3d_icp* s, hipStream_t st) {
    Carve cc;
    return alloc(s->ctx, st, cc, s->src->n, "robust point-to-plane partials");
  }
  hipError_t pass(const m3d_icp* s, double* sums, bool with_defer, hipStream_t st) const {
    return launch_robust_terms(s, kernel->kind, kernel->k, nullptr, nullptr, partials, sums, with_defer, st);
  }
};

// ------------------------------------------------------------------------------- Colored ICP
// colored.hip.  The loop object is the point-to-plane loop's (state, NN scan, solve); the target's
// gradient records, the source's intensities in slot order and the terms pass's partials live in
// one block of their own beside it, as Generalized ICP's covariances do.
constexpr int kColoredMaxNn = 30;  // KDTreeSearchParamHybrid(2·max_dist, 30)

// the gradients of cloud c with the given normals and colours: rec (n × 4) and / or out3 (n × 3)
int color_gradients(m3d_ctx* ctx, const m3d_cloud* c, const double* colors, double radius, int k, double* rec,
                    double* out3, hipStream_t st) {
  if (c->n == 0) return M3D_OK;
  const Grid *g = nullptr, *gf = nullptr;
  double hf = 0.0;
  const int rc = search_grids(ctx, c, radius, k, st, &g, &gf, &hf);
  if (rc) return rc;
  HIPX(ctx, launch_color_gradients(c, c->nrm64, colors, g, radius, k, rec, out3, st, gf, hf));
  return M3D_OK;
}

int colored_check(m3d_ctx* ctx, const m3d_cloud* src, const m3d_cloud* tgt, const double* src_colors,
                  const double* tgt_colors, double max_dist, int32_t nn_method, double lambda,
                  const m3d_robust_kernel* kernel) {
  CHECK_ARG(ctx, src && tgt, "invalid arguments");
  CHECK_ARG(ctx, max_dist > 0.0, "Invalid max_correspondence_distance.");
  CHECK_ARG(ctx, nn_method == M3D_NN_BRUTE || nn_method == M3D_NN_GRID, "unknown nn_method");
  CHECK_ARG(ctx, lambda >= 0.0 && lambda <= 1.0, "lambda_geometric must lie in [0, 1]");
  CHECK_ARG(ctx, tgt->nrm64 != nullptr || tgt->n == 0,
            "ColoredICP requires pre-computed normal vectors for target PointCloud.");
  CHECK_ARG(ctx, (src_colors != nullptr || src->n == 0) && (tgt_colors != nullptr || tgt->n == 0),
            "ColoredICP requires pre-computed colors for source and target PointCloud.");
  return kernel != nullptr ? robust_check(ctx, kernel) : M3D_OK;
}

// The arrays of one Colored-ICP call: the target's records (from the caller's gradients, else
// computed) are allocated and filled before the loop object exists, the source's intensities
// gathered into the loop's slot order once it does.  kernel null: L2 through the same pass
struct ColoredCall : TermArrays {
  const double *src_colors, *tgt_colors, *tgt_gradient;
  double lambda;
  const m3d_robust_kernel* kernel;
  double* rec_t = nullptr;  // nt × 4: gradient, intensity
  double* is_s = nullptr;   // ns, slot order
  ColoredCall(const double* sc, const double* tc, const double* tg, double l, const m3d_robust_kernel* k)
      : src_colors(sc), tgt_colors(tc), tgt_gradient(tg), lambda(l), kernel(k) {}
  int before(m3d_ctx* c, const m3d_cloud* src, const m3d_cloud* tgt, double max_dist, hipStream_t st) {
    hipSetDevice(c->device);
    Carve cc;
    cc.add(&rec_t, 4 * (size_t)tgt->n);
    cc.add(&is_s, (size_t)src->n);
    const int rc = alloc(c, st, cc, src->n, "Colored ICP arrays");
    if (rc) return rc;
    if (tgt_gradient != nullptr) {
      HIPX(ctx, launch_color_rec_pack(tgt_gradient, tgt_colors, tgt->n, rec_t, st));
      return M3D_OK;
    }
    return color_gradients(ctx, tgt, tgt_colors, 2.0 * max_dist, kColoredMaxNn, rec_t, nullptr, st);
  }
  int setup(m3d_icp* s, hipStream_t st) {
    HIPX(ctx, launch_intensity_pack(src_colors, s->src->slot, s->src->n, is_s, st));
    return M3D_OK;
  }
  hipError_t pass(const m3d_icp* s, double* sums, bool with_defer, hipStream_t st) const {
    return launch_colored_terms(s, rec_t, is_s, lambda, kernel != nullptr ? kernel->kind : M3D_KERNEL_L2,
                                kernel != nullptr ? kernel->k : 0.0, partials, sums, with_defer, st);
  }
};
}  // namespace

namespace m3d {
namespace api {
// a caller's robust kernel: a known kind, and a finite k > 0 for the kinds that read it
int robust_check(m3d_ctx* ctx, const m3d_robust_kernel* kernel) {
  CHECK_ARG(ctx, kernel != nullptr, "null robust kernel");
  CHECK_ARG(ctx, kernel->kind >= M3D_KERNEL_L2 && kernel->kind <= M3D_KERNEL_TUKEY, "unknown robust kernel");
  CHECK_ARG(ctx, kernel->kind == M3D_KERNEL_L2 || kernel->kind == M3D_KERNEL_L1 ||
                     (std::isfinite(kernel->k) && kernel->k > 0.0),
            "robust kernel: k must be finite and > 0");
  return M3D_OK;
}
}  // namespace api
}  // namespace m3d

extern "C" {

int m3d_covariances_from_normals(m3d_ctx* ctx, const double* normals, int64_t n, double epsilon,
                                 double* cov_out, void* stream) {
  if (!ctx) return M3D_ERR_INVALID;
  CHECK_ARG(ctx, n >= 0 && (n == 0 || (normals && cov_out)), "invalid arguments");
  CHECK_ARG(ctx, epsilon > 0.0, "epsilon must be > 0");
  hipSetDevice(ctx->device);
  HIPX(ctx, launch_cov_from_normals(normals, n, epsilon, cov_out, 9, S(stream)));
  return M3D_OK;
}

int m3d_gicp_terms(m3d_ctx* ctx, const m3d_cloud* src, const m3d_cloud* tgt, const double* src_cov,
                   const double* tgt_cov, const double* T_host, double max_dist, int32_t nn_method,
                   double epsilon, double* sums_out, int32_t* corr_idx, void* stream) {
  if (!ctx) return M3D_ERR_INVALID;
  Touch tch{ctx, S(stream)};
  return gicp_terms(ctx, src, tgt, src_cov, tgt_cov, T_host, max_dist, nn_method, epsilon, nullptr, sums_out,
                    corr_idx, S(stream));
}

int m3d_gicp_run(m3d_ctx* ctx, const m3d_cloud* src, const m3d_cloud* tgt, const double* src_cov,
                 const double* tgt_cov, const double* init, double max_dist, const m3d_gicp_params* params,
                 m3d_icp_result* out, int32_t* corr_idx, void* stream) {
  if (!ctx) return M3D_ERR_INVALID;
  Touch tch{ctx, S(stream)};
  return gicp_run(ctx, src, tgt, src_cov, tgt_cov, init, max_dist, params, nullptr, out, corr_idx, stream);
}

// ------------------------------------------------------------------------------- robust kernels
// robust.hip.  Generalized ICP with a kernel is the calls above with another terms pass;
// point-to-plane with a kernel is the same loop shape around the point-to-plane loop object.
int m3d_gicp_terms_robust(m3d_ctx* ctx, const m3d_cloud* src, const m3d_cloud* tgt, const double* src_cov,
                          const double* tgt_cov, const double* T_host, double max_dist, int32_t nn_method,
                          double epsilon, const m3d_robust_kernel* kernel, double* sums_out, int32_t* corr_idx,
                          void* stream) {
  if (!ctx) return M3D_ERR_INVALID;
  Touch tch{ctx, S(stream)};
  if (kernel != nullptr) {
    const int rc = robust_check(ctx, kernel);
    if (rc) return rc;
  }
  return gicp_terms(ctx, src, tgt, src_cov, tgt_cov, T_host, max_dist, nn_method, epsilon, non_l2(kernel), sums_out,
                    corr_idx, S(stream));
}

int m3d_gicp_run_robust(m3d_ctx* ctx, const m3d_cloud* src, const m3d_cloud* tgt, const double* src_cov,
                        const double* tgt_cov, const double* init, double max_dist,
                        const m3d_gicp_params* params, const m3d_robust_kernel* kernel, m3d_icp_result* out,
                        int32_t* corr_idx, void* stream) {
  if (!ctx) return M3D_ERR_INVALID;
  Touch tch{ctx, S(stream)};
  if (kernel != nullptr) {
    const int rc = robust_check(ctx, kernel);
    if (rc) return rc;
  }
  return gicp_run(ctx, src, tgt, src_cov, tgt_cov, init, max_dist, params, non_l2(kernel), out, corr_idx, stream);
}

int m3d_robust_terms(m3d_ctx* ctx, const m3d_cloud* src, const m3d_cloud* tgt, const double* T_host,
                     double max_dist, int32_t nn_method, const m3d_robust_kernel* kernel, double* sums_out,
                     int32_t* corr_idx, void* stream) {
  if (!ctx) return M3D_ERR_INVALID;
  Touch tch{ctx, S(stream)};
  CHECK_ARG(ctx, src && tgt && sums_out, "invalid arguments");
  int rc = robust_check(ctx, kernel);
  if (rc) return rc;
  CHECK_ARG(ctx, max_dist > 0.0, "Invalid max_correspondence_distance.");
  CHECK_ARG(ctx, nn_method == M3D_NN_BRUTE || nn_method == M3D_NN_GRID, "unknown nn_method");
  CHECK_ARG(ctx, tgt->nrm64 != nullptr || tgt->n == 0,
            "TransformationEstimationPointToPlane requires pre-computed normal vectors for target "
            "PointCloud.");
  RobustPlaneCall call(kernel);
  return side_terms_once(ctx, src, tgt, T_host, max_dist, M3D_EST_POINT_TO_PLANE, nn_method, call, sums_out,
                         corr_idx, S(stream));
}

int m3d_robust_icp_run(m3d_ctx* ctx, const m3d_cloud* src, const m3d_cloud* tgt, const double* init,
                       double max_dist, const m3d_icp_params* params, const m3d_robust_kernel* kernel,
                       m3d_icp_result* out, int32_t* corr_idx, void* stream) {
  if (!ctx) return M3D_ERR_INVALID;
  Touch tch{ctx, S(stream)};
  CHECK_ARG(ctx, out != nullptr && params != nullptr, "null output or parameters");
  int rc = robust_check(ctx, kernel);
  if (rc) return rc;
  CHECK_ARG(ctx, params->estimation == M3D_EST_POINT_TO_PLANE,
            "a robust kernel needs the point-to-plane estimation (TransformationEstimationPointToPoint takes none)");
  RobustPlaneCall call(kernel);
  return side_terms_run(ctx, src, tgt, init, max_dist, *params, call, out, corr_idx, stream);
}

int m3d_color_gradients(m3d_ctx* ctx, const m3d_cloud* cloud, const double* colors, double radius,
                        int32_t max_nn, double* out, void* stream) {
  if (!ctx) return M3D_ERR_INVALID;
  CHECK_ARG(ctx, cloud != nullptr, "invalid arguments");
  CHECK_ARG(ctx, radius > 0.0 && max_nn >= 1 && max_nn <= 64, "radius > 0 and 1 <= max_nn <= 64");
  CHECK_ARG(ctx, cloud->nrm64 != nullptr || cloud->n == 0, "color gradients: the cloud has no normals");
  CHECK_ARG(ctx, (colors != nullptr && out != nullptr) || cloud->n == 0, "color gradients: null colors or output");
  hipSetDevice(ctx->device);
  hipStream_t st = S(stream);
  Touch tch{ctx, st};
  const int rc = color_gradients(ctx, cloud, colors, radius, max_nn, nullptr, out, st);
  if (rc) return rc;
  HIPX(ctx, hipStreamSynchronize(st));
  return M3D_OK;
}

int m3d_colored_terms(m3d_ctx* ctx, const m3d_cloud* src, const m3d_cloud* tgt, const double* src_colors,
                      const double* tgt_colors, const double* tgt_gradient, const double* T_host,
                      double max_dist, int32_t nn_method, double lambda_geometric,
                      const m3d_robust_kernel* kernel, double* sums_out, int32_t* corr_idx, void* stream) {
  if (!ctx) return M3D_ERR_INVALID;
  hipStream_t st = S(stream);
  Touch tch{ctx, st};
  CHECK_ARG(ctx, sums_out != nullptr, "null output");
  int rc = colored_check(ctx, src, tgt, src_colors, tgt_colors, max_dist, nn_method, lambda_geometric, kernel);
  if (rc) return rc;
  ColoredCall call(src_colors, tgt_colors, tgt_gradient, lambda_geometric, kernel);
  return side_terms_once(ctx, src, tgt, T_host, max_dist, M3D_EST_POINT_TO_PLANE, nn_method, call, sums_out,
                         corr_idx, st);
}

int m3d_colored_icp_run(m3d_ctx* ctx, const m3d_cloud* src, const m3d_cloud* tgt, const double* src_colors,
                        const double* tgt_colors, const double* tgt_gradient, const double* init,
                        double max_dist, const m3d_colored_params* params, const m3d_robust_kernel* kernel,
                        m3d_icp_result* out, int32_t* corr_idx, void* stream) {
  if (!ctx) return M3D_ERR_INVALID;
  hipStream_t st = S(stream);
  Touch tch{ctx, st};
  CHECK_ARG(ctx, out != nullptr && params != nullptr, "null output or parameters");
  int rc = colored_check(ctx, src, tgt, src_colors, tgt_colors, max_dist, params->nn_method,
                         params->lambda_geometric, kernel);
  if (rc) return rc;
  CHECK_ARG(ctx, params->max_iteration >= 0, "max_iteration must be >= 0");
  ColoredCall call(src_colors, tgt_colors, tgt_gradient, params->lambda_geometric, kernel);
  const m3d_icp_params p{params->relative_fitness, params->relative_rmse, params->max_iteration,
                         M3D_EST_POINT_TO_PLANE,   params->nn_method,     0};
  return side_terms_run(ctx, src, tgt, init, max_dist, p, call, out, corr_idx, stream);
}

}  // extern "C"
