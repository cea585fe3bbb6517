// api_prep.cpp — preprocessing calls of the C ABI (include/m3d.h): voxel down-sampling, hybrid and k-NN search,
// normals, FPFH, the outlier filters, plane segmentation, DBSCAN, ISS keypoints, minimum-distance
// thinning and Fast Global Registration.  Which scratch each call draws from: api_internal.h.
#include <string.h>

#include <algorithm>
#include <cmath>
#include <string>

#include "api_internal.h"

using namespace m3d;
using namespace m3d::api;

namespace {
// Neighbour lists of the synchronous preprocessing calls (estimate_normals, compute_fpfh), carved
// from the context's preprocessing buffer (api_internal.h, source 4)
struct NbrLists {
  int32_t* idx = nullptr;
  double* d2 = nullptr;
  int32_t* cnt = nullptr;
  double* extra = nullptr;  // caller's n × extra_per_point doubles (FPFH: the SPFH rows)
  char* scratch = nullptr;  // caller's scratch_bytes behind the lists (k-NN normals: the ladder's)
};

int prep_lists(m3d_ctx* ctx, int64_t n, int k, int64_t extra_per_point, NbrLists* L, size_t scratch_bytes = 0) {
  Carve cv;
  cv.add(&L->idx, (size_t)n * k);
  cv.add(&L->d2, (size_t)n * k);
  cv.add(&L->cnt, (size_t)n);
  if (extra_per_point > 0) cv.add(&L->extra, (size_t)(n * extra_per_point));
  if (scratch_bytes > 0) cv.add(&L->scratch, scratch_bytes);
  char* b = nullptr;
  const int rc = prep_buffer(ctx, cv.bytes(), &b);
  if (!rc) cv.place(b);
  return rc;
}

// hybrid neighbourhoods of every point of `c` (grid cell = radius)
int neighbourhoods(m3d_ctx* ctx, const m3d_cloud* c, double radius, int k, hipStream_t st,
                   int64_t extra_per_point, NbrLists* L) {
  const Grid *g = nullptr, *gf = nullptr;
  double hf = 0.0;
  int rc = search_grids(ctx, c, radius, k, st, &g, &gf, &hf);
  if (rc) return rc;
  rc = prep_lists(ctx, std::max<int64_t>(c->n, 1), k, extra_per_point, L);
  if (rc) return rc;
  HIPX(ctx, hybrid_search(c, g, radius, k, L->idx, L->d2, L->cnt, st, gf, hf));
  return M3D_OK;
}

int fgr_check(m3d_ctx* ctx, const m3d_cloud* src, const m3d_cloud* tgt, int64_t nc, const m3d_fgr_params* p) {
  CHECK_ARG(ctx, src && tgt && p, "invalid arguments");
  CHECK_ARG(ctx, nc >= 0 && nc < ((int64_t)1 << 31) / 300, "fgr: 0 <= rows < 2^31 / 300");
  CHECK_ARG(ctx, p->tuple_scale > 0.0 && p->tuple_scale <= 1.0, "fgr: tuple_scale must be in (0, 1]");
  CHECK_ARG(ctx, p->division_factor > 0.0, "fgr: division_factor must be > 0");
  CHECK_ARG(ctx, p->iteration_number >= 0 && p->maximum_tuple_count >= 0,
            "fgr: iteration_number and maximum_tuple_count must be >= 0");
  CHECK_ARG(ctx, p->path >= 0 && p->path <= 2, "fgr: path is 0, 1 or 2");
  return M3D_OK;
}

// steps 2-3 into a scratch block of the call's own
int fgr_rows_call(m3d_ctx* ctx, const m3d_cloud* src, const m3d_cloud* tgt, const int32_t* corr, int64_t nc,
                  const m3d_fgr_params* p, m3d_fgr_result* out, int32_t* rows_out, DevTmp<char>* scratch,
                  hipStream_t st) {
  CHECK_ARG(ctx, nc == 0 || corr != nullptr, "null correspondence pointer");
  int rc = dev_alloc(ctx, &scratch->p, (int64_t)fgr_scratch_bytes(src->n, tgt->n, nc, fgr_tuple_cap(p, nc)));
  if (rc) return rc;
  int bad = 0;
  HIPX(ctx, fgr_rows(ctx, src->xyz64, src->n, tgt->xyz64, tgt->n, corr, nc, p, out, rows_out, scratch->p, st, &bad));
  if (bad) return m3d_fail(ctx, M3D_ERR_INVALID, "fgr: a correspondence index is outside its cloud");
  return M3D_OK;
}
}  // namespace

namespace m3d {
namespace api {
// the grids of a hybrid search: cell = radius, plus the finer first-stage grid when the cloud is
// dense enough (prep.hip hybrid_fine_radius; both cached on the cloud)
int search_grids(m3d_ctx* ctx, const m3d_cloud* c, double radius, int k, hipStream_t st,
                 const Grid** g, const Grid** gf, double* hf) {
  int rc = ensure_grid(ctx, c, radius, st, g);
  if (rc) return rc;
  hipError_t e = grid_occupancy(const_cast<Grid*>(*g), &ctx->tmp, st);  // hybrid_fine_radius reads it
  if (e != hipSuccess) return m3d_fail(ctx, M3D_ERR_HIP, std::string("grid occupancy: ") + hipGetErrorString(e));
  *gf = nullptr;
  *hf = hybrid_fine_radius(*g, radius, k);
  if (*hf > 0.0) rc = ensure_grid(ctx, c, *hf, st, gf);
  return rc;
}
}  // namespace api
}  // namespace m3d

extern "C" {

// ------------------------------------------------------------------------------- preprocessing
int m3d_voxel_down_sample(m3d_ctx* ctx, const double* xyz, const double* normals, int64_t n,
                          double voxel_size, double* out_xyz, double* out_normals, int64_t* out_n,
                          void* stream) {
  if (!ctx) return M3D_ERR_INVALID;
  CHECK_ARG(ctx, out_n != nullptr && n >= 0 && n < ((int64_t)1 << 31), "invalid arguments");
  CHECK_ARG(ctx, voxel_size > 0.0, "voxel_size <= 0.");
  CHECK_ARG(ctx, n == 0 || (xyz && out_xyz), "null device pointer");
  hipSetDevice(ctx->device);
  std::string why;
  // scratch from the context's preprocessing buffer: the call synchronises before returning
  char* scratch = nullptr;
  int rc = n > 0 ? prep_buffer(ctx, voxel_scratch_bytes(n), &scratch) : M3D_OK;
  if (rc) return rc;
  hipError_t e = voxel_down_sample(xyz, normals, n, voxel_size, out_xyz, normals ? out_normals : nullptr,
                                   out_n, scratch, S(stream), &why);
  if (e != hipSuccess)
    return m3d_fail(ctx, why.empty() ? M3D_ERR_HIP : M3D_ERR_INVALID,
                    why.empty() ? std::string("voxel_down_sample: ") + hipGetErrorString(e) : why);
  return M3D_OK;
}

int m3d_hybrid_search(m3d_ctx* ctx, const m3d_cloud* cloud, double radius, int32_t max_nn,
                      int32_t* idx, double* d2, int32_t* count, void* stream) {
  if (!ctx) return M3D_ERR_INVALID;
  CHECK_ARG(ctx, cloud && idx && d2 && count, "invalid arguments");
  CHECK_ARG(ctx, radius > 0.0 && max_nn >= 1 && max_nn <= 256, "radius > 0 and 1 <= max_nn <= 256");
  hipSetDevice(ctx->device);
  hipStream_t st = S(stream);
  Touch tch{ctx, st};
  const Grid *g = nullptr, *gf = nullptr;
  double hf = 0.0;
  int rc = search_grids(ctx, cloud, radius, max_nn, st, &g, &gf, &hf);
  if (rc) return rc;
  HIPX(ctx, hybrid_search(cloud, g, radius, max_nn, idx, d2, count, st, gf, hf));
  HIPX(ctx, hipStreamSynchronize(st));
  return M3D_OK;
}

int m3d_estimate_normals(m3d_ctx* ctx, const m3d_cloud* cloud, double radius, int32_t max_nn,
                         double* normals_out, void* stream) {
  if (!ctx) return M3D_ERR_INVALID;
  CHECK_ARG(ctx, cloud && (normals_out || cloud->n == 0), "invalid arguments");
  CHECK_ARG(ctx, radius > 0.0 && max_nn >= 1 && max_nn <= 256, "radius > 0 and 1 <= max_nn <= 256");
  hipSetDevice(ctx->device);
  hipStream_t st = S(stream);
  Touch tch{ctx, st};
  NbrLists L;
  int rc = neighbourhoods(ctx, cloud, radius, max_nn, st, 0, &L);
  if (rc) return rc;
  HIPX(ctx, launch_normals(cloud, L.idx, max_nn, L.cnt, cloud->nrm64, normals_out, st));
  HIPX(ctx, hipStreamSynchronize(st));
  return M3D_OK;
}

int m3d_compute_fpfh(m3d_ctx* ctx, const m3d_cloud* cloud, const double* normals, double radius,
                     int32_t max_nn, double* fpfh_out, void* stream) {
  if (!ctx) return M3D_ERR_INVALID;
  CHECK_ARG(ctx, cloud && ((normals && fpfh_out) || cloud->n == 0),
            "Failed because input point cloud has no normal.");
  CHECK_ARG(ctx, radius > 0.0 && max_nn >= 1 && max_nn <= 256, "radius > 0 and 1 <= max_nn <= 256");
  hipSetDevice(ctx->device);
  hipStream_t st = S(stream);
  Touch tch{ctx, st};
  NbrLists L;
  int rc = neighbourhoods(ctx, cloud, radius, max_nn, st, 33, &L);
  if (rc) return rc;
  HIPX(ctx, launch_fpfh(cloud, normals, L.idx, L.d2, max_nn, L.cnt, L.extra, fpfh_out, st));
  HIPX(ctx, hipStreamSynchronize(st));
  return M3D_OK;
}

// ------------------------------------------------------------------------------- outlier removal
// clean.hip; scratch from the context's preprocessing buffer, the ladder's grids from the block cache:
// no hipMalloc per call on the steady path
int m3d_knn_search(m3d_ctx* ctx, const m3d_cloud* cloud, int32_t k, int32_t* idx, double* d2,
                   int32_t* count, void* stream) {
  if (!ctx) return M3D_ERR_INVALID;
  CHECK_ARG(ctx, cloud && idx && d2 && count, "invalid arguments");
  CHECK_ARG(ctx, k >= 1 && k <= 256, "1 <= k <= 256");
  if (cloud->n == 0) return M3D_OK;
  hipSetDevice(ctx->device);
  hipStream_t st = S(stream);
  Touch tch{ctx, st};
  char* scratch = nullptr;
  int rc = prep_buffer(ctx, clean_scratch_bytes(cloud->n), &scratch);
  if (rc) return rc;
  std::string why;
  hipError_t e = knn_search(ctx, cloud, k, idx, d2, count, scratch, st, &why);
  if (e != hipSuccess) return hip_fail(ctx, "knn_search", e, why);
  return M3D_OK;
}

int m3d_estimate_normals_knn(m3d_ctx* ctx, const m3d_cloud* cloud, int32_t k, double* normals_out,
                             void* stream) {
  if (!ctx) return M3D_ERR_INVALID;
  CHECK_ARG(ctx, cloud && (normals_out || cloud->n == 0), "invalid arguments");
  CHECK_ARG(ctx, k >= 1 && k <= 256, "1 <= k <= 256");
  const int64_t n = cloud->n;
  if (n == 0) return M3D_OK;
  hipSetDevice(ctx->device);
  hipStream_t st = S(stream);
  Touch tch{ctx, st};
  // the k-NN lists and the ladder's scratch side by side in the context's preprocessing buffer
  NbrLists L;
  int rc = prep_lists(ctx, n, k, 0, &L, clean_scratch_bytes(n));
  if (rc) return rc;
  std::string why;
  hipError_t e = knn_search(ctx, cloud, k, L.idx, L.d2, L.cnt, L.scratch, st, &why);
  if (e != hipSuccess) return hip_fail(ctx, "knn_search", e, why);
  HIPX(ctx, launch_normals(cloud, L.idx, k, L.cnt, cloud->nrm64, normals_out, st));
  HIPX(ctx, hipStreamSynchronize(st));
  return M3D_OK;
}

int m3d_remove_statistical_outlier(m3d_ctx* ctx, const m3d_cloud* cloud, int32_t nb_neighbors,
                                   double std_ratio, int32_t* index_out, int64_t* n_out,
                                   m3d_outlier_stats* stats, double* avg_out, void* stream) {
  if (!ctx) return M3D_ERR_INVALID;
  CHECK_ARG(ctx, cloud && n_out && (index_out || cloud->n == 0), "invalid arguments");
  CHECK_ARG(ctx, nb_neighbors >= 1 && std_ratio > 0.0, "Illegal input parameters, the number of neighbors and "
                                                       "standard deviation ratio must be positive.");
  CHECK_ARG(ctx, nb_neighbors <= 256, "1 <= nb_neighbors <= 256");
  *n_out = 0;
  if (stats) *stats = m3d_outlier_stats{0, 0, 0.0, 0.0, 0.0};
  if (cloud->n == 0) return M3D_OK;  // Open3D: an empty cloud gives an empty result
  hipSetDevice(ctx->device);
  hipStream_t st = S(stream);
  Touch tch{ctx, st};
  char* scratch = nullptr;
  int rc = prep_buffer(ctx, clean_scratch_bytes(cloud->n), &scratch);
  if (rc) return rc;
  std::string why;
  double h[4] = {0.0, 0.0, 0.0, 0.0};
  hipError_t e = statistical_outliers(ctx, cloud, nb_neighbors, std_ratio, index_out, n_out, h, avg_out, scratch,
                                      st, &why);
  if (e != hipSuccess) return hip_fail(ctx, "remove_statistical_outlier", e, why);
  if (stats) *stats = m3d_outlier_stats{*n_out, (int64_t)h[0], h[1], h[2], h[3]};
  return M3D_OK;
}

int m3d_remove_radius_outlier(m3d_ctx* ctx, const m3d_cloud* cloud, int32_t nb_points, double radius,
                              int32_t* index_out, int64_t* n_out, int32_t* count_out, void* stream) {
  if (!ctx) return M3D_ERR_INVALID;
  CHECK_ARG(ctx, cloud && n_out && (index_out || cloud->n == 0), "invalid arguments");
  CHECK_ARG(ctx, nb_points >= 1 && radius > 0.0, "Illegal input parameters, the number of points and radius "
                                                 "must be positive.");
  *n_out = 0;
  if (cloud->n == 0) return M3D_OK;
  hipSetDevice(ctx->device);
  hipStream_t st = S(stream);
  Touch tch{ctx, st};
  const Grid* g = nullptr;  // cell = radius, cached on the cloud like the hybrid search's grid
  int rc = ensure_grid(ctx, cloud, radius, st, &g);
  if (rc) return rc;
  char* scratch = nullptr;
  rc = prep_buffer(ctx, clean_scratch_bytes(cloud->n), &scratch);
  if (rc) return rc;
  hipError_t e = radius_outliers(cloud, g, nb_points, radius, index_out, n_out, count_out, scratch, st);
  if (e != hipSuccess) return hip_fail(ctx, "remove_radius_outlier", e, std::string());
  return M3D_OK;
}

// ------------------------------------------------------------------------------- plane segmentation
// plane.hip; scratch from the context's arena (m3d_plane_score only enqueues)
int32_t m3d_plane_chunk(void) { return kPlaneChunk; }

int m3d_plane_score(m3d_ctx* ctx, const m3d_cloud* cloud, const double* planes, int64_t H,
                    double distance_threshold, int32_t* counts, double* err, void* stream) {
  if (!ctx) return M3D_ERR_INVALID;
  CHECK_ARG(ctx, cloud && H >= 0 && H < ((int64_t)1 << 31), "invalid arguments");
  if (H == 0 || cloud->n == 0) return M3D_OK;  // nothing to score: no array is touched
  CHECK_ARG(ctx, planes && counts, "null device pointer");
  hipSetDevice(ctx->device);
  hipStream_t st = S(stream);
  Touch tch{ctx, st};
  Arena a(ctx, st);
  const size_t o = a.take(plane_score_scratch_bytes(cloud->n, H));
  int rc = a.commit();
  if (rc) return rc;
  HIPX(ctx, plane_score(cloud, planes, H, distance_threshold, counts, err, a.at<char>(o), st));
  return M3D_OK;
}

int m3d_segment_plane(m3d_ctx* ctx, const m3d_cloud* cloud, const m3d_plane_params* p, const int32_t* samples,
                      m3d_plane_result* out, int32_t* inliers_out, int32_t* counts_out, double* err_out,
                      void* stream) {
  if (!ctx) return M3D_ERR_INVALID;
  CHECK_ARG(ctx, cloud && p && out, "invalid arguments");
  CHECK_ARG(ctx, p->ransac_n >= 3, "ransac_n should be set to higher than or equal to 3.");
  CHECK_ARG(ctx, p->ransac_n <= 32, "ransac_n <= 32");
  CHECK_ARG(ctx, p->probability > 0.0 && p->probability <= 1.0, "Probability must be > 0 and <= 1.0");
  CHECK_ARG(ctx, p->num_iterations >= 0, "num_iterations >= 0");
  CHECK_ARG(ctx, std::isfinite(p->distance_threshold) && p->distance_threshold >= 0.0,
            "distance_threshold must be finite and >= 0");
  CHECK_ARG(ctx, cloud->n >= p->ransac_n, "There must be at least 'ransac_n' points.");
  CHECK_ARG(ctx, inliers_out != nullptr, "null device pointer");
  *out = m3d_plane_result{};
  out->best_index = -1;
  hipSetDevice(ctx->device);
  hipStream_t st = S(stream);
  Touch tch{ctx, st};
  const int batch = segment_plane_batch(cloud->n, p);
  Arena a(ctx, st);
  const size_t o = a.take(segment_plane_scratch_bytes(cloud->n, batch));
  int rc = a.commit();
  if (rc) return rc;
  int bad = 0;
  HIPX(ctx, segment_plane(cloud, p, batch, samples, out, inliers_out, counts_out, err_out, a.at<char>(o), st, &bad));
  if (bad) {
    *out = m3d_plane_result{};
    out->best_index = -1;
    return m3d_fail(ctx, M3D_ERR_INVALID, "segment_plane: a sample index is outside [0, n)");
  }
  return M3D_OK;
}

// ------------------------------------------------------------------------------- DBSCAN
// cluster.hip; the grid of cell eps cached on the cloud, scratch from the preprocessing buffer
int m3d_cluster_dbscan(m3d_ctx* ctx, const m3d_cloud* cloud, double eps, int32_t min_points,
                       int32_t* labels_out, m3d_dbscan_result* out, int32_t* sizes_out, int32_t* count_out,
                       void* stream) {
  if (!ctx) return M3D_ERR_INVALID;
  CHECK_ARG(ctx, cloud && out && (labels_out || cloud->n == 0), "invalid arguments");
  CHECK_ARG(ctx, std::isfinite(eps) && eps > 0.0 && min_points >= 1,
            "cluster_dbscan: eps must be finite and > 0, min_points >= 1");
  *out = m3d_dbscan_result{0, 0, 0, -1, 0};
  if (cloud->n == 0) return M3D_OK;
  hipSetDevice(ctx->device);
  hipStream_t st = S(stream);
  Touch tch{ctx, st};
  const Grid* g = nullptr;
  int rc = ensure_grid(ctx, cloud, eps, st, &g);
  if (rc) return rc;
  char* scratch = nullptr;
  rc = prep_buffer(ctx, cluster_scratch_bytes(cloud->n), &scratch);
  if (rc) return rc;
  std::string why;
  hipError_t e = cluster_dbscan(ctx, cloud, g, eps, min_points, labels_out, out, sizes_out, count_out, scratch, st, &why);
  if (e != hipSuccess) {
    *out = m3d_dbscan_result{0, 0, 0, -1, 0};
    return hip_fail(ctx, "cluster_dbscan", e, why);
  }
  return M3D_OK;
}

// ------------------------------------------------------------------------------- ISS keypoints
// iss.hip (clean.hip for the resolution); the grids of cell salient_radius / non_max_radius cached
// on the cloud, scratch from the preprocessing buffer
int m3d_model_resolution(m3d_ctx* ctx, const m3d_cloud* cloud, double* res_out, void* stream) {
  if (!ctx) return M3D_ERR_INVALID;
  CHECK_ARG(ctx, cloud && res_out, "invalid arguments");
  *res_out = 0.0;
  if (cloud->n == 0) return M3D_OK;
  hipSetDevice(ctx->device);
  hipStream_t st = S(stream);
  Touch tch{ctx, st};
  char* scratch = nullptr;
  int rc = prep_buffer(ctx, clean_scratch_bytes(cloud->n), &scratch);
  if (rc) return rc;
  std::string why;
  hipError_t e = model_resolution(ctx, cloud, res_out, scratch, st, &why);
  if (e != hipSuccess) {
    *res_out = 0.0;
    return hip_fail(ctx, "model_resolution", e, why);
  }
  return M3D_OK;
}

int m3d_compute_iss_keypoints(m3d_ctx* ctx, const m3d_cloud* cloud, const m3d_iss_params* params,
                              m3d_iss_result* out, int32_t* index_out, double* third_out, int32_t* count_out,
                              void* stream) {
  if (!ctx) return M3D_ERR_INVALID;
  CHECK_ARG(ctx, cloud && params && out && (index_out || cloud->n == 0), "invalid arguments");
  double rs = params->salient_radius, rn = params->non_max_radius;
  CHECK_ARG(ctx, std::isfinite(rs) && rs >= 0.0 && std::isfinite(rn) && rn >= 0.0,
            "compute_iss_keypoints: the radii must be finite and >= 0");
  CHECK_ARG(ctx, std::isfinite(params->gamma_21) && std::isfinite(params->gamma_32) && params->min_neighbors >= 0,
            "compute_iss_keypoints: the gammas must be finite, min_neighbors >= 0");
  *out = m3d_iss_result{0, 0, 0, rs, rn, 0.0};
  const int64_t n = cloud->n;
  if (n == 0) return M3D_OK;
  hipSetDevice(ctx->device);
  hipStream_t st = S(stream);
  Touch tch{ctx, st};
  const size_t clean_bytes = clean_scratch_bytes(n);
  char* scratch = nullptr;
  int rc = prep_buffer(ctx, clean_bytes + iss_scratch_bytes(n), &scratch);
  if (rc) return rc;
  std::string why;
  if (rs == 0.0 || rn == 0.0) {
    double res = 0.0;
    hipError_t e = model_resolution(ctx, cloud, &res, scratch, st, &why);
    if (e != hipSuccess) return hip_fail(ctx, "compute_iss_keypoints (model resolution)", e, why);
    rs = 6.0 * res;
    rn = 4.0 * res;
    out->resolution = res;
    out->salient_radius = rs;
    out->non_max_radius = rn;
  }
  if (!(rs > 0.0 && rn > 0.0) || !std::isfinite(rs)) {  // coincident points (or one): nothing is salient
    if (third_out) HIPX(ctx, hipMemsetAsync(third_out, 0, sizeof(double) * (size_t)n, st));
    if (count_out) HIPX(ctx, hipMemsetAsync(count_out, 0, sizeof(int32_t) * (size_t)n, st));
    HIPX(ctx, hipStreamSynchronize(st));
    return M3D_OK;
  }
  const Grid *gs = nullptr, *gn = nullptr;
  if ((rc = ensure_grid(ctx, cloud, rs, st, &gs)) != 0) return rc;
  if ((rc = ensure_grid(ctx, cloud, rn, st, &gn)) != 0) return rc;
  int64_t tally[3] = {0, 0, 0};
  hipError_t e = iss_keypoints(ctx, cloud, gs, gn, rs, rn, params->gamma_21, params->gamma_32,
                               params->min_neighbors, index_out, third_out, count_out, tally, scratch + clean_bytes,
                               scratch, st);
  if (e != hipSuccess) return hip_fail(ctx, "compute_iss_keypoints", e, why);
  out->num_keypoints = tally[0];
  out->num_salient = tally[1];
  out->num_counted = tally[2];
  return M3D_OK;
}

// ------------------------------------------------------------------------------- Fast Global Registration
// fgr.hip; scratch is an allocation of the call's own (api_internal.h, source 5)
int32_t m3d_fgr_trial_batch(void) { return kFgrTrialBatch; }
int32_t m3d_fgr_one_wg_rows(void) { return kFgrOneWgRows; }

int m3d_fgr_on_correspondences(m3d_ctx* ctx, const m3d_cloud* src, const m3d_cloud* tgt, const int32_t* corr,
                               int64_t nc, const m3d_fgr_params* p, m3d_fgr_result* out, int32_t* rows_out,
                               int32_t* corr_set_out, void* stream) {
  if (!ctx) return M3D_ERR_INVALID;
  int rc = fgr_check(ctx, src, tgt, nc, p);
  if (rc) return rc;
  CHECK_ARG(ctx, out != nullptr, "invalid arguments");
  hipSetDevice(ctx->device);
  hipStream_t st = S(stream);
  memset(out, 0, sizeof(*out));
  for (int k = 0; k < 16; ++k) out->T[k] = out->T_norm[k] = (k % 5 == 0) ? 1.0 : 0.0;
  const int64_t ns = src->n, nt = tgt->n;
  if (ns == 0 || nt == 0) {
    Touch tch{ctx, st};
    if (corr_set_out && ns > 0) HIPX(ctx, hipMemsetAsync(corr_set_out, 0xFF, 4 * ns, st));
    HIPX(ctx, hipStreamSynchronize(st));
    return M3D_OK;
  }
  {
    Touch tch{ctx, st};
    DevTmp<char> scratch;
    rc = fgr_rows_call(ctx, src, tgt, corr, nc, p, out, rows_out, &scratch, st);
    if (rc) return rc;
    CHECK_ARG(ctx, p->path != 1 || out->n_rows <= kFgrOneWgRows, "fgr: path 1 holds at most m3d_fgr_one_wg_rows rows");
    HIPX(ctx, fgr_optimise(ctx, ns, nt, nc, p, out, scratch.p, st));
  }
  // O = (R, ((−R·m1) + g·t) + m0), returned: O⁻¹ = (Rᵀ, −Rᵀ·o)
  const double* Tn = out->T_norm;
  const double g = out->scale_global;
  double o[3];
  for (int i = 0; i < 3; ++i) {
    const double rm = (Tn[4 * i] * out->mean_tgt[0] + Tn[4 * i + 1] * out->mean_tgt[1]) + Tn[4 * i + 2] * out->mean_tgt[2];
    o[i] = ((0.0 - rm) + g * Tn[4 * i + 3]) + out->mean_src[i];
  }
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) out->T[4 * i + j] = Tn[4 * j + i];
    out->T[4 * i + 3] = 0.0 - ((Tn[i] * o[0] + Tn[4 + i] * o[1]) + Tn[8 + i] * o[2]);
  }
  if (p->maximum_correspondence_distance > 0.0) {
    m3d_eval_result ev;
    rc = m3d_evaluate_registration(ctx, src, tgt, out->T, p->maximum_correspondence_distance, M3D_NN_GRID, 0, &ev,
                                   corr_set_out, nullptr, stream);
    if (rc) return rc;
    out->fitness = ev.fitness;
    out->inlier_rmse = ev.inlier_rmse;
  } else if (corr_set_out) {
    HIPX(ctx, hipMemsetAsync(corr_set_out, 0xFF, 4 * ns, st));
    HIPX(ctx, hipStreamSynchronize(st));
  }
  return M3D_OK;
}

int m3d_fgr_tuple_test(m3d_ctx* ctx, const m3d_cloud* src, const m3d_cloud* tgt, const int32_t* corr, int64_t nc,
                       const m3d_fgr_params* p, int32_t* rows_out, int64_t* n_rows_out, int64_t* trials_out,
                       void* stream) {
  if (!ctx) return M3D_ERR_INVALID;
  int rc = fgr_check(ctx, src, tgt, nc, p);
  if (rc) return rc;
  CHECK_ARG(ctx, n_rows_out && trials_out && (rows_out || nc == 0), "invalid arguments");
  *n_rows_out = *trials_out = 0;
  if (src->n == 0 || tgt->n == 0) return M3D_OK;
  hipSetDevice(ctx->device);
  hipStream_t st = S(stream);
  Touch tch{ctx, st};
  DevTmp<char> scratch;
  m3d_fgr_result r;
  memset(&r, 0, sizeof(r));
  rc = fgr_rows_call(ctx, src, tgt, corr, nc, p, &r, rows_out, &scratch, st);
  if (rc) return rc;
  *n_rows_out = r.n_rows;
  *trials_out = r.trials;
  return M3D_OK;
}

int m3d_fgr_terms(m3d_ctx* ctx, const double* p, const double* q, int64_t n, double par, double* sums27_out,
                  void* stream) {
  if (!ctx) return M3D_ERR_INVALID;
  CHECK_ARG(ctx, sums27_out && n >= 0 && n < ((int64_t)1 << 31) && (n == 0 || (p && q)), "invalid arguments");
  for (int k = 0; k < 27; ++k) sums27_out[k] = 0.0;
  if (n == 0) return M3D_OK;
  hipSetDevice(ctx->device);
  hipStream_t st = S(stream);
  Touch tch{ctx, st};
  DevTmp<char> scratch;
  int rc = dev_alloc(ctx, &scratch.p, (int64_t)fgr_terms_scratch_bytes(n));
  if (rc) return rc;
  HIPX(ctx, fgr_terms(ctx, p, q, n, par, 0, sums27_out, scratch.p, st));
  return M3D_OK;
}

// ------------------------------------------------------------------------------- minimum-distance thinning
// thin.hip; the grid of cell `radius` cached on the cloud, scratch from the preprocessing buffer
int m3d_thin_min_distance(m3d_ctx* ctx, const m3d_cloud* cloud, double radius, uint64_t seed, int32_t* decided_out,
                          int64_t* kept_count_out, int32_t* rounds_out, void* stream) {
  if (!ctx) return M3D_ERR_INVALID;
  CHECK_ARG(ctx, cloud && (decided_out || cloud->n == 0), "invalid arguments");
  CHECK_ARG(ctx, std::isfinite(radius) && radius > 0.0, "thin_min_distance: radius must be finite and > 0");
  if (kept_count_out) *kept_count_out = 0;
  if (rounds_out) *rounds_out = 0;
  if (cloud->n == 0) return M3D_OK;
  hipSetDevice(ctx->device);
  hipStream_t st = S(stream);
  Touch tch{ctx, st};
  const Grid* g = nullptr;
  int rc = ensure_grid(ctx, cloud, radius, st, &g);
  if (rc) return rc;
  char* scratch = nullptr;
  rc = prep_buffer(ctx, thin_scratch_bytes(cloud->n), &scratch);
  if (rc) return rc;
  std::string why;
  int64_t kept = 0;
  int32_t rounds = 0;
  hipError_t e = thin_min_distance(cloud, g, radius, seed, decided_out, &kept, &rounds, scratch, st, &why);
  if (rounds_out) *rounds_out = rounds;
  if (e != hipSuccess) return hip_fail(ctx, "thin_min_distance", e, why);
  if (kept_count_out) *kept_count_out = kept;
  return M3D_OK;
}

}  // extern "C"
