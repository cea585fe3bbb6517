// api_mesh.cpp — triangle meshes of the C ABI (include/m3d.h): create / destroy, closest points, ray casting,
// surface sampling and ICP against a mesh.  A query's scratch comes from the context's preprocessing
// buffer, the mesh ICP loop's arrays from the run arena (api_internal.h, sources 4 and 3); the mesh's
// arrays, its grid and its sampling weights are blocks of the block cache.
#include <cmath>
#include <string>

#include "api_internal.h"

using namespace m3d;
using namespace m3d::api;

namespace {
// What every query on a mesh checks, and its path: `path` is 0, 1 or 2 and the mesh has a triangle to
// query; *brute: the brute-force sweep (path 1, or path 0 on a mesh of at most auto_brute_max
// triangles — the caller's threshold, m3d_internal.h kMesh*AutoBruteMax), else the grid.  brute null
// (surface sampling takes no path): the mesh's check alone
int mesh_path(m3d_ctx* ctx, const m3d_mesh* mesh, int32_t path, int64_t auto_brute_max, bool* brute) {
  CHECK_ARG(ctx, path >= 0 && path <= 2, "path: 0 automatic, 1 brute force, 2 grid");
  CHECK_ARG(ctx, mesh->usable > 0, "the mesh has no usable triangle (none, or every one degenerate or not finite)");
  if (brute != nullptr) *brute = path == 1 || (path == 0 && mesh->nf <= auto_brute_max);
  return M3D_OK;
}

// ------------------------------------------------------------------------------- ray casting
// mesh_ray.hip; the two calls differ in their outputs alone (count_out null: the first hit)
int mesh_rays(m3d_ctx* ctx, m3d_mesh* mesh, const double* rays, int64_t n, double tnear, double tfar, int32_t path,
              double* t_out, int32_t* tri_out, double* uv_out, int32_t* count_out, void* stream, const char* what) {
  bool brute = false;
  const int prc = mesh_path(ctx, mesh, path, kMeshRayAutoBruteMax, &brute);
  if (prc) return prc;
  mesh->last_ray_path = brute ? 1 : 2;
  mesh->last_ray_fallback = 0;
  if (n == 0) return M3D_OK;
  hipSetDevice(ctx->device);
  hipStream_t st = S(stream);
  Touch tch{ctx, st};
  if (brute) {
    HIPX(ctx, mesh_rays_brute(mesh, rays, n, tnear, tfar, t_out, tri_out, uv_out, count_out, st));
    return M3D_OK;
  }
  char* scratch = nullptr;
  const int rc = prep_buffer(ctx, 256, &scratch);
  if (rc) return rc;
  std::string why;
  const hipError_t e = mesh_rays_grid(ctx, mesh, rays, n, tnear, tfar, t_out, tri_out, uv_out, count_out, scratch,
                                      &mesh->last_ray_fallback, st, &why);
  if (e != hipSuccess) return hip_fail(ctx, what, e, why);
  return M3D_OK;
}

// ------------------------------------------------------------------------------- surface sampling
// mesh_sample.hip; the cumulative weights are built by the first call and cached on the mesh
int mesh_sample_ready(m3d_ctx* ctx, m3d_mesh* mesh, hipStream_t st) {
  const int prc = mesh_path(ctx, mesh, 0, 0, nullptr);
  if (prc) return prc;
  if (!mesh->sample_built) {
    hipSetDevice(ctx->device);
    Touch tch{ctx, st};
    HIPX(ctx, mesh_sample_build(ctx, mesh, st));
  }
  CHECK_ARG(ctx, mesh->sample_W > 0, "the mesh has no triangle with a finite non-zero area");
  return M3D_OK;
}

// ------------------------------------------------------------------------------- ICP against a mesh
// mesh_icp.hip.  A loop of its own around the mesh only where m3d_icp is bound to a target cloud's
// NN — the scan and its arrays.  The state's reset, the solve and the result read are the cloud
// loops' (launch_icp_state_init, launch_icp_solve_state, read_result).  The arrays come from the
// context's run arena (the calls synchronise before returning), the source is in the Morton slot
// order of its cloud, the mesh's grid is built on first use.  `init` is affine, as every documented
// input is and matmul4_affine assumes: the state starts with the bottom row (0, 0, 0, 1) whatever
// the caller's last four values, m3d_icp_reset's rule.  Profiling (m3d_profile_*): the scan under
// M3D_KERNEL_NN, terms + reduce under M3D_KERNEL_TERMS, the solve under M3D_KERNEL_LOOP.
struct MeshIcpCall {
  MeshIcpLoop L;
  const m3d_cloud* ms = nullptr;  // the source's Morton copy
  bool brute = false;
  int32_t kind = M3D_KERNEL_L2;
  double k = 1.0;
};

// the checks both entry points share, the path, the loop's arrays and its state at `init`
int mesh_icp_setup(m3d_ctx* ctx, m3d_mesh* mesh, const m3d_cloud* src, const double* init, double max_dist,
                   const m3d_robust_kernel* kernel, int32_t path, MeshIcpCall* c, hipStream_t st) {
  CHECK_ARG(ctx, src != nullptr, "invalid arguments");
  CHECK_ARG(ctx, std::isfinite(max_dist) && max_dist > 0.0, "Invalid max_correspondence_distance.");
  if (kernel != nullptr) {
    const int rc = robust_check(ctx, kernel);
    if (rc) return rc;
    c->kind = kernel->kind;
    c->k = kernel->k;
  }
  const int prc = mesh_path(ctx, mesh, path, kMeshIcpAutoBruteMax, &c->brute);
  if (prc) return prc;
  hipSetDevice(ctx->device);
  MeshIcpLoop& L = c->L;
  L.ns = src->n;
  L.max_dist = max_dist;
  if (!c->brute) {
    std::string why;
    const hipError_t e = mesh_grid_build(ctx, mesh, st, &why);
    if (e != hipSuccess) return hip_fail(ctx, "mesh_icp", e, why);
  }
  if (L.ns > 0) {
    const Grid* sg = nullptr;
    const int rc = ensure_morton_source(ctx, src, max_dist * 1.001, &c->ms, &sg);
    if (rc) return rc;
    HIPX(ctx, hipStreamSynchronize(nullptr));  // the copy is made on the null stream
  }
  const size_t n1 = (size_t)std::max<int64_t>(L.ns, 1);
  Carve cv;
  cv.add(&L.state, 1);
  cv.add(&L.sums, kTermSlots);
  cv.add(&L.partials, (size_t)kTermSlots * (size_t)std::max<int64_t>(side_terms_blocks(L.ns), 1));
  cv.add(&L.pcd64, 3 * n1);
  cv.add(&L.tri, n1);
  cv.add(&L.d2, n1);
  cv.add(&L.pt, 3 * n1);
  if (ctx->run.reserve(cv.bytes()) != hipSuccess)
    return m3d_fail(ctx, M3D_ERR_OOM, "device allocation failed (mesh ICP loop arrays)");
  cv.place(ctx->run.base);
  if (L.ns > 0) {
    HIPX(ctx, hipMemcpyAsync(L.pcd64, c->ms->xyz64, sizeof(double) * 3 * (size_t)L.ns, hipMemcpyDeviceToDevice, st));
    HIPX(ctx, hipMemsetAsync(L.tri, 0xFF, sizeof(int32_t) * (size_t)L.ns, st));  // no seed, no match: −1
  }
  const double* T = init != nullptr ? init : kIdentity16;
  HIPX(ctx, launch_icp_state_init(L.state, T, apply_init_of(T, true), max_dist * max_dist, mesh_icp_frame(), st));
  return M3D_OK;
}
}  // namespace

extern "C" {

// ------------------------------------------------------------------------------- point-to-mesh distance
// mesh.hip
int m3d_mesh_create(m3d_ctx* ctx, const double* vertices, int64_t nv, const int32_t* triangles, int64_t nf,
                    m3d_mesh** out) {
  if (!ctx) return M3D_ERR_INVALID;
  CHECK_ARG(ctx, out != nullptr, "null output");
  *out = nullptr;
  CHECK_ARG(ctx, nv >= 0 && nv < ((int64_t)1 << 31) && nf >= 0 && nf < ((int64_t)1 << 26), "mesh size out of range");
  CHECK_ARG(ctx, (nv == 0 || vertices) && (nf == 0 || triangles), "null device pointer");
  hipSetDevice(ctx->device);
  hipStream_t st = nullptr;
  Touch tch{ctx, st};
  m3d_mesh* m = new m3d_mesh();
  m->ctx = ctx;
  m->ctx_id = ctx->id;
  m->nv = nv;
  m->nf = nf;
  Carve cv;
  cv.add(&m->v64, 3 * (size_t)nv);
  cv.add(&m->tri, 3 * (size_t)nf);
  cv.add(&m->tri9, 9 * (size_t)nf);
  cv.add(&m->ok, (size_t)nf);
  if (cv.alloc(&m->block, &m->block_bytes, st) != hipSuccess) {
    m3d_mesh_destroy(m);
    return m3d_fail(ctx, M3D_ERR_OOM, "device allocation failed (mesh)");
  }
  hipError_t e = hipSuccess;
  if (nv > 0) e = hipMemcpyAsync(m->v64, vertices, sizeof(double) * 3 * (size_t)nv, hipMemcpyDeviceToDevice, st);
  if (e == hipSuccess && nf > 0)
    e = hipMemcpyAsync(m->tri, triangles, sizeof(int32_t) * 3 * (size_t)nf, hipMemcpyDeviceToDevice, st);
  int bad = 0;
  if (e == hipSuccess) e = mesh_upload(m, st, &bad);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess || bad != 0) {
    m3d_mesh_destroy(m);
    if (e != hipSuccess) return m3d_fail(ctx, M3D_ERR_HIP, std::string("mesh upload: ") + hipGetErrorString(e));
    return m3d_fail(ctx, M3D_ERR_INVALID, "triangle index outside [0, number of vertices)");
  }
  *out = m;
  return M3D_OK;
}

void m3d_mesh_destroy(m3d_mesh* m) {
  if (!m) return;
  ReleaseScope rs(m->ctx, m->ctx_id);
  if (m->gblock) block_release(m->gblock);
  if (m->sblock) block_release(m->sblock);
  if (m->block) block_release(m->block);
  delete m;
}

int64_t m3d_mesh_size(const m3d_mesh* m) { return m ? m->nf : -1; }

int m3d_mesh_closest(m3d_ctx* ctx, m3d_mesh* mesh, const double* xyz, int64_t n, const double* T, int32_t path,
                     double r0, double* d2_out, int32_t* tri_out, double* point_out, double* uv_out,
                     uint8_t* region_out, void* stream) {
  if (!ctx) return M3D_ERR_INVALID;
  CHECK_ARG(ctx, mesh && n >= 0 && n < ((int64_t)1 << 31) && (n == 0 || xyz), "invalid arguments");
  bool brute = false;
  int rc = mesh_path(ctx, mesh, path, kMeshAutoBruteMax, &brute);
  if (rc) return rc;
  mesh->last_rounds = 0;
  if (n == 0) return M3D_OK;
  hipSetDevice(ctx->device);
  hipStream_t st = S(stream);
  Touch tch{ctx, st};
  double T12[12];
  if (T != nullptr)
    for (int k = 0; k < 12; ++k) T12[k] = T[k];
  const double* Tp = T != nullptr ? T12 : nullptr;
  if (brute) {
    HIPX(ctx, mesh_closest_brute(mesh, xyz, n, Tp, d2_out, tri_out, point_out, uv_out, region_out, st));
    return M3D_OK;
  }
  char* scratch = nullptr;
  rc = prep_buffer(ctx, mesh_scratch_bytes(n), &scratch);
  if (rc) return rc;
  std::string why;
  hipError_t e = mesh_closest_grid(ctx, mesh, xyz, n, Tp, r0, d2_out, tri_out, point_out, uv_out, region_out,
                                   scratch, st, &why);
  if (e != hipSuccess) return hip_fail(ctx, "mesh_closest", e, why);
  return M3D_OK;
}

int m3d_mesh_grid_info(const m3d_mesh* mesh, int64_t* out4) {
  if (!mesh || !out4) return M3D_ERR_INVALID;
  out4[0] = mesh->grid_built ? mesh->grid.ncells : 0;
  out4[1] = mesh->grid_built ? mesh->nrefs : 0;
  out4[2] = mesh->grid_built ? mesh->doublings : 0;
  out4[3] = mesh->last_rounds;
  return M3D_OK;
}

int m3d_mesh_cast_rays(m3d_ctx* ctx, m3d_mesh* mesh, const double* rays, int64_t n, double tnear, double tfar,
                       int32_t path, double* t_out, int32_t* tri_out, double* uv_out, void* stream) {
  if (!ctx) return M3D_ERR_INVALID;
  CHECK_ARG(ctx, mesh && n >= 0 && n < ((int64_t)1 << 31) && (n == 0 || rays), "invalid arguments");
  return mesh_rays(ctx, mesh, rays, n, tnear, tfar, path, t_out, tri_out, uv_out, nullptr, stream, "mesh_cast_rays");
}

int m3d_mesh_count_rays(m3d_ctx* ctx, m3d_mesh* mesh, const double* rays, int64_t n, double tnear, double tfar,
                        int32_t path, int32_t* count_out, void* stream) {
  if (!ctx) return M3D_ERR_INVALID;
  CHECK_ARG(ctx, mesh && n >= 0 && n < ((int64_t)1 << 31) && (n == 0 || (rays && count_out)), "invalid arguments");
  return mesh_rays(ctx, mesh, rays, n, tnear, tfar, path, nullptr, nullptr, nullptr, count_out, stream,
                   "mesh_count_rays");
}

int m3d_mesh_ray_info(const m3d_mesh* mesh, int64_t* out2) {
  if (!mesh || !out2) return M3D_ERR_INVALID;
  out2[0] = mesh->last_ray_path;
  out2[1] = mesh->last_ray_fallback;
  return M3D_OK;
}

int32_t m3d_mesh_ray_auto_brute_max(void) { return kMeshRayAutoBruteMax; }

int m3d_mesh_sample(m3d_ctx* ctx, m3d_mesh* mesh, int64_t n, uint64_t seed, double* points_out,
                    int32_t* triangle_out, double* uv_out, double* normals_out, void* stream) {
  if (!ctx) return M3D_ERR_INVALID;
  CHECK_ARG(ctx, mesh && n >= 0 && n < ((int64_t)1 << 31), "invalid arguments");
  hipStream_t st = S(stream);
  const int rc = mesh_sample_ready(ctx, mesh, st);
  if (rc) return rc;
  if (n == 0) return M3D_OK;
  hipSetDevice(ctx->device);
  Touch tch{ctx, st};
  HIPX(ctx, mesh_sample(mesh, n, seed, points_out, triangle_out, uv_out, normals_out, st));
  HIPX(ctx, hipStreamSynchronize(st));
  return M3D_OK;
}

int m3d_mesh_sample_info(const m3d_mesh* mesh, uint64_t* out2) {
  if (!mesh || !out2) return M3D_ERR_INVALID;
  out2[0] = mesh->sample_built ? mesh->sample_W : 0;
  out2[1] = mesh->sample_built ? (uint64_t)mesh->sample_nonzero : 0;
  return M3D_OK;
}

int m3d_mesh_icp_terms(m3d_ctx* ctx, m3d_mesh* mesh, const m3d_cloud* src, const double* T_host, double max_dist,
                       const m3d_robust_kernel* kernel, int32_t path, const int32_t* seed_tri, double* sums_out,
                       int32_t* tri_idx, double* d2_out, void* stream) {
  if (!ctx || !mesh) return M3D_ERR_INVALID;
  hipStream_t st = S(stream);
  Touch tch{ctx, st};
  CHECK_ARG(ctx, sums_out != nullptr, "null output");
  for (int k = 0; k < kTermSlots; ++k) sums_out[k] = 0.0;
  MeshIcpCall c;
  const int rc = mesh_icp_setup(ctx, mesh, src, T_host, max_dist, kernel, path, &c, st);
  if (rc) return rc;
  const MeshIcpLoop& L = c.L;
  hipError_t e = hipSuccess;
  if (L.ns == 0) {  // nothing to scan; the state's reset is in flight on the arena
    HIPX(ctx, hipStreamSynchronize(st));
    return M3D_OK;
  }
  if (seed_tri != nullptr) e = launch_gather_i32(seed_tri, c.ms->slot, L.ns, L.tri, st);
  if (e == hipSuccess) e = launch_mesh_icp_scan(mesh, L, c.brute, seed_tri != nullptr, st);
  if (e == hipSuccess) e = launch_mesh_icp_terms(mesh, L, c.kind, c.k, L.sums, st);
  if (e == hipSuccess && tri_idx != nullptr) e = launch_scatter_i32(L.tri, c.ms->slot, L.ns, tri_idx, st);
  if (e == hipSuccess && d2_out != nullptr) e = launch_scatter_f64(L.d2, c.ms->slot, L.ns, d2_out, st);
  double sums[kTermSlots];
  if (e == hipSuccess) e = hipMemcpyAsync(sums, L.sums, sizeof sums, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) {
    (void)hipStreamSynchronize(st);
    return m3d_fail(ctx, M3D_ERR_HIP, std::string("mesh_icp_terms: ") + hipGetErrorString(e));
  }
  for (int k = 0; k < 30; ++k) sums_out[k] = sums[k];
  return M3D_OK;
}

int m3d_mesh_icp_run(m3d_ctx* ctx, m3d_mesh* mesh, const m3d_cloud* src, const double* init, double max_dist,
                     const m3d_icp_params* params, const m3d_robust_kernel* kernel, int32_t path, int32_t seed,
                     m3d_icp_result* out, int32_t* tri_idx, void* stream) {
  if (!ctx || !mesh) return M3D_ERR_INVALID;
  hipStream_t st = S(stream);
  Touch tch{ctx, st};
  CHECK_ARG(ctx, out != nullptr && params != nullptr, "null output or parameters");
  CHECK_ARG(ctx, params->estimation == M3D_EST_POINT_TO_PLANE,
            "ICP against a mesh is point-to-plane (the face normal); point-to-point is not implemented");
  CHECK_ARG(ctx, params->max_iteration >= 0, "max_iteration must be >= 0");
  MeshIcpCall c;
  int rc = mesh_icp_setup(ctx, mesh, src, init, max_dist, kernel, path, &c, st);
  if (rc) return rc;
  const MeshIcpLoop& L = c.L;
  auto step = [&](int32_t n) {
    hipError_t e = hipSuccess;
    for (int32_t it = 0; it < n && e == hipSuccess; ++it) {
      {
        KTimer kt(ctx, M3D_KERNEL_NN, st);
        e = launch_mesh_icp_scan(mesh, L, c.brute, seed != 0, st);
      }
      if (e == hipSuccess) {
        KTimer kt(ctx, M3D_KERNEL_TERMS, st);
        e = launch_mesh_icp_terms(mesh, L, c.kind, c.k, L.sums, st);
      }
      if (e == hipSuccess) {
        KTimer kt(ctx, M3D_KERNEL_LOOP, st);
        e = launch_icp_solve_state(L.state, L.sums, params->relative_fitness, params->relative_rmse, params->max_iteration,
                                   M3D_EST_POINT_TO_PLANE, L.ns, kIdentity16, mesh_icp_frame(), st);
      }
    }
    return e == hipSuccess ? M3D_OK : m3d_fail(ctx, M3D_ERR_HIP, std::string("mesh ICP step: ") + hipGetErrorString(e));
  };
  rc = run_chunked(ctx, L.state, params->max_iteration + 1, step, st);
  hipError_t e = hipSuccess;
  if (!rc && tri_idx != nullptr) e = launch_scatter_i32(L.tri, L.ns > 0 ? c.ms->slot : nullptr, L.ns, tri_idx, st);
  // the arena is idle when the call returns: read_result synchronises, a failed call here
  if (!rc && e == hipSuccess) return read_result(ctx, "mesh_icp_run", L.state, nullptr, out, st);
  (void)hipStreamSynchronize(st);
  return rc ? rc : m3d_fail(ctx, M3D_ERR_HIP, std::string("mesh_icp_run: ") + hipGetErrorString(e));
}

int32_t m3d_mesh_brute_tile(void) { return kMeshBruteTile; }
int32_t m3d_mesh_auto_brute_max(void) { return kMeshAutoBruteMax; }

}  // extern "C"
