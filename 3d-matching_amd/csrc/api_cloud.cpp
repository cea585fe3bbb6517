// api_cloud.cpp — packed clouds of the C ABI (include/m3d.h): create (device or host arrays) / destroy, and
// what is built once and cached on a cloud: its grids per cell size and its copies in Morton slot order.
#include <algorithm>
#include <cmath>
#include <string>

#include "api_internal.h"

using namespace m3d;
using namespace m3d::api;

namespace {
constexpr int64_t kCloudPad = 1024; // NN tile multiple

// A cloud's centre (mean, unless given), centred fp32 copy, rmax and grid bounds with ONE host
// sync (ransac.hip cloud_pack_kernel).  Temporaries from ctx->tmp, the summary through the pinned page.
int cloud_pack(m3d_ctx* ctx, m3d_cloud* c, int64_t n, bool mean, hipStream_t st) {
  c->rmax = 0.0;
  c->has_bounds = false;
  if (c->n_pad == 0) return M3D_OK;
  int rc = pin_ensure(ctx);
  if (rc) return rc;
  const int sblocks = 128;
  const int blocks = (int)std::min<int64_t>(1024, (c->n_pad + 255) / 256);
  // scratch [block sums | centre | block (rmax, lo, hi)]; the summary goes to pinned memory
  const size_t o_sum = 0, o_c = tmp_align(sizeof(double) * 3 * sblocks), o_p7 = o_c + tmp_align(3 * sizeof(double));
  const size_t bytes = o_p7 + tmp_align(sizeof(float) * 7 * blocks);
  hipError_t e = ctx->tmp.reserve(bytes);
  if (e != hipSuccess) return m3d_fail(ctx, M3D_ERR_OOM, "cloud scratch");
  char* b = ctx->tmp.base;
  double* cdev = reinterpret_cast<double*>(b + o_c);
  double* sum_part = reinterpret_cast<double*>(b + o_sum);
  float* p7 = reinterpret_cast<float*>(b + o_p7);
  const bool dmean = mean && n > 0;
  double* pin_c = pin_read<double>(ctx, true);
  float* pin7 = reinterpret_cast<float*>(pin_c + 3);
  if (dmean) e = launch_sum3(c->xyz64, n, sum_part, sblocks, st);
  if (e == hipSuccess)
    e = launch_cloud_pack(c->xyz64, n, c->n_pad, dmean ? sum_part : nullptr, sblocks, cdev, c->center, c->xyz32,
                          kFar, p7, blocks, pin_c, pin7, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return m3d_fail(ctx, M3D_ERR_HIP, hipGetErrorString(e));
  const volatile double* hc = pin_read<double>(ctx, false);
  const volatile float* h = reinterpret_cast<const volatile float*>(hc + 3);
  if (dmean)
    for (int k = 0; k < 3; ++k) c->center[k] = hc[k];
  for (int k = 0; k < 3; ++k) {
    c->lo[k] = h[1 + k];
    c->hi[k] = h[4 + k];
  }
  c->rmax = (double)h[0] * (1.0 + 1e-6);
  c->has_bounds = n > 0;
  return M3D_OK;
}

// Host arrays → device: pageable hipMemcpyAsync straight into the cloud's buffers (the runtime
// stages them itself).  Measured against pinned staging through the host pool and against
// hipHostRegister of the caller's arrays (round 3): both were slower at cfg1 sizes.
int upload_host(m3d_ctx* ctx, int narr, void* const* dst, const void* const* src, const size_t* bytes,
                hipStream_t st) {
  for (int i = 0; i < narr; ++i)
    if (bytes[i] > 0) HIPX(ctx, hipMemcpyAsync(dst[i], src[i], bytes[i], hipMemcpyHostToDevice, st));
  return M3D_OK;
}

int cloud_create(m3d_ctx* ctx, const double* xyz, const double* normals, int64_t n, const double* center,
                 bool host, void* stream, m3d_cloud** out) {
  if (!ctx) return M3D_ERR_INVALID;
  CHECK_ARG(ctx, out != nullptr, "null output");
  CHECK_ARG(ctx, n >= 0 && n < (int64_t)1 << 31, "point count out of range");
  CHECK_ARG(ctx, n == 0 || xyz != nullptr, "null device pointer");
  CHECK_ARG(ctx, center == nullptr || (std::isfinite(center[0]) && std::isfinite(center[1]) &&
                                       std::isfinite(center[2])),
            "non-finite centre");
  hipSetDevice(ctx->device);
  hipStream_t st = S(stream);
  Touch tch{ctx, st};
  m3d_cloud* c = new m3d_cloud();
  c->ctx = ctx;
  c->ctx_id = ctx->id;
  c->n = n;
  c->n_pad = round_up(std::max<int64_t>(n, 1), kCloudPad);
  int rc = M3D_OK;
  {
    Carve cv;  // the three point arrays in one allocation
    if (n > 0) cv.add(&c->xyz64, 3 * (size_t)n);
    if (n > 0 && normals) cv.add(&c->nrm64, 3 * (size_t)n);
    cv.add(&c->xyz32, (size_t)c->n_pad);
    if (cv.alloc(&c->block, &c->block_bytes, st) != hipSuccess) rc = m3d_fail(ctx, M3D_ERR_OOM, "device allocation failed (cloud)");
  }
  if (rc) {
    m3d_cloud_destroy(c);
    return rc;
  }
  if (n > 0 && host) {
    void* const dst[2] = {c->xyz64, c->nrm64};
    const void* const srcs[2] = {xyz, normals};
    const size_t bytes[2] = {sizeof(double) * 3 * (size_t)n, normals ? sizeof(double) * 3 * (size_t)n : 0};
    rc = upload_host(ctx, 2, dst, srcs, bytes, st);
    if (rc) {
      m3d_cloud_destroy(c);
      return rc;
    }
  } else if (n > 0) {
    hipError_t e = hipMemcpyAsync(c->xyz64, xyz, sizeof(double) * 3 * n, hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess && normals)
      e = hipMemcpyAsync(c->nrm64, normals, sizeof(double) * 3 * n, hipMemcpyDeviceToDevice, st);
    if (e != hipSuccess) {
      m3d_cloud_destroy(c);
      return m3d_fail(ctx, M3D_ERR_HIP, hipGetErrorString(e));
    }
  }
  if (center != nullptr) {
    for (int k = 0; k < 3; ++k) c->center[k] = center[k];
    c->center_given = 1;
  }
  rc = cloud_pack(ctx, c, n, center == nullptr, st);
  if (!rc) {
    // fp16 screen operand scale: a power of two with |S·x|∞ ≤ 32 (nn_brute.hip pack16_sorted)
    int ex = 0;
    std::frexp(std::max(c->rmax, 1e-30) / 32.0, &ex);
    c->s16 = std::ldexp(1.0, -std::min(std::max(ex, -100), 100));
  }
  if (rc) {
    m3d_cloud_destroy(c);
    return rc;
  }
  *out = c;
  return M3D_OK;
}
}  // namespace

namespace m3d {
namespace api {
// uniform grid of a cloud for cell size `cell` (built once, synchronously, and cached on the
// cloud per cell size)
int ensure_grid(m3d_ctx* ctx, const m3d_cloud* c, double cell, hipStream_t st, const Grid** out) {
  for (Grid* g : c->grids)
    if (g->cell_req == cell && g->n_pts == c->n) {
      *out = g;
      return M3D_OK;
    }
  Grid* g = new Grid();
  float lohi[6];
  for (int k = 0; k < 3; ++k) {
    lohi[k] = c->lo[k];
    lohi[3 + k] = c->hi[k];
  }
  // asynchronous: the cloud's packing pass gave the bounds, the temporaries come from the arena
  hipError_t e = grid_build(c->xyz32, c->n, cell, st, g, &ctx->tmp, c->has_bounds ? lohi : nullptr);
  if (e != hipSuccess) {
    grid_free(g);
    delete g;
    return m3d_fail(ctx, M3D_ERR_HIP, std::string("grid build: ") + hipGetErrorString(e));
  }
  g->cell_req = cell;
  c->grids.push_back(g);
  *out = g;
  return M3D_OK;
}

// The ICP source in Morton slot order for cell size `cell` (grid.hip morton_source), built once and
// cached on the caller's cloud; sg = the caller's grid at that cell size.
int ensure_morton_source(m3d_ctx* ctx, const m3d_cloud* c, double cell, const m3d_cloud** out,
                         const Grid** gout) {
  for (auto& m : c->morton)
    if (m.first == cell && m.second->n == c->n) {
      *out = m.second;
      *gout = m.second->grids.front();
      return M3D_OK;
    }
  // straight from the points (grid.hip morton_source: the slots without the source's cell grid)
  m3d_cloud* mc = new m3d_cloud();
  mc->ctx = ctx;
  mc->ctx_id = ctx->id;
  Grid* g = new Grid();
  mc->grids.push_back(g);
  hipError_t e = morton_source(c, cell, mc, g, &ctx->tmp, nullptr);
  if (e != hipSuccess) {
    m3d_cloud_destroy(mc);
    return m3d_fail(ctx, M3D_ERR_HIP, std::string("morton source: ") + hipGetErrorString(e));
  }
  c->morton.emplace_back(cell, mc);
  // bounded cache: callers that query with many different radii (m3d_nn1, the a6 validation) would
  // otherwise keep one full source copy per cell size for the cloud's lifetime
  constexpr size_t kMortonKeep = 4;
  for (size_t k = 0; c->morton.size() > kMortonKeep && k + 1 < c->morton.size();) {
    if (c->morton[k].second->refs == 0) {
      m3d_cloud_destroy(c->morton[k].second);
      c->morton.erase(c->morton.begin() + (ptrdiff_t)k);
    } else {
      ++k;
    }
  }
  *out = mc;
  *gout = g;
  return M3D_OK;
}
}  // namespace api
}  // namespace m3d

extern "C" {

// ------------------------------------------------------------------------------- clouds
int m3d_cloud_create(m3d_ctx* ctx, const double* xyz, const double* normals, int64_t n,
                     void* stream, m3d_cloud** out) {
  return m3d_cloud_create_framed(ctx, xyz, normals, n, nullptr, stream, out);
}

int m3d_cloud_create_framed(m3d_ctx* ctx, const double* xyz, const double* normals, int64_t n,
                            const double* center, void* stream, m3d_cloud** out) {
  return cloud_create(ctx, xyz, normals, n, center, false, stream, out);
}

int m3d_cloud_create_host(m3d_ctx* ctx, const double* xyz, const double* normals, int64_t n,
                          const double* center, void* stream, m3d_cloud** out) {
  return cloud_create(ctx, xyz, normals, n, center, true, stream, out);
}

void m3d_cloud_destroy(m3d_cloud* c) {
  if (!c) return;
  // the blocks go back to the cache marked after every stream the context used (stream-ordered
  // reuse, no device sync)
  ReleaseScope rs(c->ctx, c->ctx_id);
  for (Grid* g : c->grids) {
    grid_free(g);
    delete g;
  }
  // Morton copies a live ICP loop still runs on are detached, not freed: the last loop to go
  // frees them (m3d_icp_destroy), so destroying the source before its loops stays safe
  for (auto& m : c->morton) {
    if (m.second->refs > 0)
      m.second->orphan = true;
    else
      m3d_cloud_destroy(m.second);
  }
  for (void** p : {reinterpret_cast<void**>(&c->slot), reinterpret_cast<void**>(&c->xyz64),
                   reinterpret_cast<void**>(&c->nrm64), reinterpret_cast<void**>(&c->xyz32)})
    if (in_block(*p, c->block, c->block_bytes)) *p = nullptr;
  block_release(c->block);
  hipFree(c->slot);
  hipFree(c->xyz64);
  hipFree(c->nrm64);
  hipFree(c->xyz32);
  block_release(c->rec64);
  delete c;
}

int64_t m3d_cloud_size(const m3d_cloud* c) { return c ? c->n : -1; }

}  // extern "C"
