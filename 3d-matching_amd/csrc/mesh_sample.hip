// mesh_sample.hip — points drawn uniformly from a mesh's surface on the device (Open3D
// TriangleMesh.sample_points_uniformly): per sample the point, its triangle, its barycentric
// (u, v) and the triangle's unit face normal.
//
// CONTRACT (restated in numpy by tests/mesh_sample_restatement.py).  All floating-point arithmetic
// is fp64, one operation at a time (-ffp-contract=off).
//
// WEIGHTS, built once per m3d_mesh by the first call, cached on it and dropped with it.
//   Triangle f = (a, b, c) is USABLE by mesh.hip's rule (nine finite coordinates, c = ab × ac =
//   (ab1*ac2 − ab2*ac1, ab2*ac0 − ab0*ac2, ab0*ac1 − ab1*ac0) not three exact zeros).
//   len_f = sqrt((cx*cx + cy*cy) + cz*cz): twice the area, mesh_icp.hip's expression (the device's
//   fp64 sqrt is correctly rounded).  An unusable triangle, or a len_f that is not finite, counts as
//   len_f = 0.
//   L = max len_f, an integer atomic max over ord_of (mesh_tri.h).  L = m·2^e with m ∈ [0.5, 1):
//   w_f = (uint64) trunc(ldexp(len_f, 32 − e)).  The scaling is by a power of two, hence exact (a
//   result below the normal range is below 1 and truncates to 0 either way), and the largest
//   triangle lands in [2^31, 2^32).  A triangle more than ≈ 2^32 times smaller than the largest one
//   therefore gets weight 0 and is NEVER drawn: its share of the surface is below 2^-32 of the
//   largest triangle's.
//   cum_f = Σ_{g ≤ f} w_g in uint64 (an inclusive scan; the sums are integers, so the scan's order
//   cannot change a bit; F < 2^26 triangles of weight < 2^32 stay far below 2^63), W = cum_{F−1}.
//   W = 0 (no triangle with a finite non-zero len_f) is an error of the call.
//
// SAMPLE k of a call with `seed` (sampler.h): base = sample_base(seed, k), x_j = splitmix64(base + j).
//   t = the high 64 bits of x_0 · W, so t ∈ [0, W).  The triangle is the smallest f with cum_f > t: a
//   triangle of weight 0 has cum_f = cum_{f−1} (or 0 for f = 0) and can never be that f, wherever it
//   stands.  u = (x_1 >> 11)·2^-53, v = (x_2 >> 11)·2^-53; if u + v > 1.0 (the fp64 sum) then
//   u = 1.0 − u and v = 1.0 − v.  Per coordinate, point = (a + ab*u) + ac*v — the face region's
//   expression in tri_closest (mesh_tri.h), (u, v) in m3d_mesh_closest's uv convention.  The normal
//   is (cx/len, cy/len, cz/len) of that triangle.
//
// One thread per sample; the search over cum is a bisection of at most 64 steps (the interval
// halves; 26 suffice for F < 2^26); the vertices come from the packed tri9 array mesh.hip keeps.
// A sample writes only its own outputs: no atomics in the sample kernel, n == 0 launches nothing,
// and a sample's bits depend on (mesh, seed, k) alone.
#include <algorithm>
#include <cmath>

#include <hipcub/hipcub.hpp>

#include "m3d_internal.h"
#include "mesh_tri.h"
#include "sampler.h"

namespace m3d {
namespace {

constexpr int kSmpBlock = 256;

// what the build reads back: ord_of(L), then W's pieces
struct SampleInfo {
  unsigned long long lmax;
  unsigned long long nonzero;
};

__device__ __forceinline__ void tri_cross(const double* t9, double c[3]) {
  const double ab[3] = {t9[3] - t9[0], t9[4] - t9[1], t9[5] - t9[2]};
  const double ac[3] = {t9[6] - t9[0], t9[7] - t9[1], t9[8] - t9[2]};
  c[0] = ab[1] * ac[2] - ab[2] * ac[1];
  c[1] = ab[2] * ac[0] - ab[0] * ac[2];
  c[2] = ab[0] * ac[1] - ab[1] * ac[0];
}

// len_f of the contract: 0 for an unusable triangle or a length that is not finite
__device__ __forceinline__ double tri_len(const double* __restrict__ tri9, const uint8_t* __restrict__ ok, int64_t f) {
  if (!ok[f]) return 0.0;
  double c[3];
  tri_cross(tri9 + 9 * f, c);
  const double len = sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]);
  return isfinite(len) ? len : 0.0;
}

__global__ __launch_bounds__(kSmpBlock) void len_max_kernel(const double* __restrict__ tri9,
                                                            const uint8_t* __restrict__ ok, int64_t nf,
                                                            SampleInfo* __restrict__ info) {
  const int64_t f = (int64_t)blockIdx.x * kSmpBlock + threadIdx.x;
  double len = f < nf ? tri_len(tri9, ok, f) : 0.0;
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) len = fmax(len, __shfl_xor(len, o));  // len ≥ 0, never NaN
  if ((threadIdx.x & 63) == 0 && len > 0.0) atomicMax(&info->lmax, (unsigned long long)ord_of(len));
}

__global__ __launch_bounds__(kSmpBlock) void weight_kernel(const double* __restrict__ tri9,
                                                           const uint8_t* __restrict__ ok, int64_t nf, int shift,
                                                           unsigned long long* __restrict__ w,
                                                           SampleInfo* __restrict__ info) {
  const int64_t f = (int64_t)blockIdx.x * kSmpBlock + threadIdx.x;
  unsigned long long wf = 0;
  if (f < nf) {
    wf = (unsigned long long)trunc(ldexp(tri_len(tri9, ok, f), shift));  // < 2^32 by the choice of shift
    w[f] = wf;
  }
  const int nz = __popcll(__ballot(wf != 0));
  if ((threadIdx.x & 63) == 0 && nz != 0) atomicAdd(&info->nonzero, (unsigned long long)nz);
}

struct SampleOut {
  double* point;
  int32_t* tri;
  double* uv;
  double* normal;
};

__global__ __launch_bounds__(kSmpBlock) void sample_kernel(const double* __restrict__ tri9,
                                                           const unsigned long long* __restrict__ cum, int64_t nf,
                                                           unsigned long long W, uint64_t seed, int64_t n,
                                                           SampleOut out) {
  const int64_t k = (int64_t)blockIdx.x * kSmpBlock + threadIdx.x;
  if (k >= n) return;
  const uint64_t base = sample_base(seed, k);
  const uint64_t x0 = splitmix64(base), x1 = splitmix64(base + 1), x2 = splitmix64(base + 2);
  const unsigned long long t = __umul64hi(x0, W);  // < W = cum[nf − 1]
  // the smallest f with cum[f] > t: [lo, hi] always holds it (cum[nf − 1] = W > t)
  int64_t lo = 0, hi = nf - 1;
  for (int it = 0; it < 64 && lo < hi; ++it) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (cum[mid] > t)
      hi = mid;
    else
      lo = mid + 1;
  }
  const int64_t f = lo;
  double u = (double)(x1 >> 11) * 0x1p-53, v = (double)(x2 >> 11) * 0x1p-53;
  if (u + v > 1.0) {
    u = 1.0 - u;
    v = 1.0 - v;
  }
  const double* t9 = tri9 + 9 * f;
  if (out.point != nullptr) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double ab = t9[3 + c] - t9[c], ac = t9[6 + c] - t9[c];
      out.point[3 * k + c] = (t9[c] + ab * u) + ac * v;
    }
  }
  if (out.tri != nullptr) out.tri[k] = (int32_t)f;
  if (out.uv != nullptr) {
    out.uv[2 * k] = u;
    out.uv[2 * k + 1] = v;
  }
  if (out.normal != nullptr) {
    double c[3];
    tri_cross(t9, c);
    const double len = sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]);
    out.normal[3 * k] = c[0] / len;
    out.normal[3 * k + 1] = c[1] / len;
    out.normal[3 * k + 2] = c[2] / len;
  }
}

}  // namespace

hipError_t mesh_sample_build(m3d_ctx* ctx, m3d_mesh* m, hipStream_t st) {
  if (m->sample_built) return hipSuccess;
  if (m->sblock != nullptr) {  // a build that failed half way
    block_release(m->sblock);
    m->sblock = nullptr;
    m->cum = nullptr;
  }
  const int64_t nf = m->nf;
  hipError_t e;
  Carve own;
  own.add(&m->cum, (size_t)nf);
  if ((e = own.alloc(&m->sblock, &m->sblock_bytes, st)) != hipSuccess) return e;
  size_t scan_bytes = 0;
  unsigned long long* w = nullptr;
  unsigned long long* cum = reinterpret_cast<unsigned long long*>(m->cum);
  SampleInfo* info = nullptr;
  char* scan_tmp = nullptr;
  if ((e = hipcub::DeviceScan::InclusiveSum(nullptr, scan_bytes, w, cum, (int)nf, st)) != hipSuccess) return e;
  Carve tmp;
  tmp.add(&info, 1);
  tmp.add(&w, (size_t)nf);
  tmp.add(&scan_tmp, std::max<size_t>(scan_bytes, 1));
  if ((e = ctx->tmp.reserve(tmp.bytes())) != hipSuccess) return e;
  tmp.place(ctx->tmp.base);
  const unsigned blocks = (unsigned)((nf + kSmpBlock - 1) / kSmpBlock);
  SampleInfo h{0ull, 0ull};
  if ((e = hipMemsetAsync(info, 0, sizeof(SampleInfo), st)) != hipSuccess) return e;
  len_max_kernel<<<blocks, kSmpBlock, 0, st>>>(m->tri9, m->ok, nf, info);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if ((e = hipMemcpyAsync(&h, info, sizeof h, hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
  if ((e = hipStreamSynchronize(st)) != hipSuccess) return e;
  m->sample_W = 0;
  m->sample_nonzero = 0;
  if (h.lmax != 0) {  // some triangle has a finite len > 0
    int ex = 0;
    (void)std::frexp(ord_inv(h.lmax), &ex);
    weight_kernel<<<blocks, kSmpBlock, 0, st>>>(m->tri9, m->ok, nf, 32 - ex, w, info);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = hipcub::DeviceScan::InclusiveSum(scan_tmp, scan_bytes, w, cum, (int)nf, st)) != hipSuccess) return e;
    unsigned long long W = 0;
    if ((e = hipMemcpyAsync(&h, info, sizeof h, hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
    if ((e = hipMemcpyAsync(&W, cum + (nf - 1), sizeof W, hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
    if ((e = hipStreamSynchronize(st)) != hipSuccess) return e;
    m->sample_W = W;
    m->sample_nonzero = (int64_t)h.nonzero;
  }
  m->sample_built = true;
  return hipSuccess;
}

hipError_t mesh_sample(const m3d_mesh* m, int64_t n, uint64_t seed, double* points, int32_t* triangle, double* uv,
                       double* normals, hipStream_t st) {
  if (n == 0) return hipSuccess;
  const unsigned blocks = (unsigned)((n + kSmpBlock - 1) / kSmpBlock);
  sample_kernel<<<blocks, kSmpBlock, 0, st>>>(m->tri9, reinterpret_cast<const unsigned long long*>(m->cum), m->nf,
                                              (unsigned long long)m->sample_W, seed, n,
                                              SampleOut{points, triangle, uv, normals});
  return hipGetLastError();
}

}  // namespace m3d
