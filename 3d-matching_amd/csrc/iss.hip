// iss.hip — ISS keypoints on the device: Open3D 0.19 keypoint::ComputeISSKeypoints (the contract is
// in include/m3d.h).
//
// S(i) = {j : d²(i, j) < rs²}, N(i) = {j : d²(i, j) < rn²} (strict, the point itself included):
// the fixed-radius scan of knn_wave.h (wave_scan_box; its contract and exactness argument are
// stated there).
//
//   A. moments   ONE WAVE per point in the cell order of the grid of cell rs, lanes over the
//                candidates of a cell row.  Each lane adds, for its candidates inside, d = pⱼ − pᵢ
//                into nine fp64 sums (Σd, Σd dᵀ) and splitmix64(j) into a 64-bit integer sum; then a
//                fixed xor butterfly.  The sums are centred on the query, so nothing cancels but
//                the mean of the neighbourhood itself.  Written: the nine sums, the signature
//                (count, Σ splitmix64(j) mod 2⁶⁴) and the count.
//   eigen        one THREAD per point: m = S1 / count, C = S2 / count − m mᵀ, Eigen's isZero, the
//                eigenvalues (linalg.h sym3_eigenvalues), the two ratio tests → third[i].  Jacobi
//                is a long chain of dependent fp64 operations; at the end of pass A it occupies a
//                whole wave for one point and took three times this launch, and the
//                nine sums a point stores and reloads are 72 B.
//   B. non-max   one wave per point with third > 0 in the cell order of the grid of cell rn: the
//                neighbours are counted, and a neighbour with a DIFFERENT signature and a larger
//                third ends the scan (the point is no keypoint, whatever its count).
//   then clean.hip's stable compaction of the keep flags.
//
// The order in which a lane meets its candidates is the grid's (a stable sort: a function of the
// points alone) and the butterfly is fixed, so two calls return the same bits.  No workgroup reads
// what another of the same launch writes; integer atomics only (the two tallies).
#include <float.h>

#include <algorithm>
#include <cmath>

#include "m3d_internal.h"
#include "knn_wave.h"
#include "linalg.h"
#include "sampler.h"

namespace m3d {
namespace {

constexpr int kIssBlock = 256;
constexpr int kIssWaves = kIssBlock / kWave;
constexpr int kTallySalient = 0, kTallyCounted = 1, kTallyWords = 2;

// pass A.  sums: n × 9 doubles (Σdx Σdy Σdz, Σdx² Σdxdy Σdxdz Σdy² Σdydz Σdz²)
__global__ __launch_bounds__(kIssBlock) void moments_kernel(const double* __restrict__ xyz64,
                                                            const float4* __restrict__ xyz32, int64_t n, GridDev g,
                                                            float Rf, double r2, float bf,
                                                            double* __restrict__ sums, uint64_t* __restrict__ sig,
                                                            int32_t* __restrict__ count) {
  const int lane = threadIdx.x & 63;
  const int64_t wq = (int64_t)blockIdx.x * kIssWaves + (threadIdx.x >> 6);
  if (wq >= n) return;  // wave-uniform
  const int64_t i = (int64_t)__float_as_int(g.pts[wq].w);
  const double q[3] = {xyz64[3 * i], xyz64[3 * i + 1], xyz64[3 * i + 2]};
  double sx = 0.0, sy = 0.0, sz = 0.0, sxx = 0.0, sxy = 0.0, sxz = 0.0, syy = 0.0, syz = 0.0, szz = 0.0;
  uint64_t h = 0;
  int32_t total = 0;
  wave_scan_box(
      xyz64, q, xyz32[i], g, Rf, r2, bf, lane, [](int32_t) {},
      [&](bool in, int32_t t, double dx, double dy, double dz) {
        if (in) {
          sx += dx, sy += dy, sz += dz;
          sxx += dx * dx, sxy += dx * dy, sxz += dx * dz;
          syy += dy * dy, syz += dy * dz, szz += dz * dz;
          h += splitmix64((uint64_t)(uint32_t)t);  // sampler.h: the per-index term of a set's signature
        }
        total += (int32_t)__popcll(__ballot(in));
        return false;
      });
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) {
    sx += __shfl_xor(sx, o), sy += __shfl_xor(sy, o), sz += __shfl_xor(sz, o);
    sxx += __shfl_xor(sxx, o), sxy += __shfl_xor(sxy, o), sxz += __shfl_xor(sxz, o);
    syy += __shfl_xor(syy, o), syz += __shfl_xor(syz, o), szz += __shfl_xor(szz, o);
    h += __shfl_xor(h, o);
  }
  // every lane holds every sum: lane k stores sum k (selects, not an indexed array)
  const double v = lane == 0 ? sx : lane == 1 ? sy : lane == 2 ? sz : lane == 3 ? sxx : lane == 4 ? sxy
                   : lane == 5 ? sxz : lane == 6 ? syy : lane == 7 ? syz : szz;
  if (lane < 9) sums[9 * i + lane] = v;
  if (lane == 0) {
    sig[i] = h;
    count[i] = total;
  }
}

// third[i] from the stored sums; tally: points with third > 0, points with count ≥ min_neighbors
__global__ __launch_bounds__(kIssBlock) void eigen_kernel(const double* __restrict__ sums,
                                                          const int32_t* __restrict__ count, int64_t n,
                                                          double g21, double g32, int32_t min_neighbors,
                                                          double* __restrict__ third, int32_t* __restrict__ tally) {
  const int64_t i = (int64_t)blockIdx.x * kIssBlock + threadIdx.x;
  const bool live = i < n;
  double out = 0.0;
  bool counted = false;
  if (live) {
    const int32_t cnt = count[i];
    counted = cnt >= min_neighbors;
    if (counted) {
      const double* s = sums + 9 * i;
      const double k = (double)cnt;
      const double mx = s[0] / k, my = s[1] / k, mz = s[2] / k;
      const double cxx = s[3] / k - mx * mx, cxy = s[4] / k - mx * my, cxz = s[5] / k - mx * mz;
      const double cyy = s[6] / k - my * my, cyz = s[7] / k - my * mz, czz = s[8] / k - mz * mz;
      const double tiny = 1e-12;  // Eigen's isZero(): every |C_ab| ≤ 1e-12·1
      const bool zero = fabs(cxx) <= tiny && fabs(cxy) <= tiny && fabs(cxz) <= tiny && fabs(cyy) <= tiny &&
                        fabs(cyz) <= tiny && fabs(czz) <= tiny;
      if (!zero) {
        double lam[3];
        sym3_eigenvalues(cxx, cxy, cxz, cyy, cyz, czz, lam);
        // the divisions as Open3D writes them: a NaN (0 / 0) compares false
        if (lam[1] / lam[2] < g21 && lam[0] / lam[1] < g32) out = lam[0];
      }
    }
    third[i] = out;
  }
  const int32_t ns = (int32_t)__popcll(__ballot(live && out > 0.0));
  const int32_t nc = (int32_t)__popcll(__ballot(counted));
  if ((threadIdx.x & 63) == 0) {
    if (ns) atomicAdd(tally + kTallySalient, ns);
    if (nc) atomicAdd(tally + kTallyCounted, nc);
  }
}

// pass B: keep[i] = third[i] > 0, |N(i)| ≥ min_neighbors and no j ∈ N(i) of another set with a larger third
__global__ __launch_bounds__(kIssBlock) void nonmax_kernel(const double* __restrict__ xyz64,
                                                           const float4* __restrict__ xyz32, int64_t n, GridDev g,
                                                           float Rf, double r2, float bf,
                                                           const double* __restrict__ third,
                                                           const uint64_t* __restrict__ sig,
                                                           const int32_t* __restrict__ count, int32_t min_neighbors,
                                                           uint8_t* __restrict__ keep) {
  const int lane = threadIdx.x & 63;
  const int64_t wq = (int64_t)blockIdx.x * kIssWaves + (threadIdx.x >> 6);
  if (wq >= n) return;  // wave-uniform
  const int64_t i = (int64_t)__float_as_int(g.pts[wq].w);
  const double ti = third[i];
  if (!(ti > 0.0)) {  // wave-uniform
    if (lane == 0) keep[i] = 0;
    return;
  }
  const uint64_t si = sig[i];
  const int32_t ci = count[i];
  const double q[3] = {xyz64[3 * i], xyz64[3 * i + 1], xyz64[3 * i + 2]};
  int32_t total = 0;
  bool beaten = false;  // wave-uniform
  double tt = 0.0;
  bool other = false;
  wave_scan_box(
      xyz64, q, xyz32[i], g, Rf, r2, bf, lane,
      [&](int32_t t) {
        tt = third[t];
        other = sig[t] != si || count[t] != ci;
      },
      [&](bool in, int32_t, double, double, double) {
        total += (int32_t)__popcll(__ballot(in));
        beaten = __ballot(in && other && tt > ti) != 0;  // in: this chunk's pre ran in this lane
        return beaten;
      });
  if (lane == 0) keep[i] = (!beaten && total >= min_neighbors) ? 1 : 0;
}

// the pieces of a call's scratch for n points, placed onto `scratch` (null: the layout's size alone)
struct IssScratch {
  double* sums = nullptr;
  uint64_t* sig = nullptr;
  double* third = nullptr;
  int32_t* count = nullptr;
  uint8_t* keep = nullptr;
  int32_t* tally = nullptr;
  size_t bytes = 0;
  IssScratch(int64_t n, void* scratch) {
    Carve cv;
    cv.add(&sums, 9 * (size_t)n);
    cv.add(&sig, (size_t)n);
    cv.add(&third, (size_t)n);
    cv.add(&count, (size_t)n);
    cv.add(&keep, (size_t)n);
    cv.add(&tally, kTallyWords);
    bytes = cv.bytes();
    if (scratch != nullptr) cv.place(scratch);
  }
};

}  // namespace

size_t iss_scratch_bytes(int64_t n) { return n > 0 ? IssScratch(n, nullptr).bytes : 0; }

// Profiling (m3d_profile_*): pass A under M3D_KERNEL_SCORE, the eigen launch under M3D_KERNEL_LOOP,
// pass B under M3D_KERNEL_NN, the compaction under M3D_KERNEL_KABSCH.
hipError_t iss_keypoints(m3d_ctx* ctx, const m3d_cloud* c, const Grid* gs, const Grid* gn, double rs, double rn,
                         double gamma_21, double gamma_32, int32_t min_neighbors, int32_t* index_out,
                         double* third_out, int32_t* count_out, int64_t tally_out[3], void* scratch,
                         void* clean_scratch, hipStream_t st) {
  const int64_t n = c->n;
  const IssScratch L(n, scratch);
  double* sums = L.sums;
  uint64_t* sig = L.sig;
  double* third = third_out != nullptr ? third_out : L.third;
  int32_t* count = count_out != nullptr ? count_out : L.count;
  uint8_t* keep = L.keep;
  int32_t* tally = L.tally;
  const unsigned per_thread = (unsigned)((n + kIssBlock - 1) / kIssBlock);
  const unsigned per_wave = (unsigned)((n + kIssWaves - 1) / kIssWaves);
  hipError_t e = hipSuccess;
  {
    KTimer t(ctx, M3D_KERNEL_SCORE, st);
    const RadiusScreen s = radius_screen(c, rs);
    moments_kernel<<<per_wave, kIssBlock, 0, st>>>(c->xyz64, c->xyz32, n, gs->dev, s.Rf, s.r2, s.bf, sums, sig, count);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  {
    KTimer t(ctx, M3D_KERNEL_LOOP, st);
    if ((e = hipMemsetAsync(tally, 0, sizeof(int32_t) * kTallyWords, st)) != hipSuccess) return e;
    eigen_kernel<<<per_thread, kIssBlock, 0, st>>>(sums, count, n, gamma_21, gamma_32, min_neighbors, third, tally);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  {
    KTimer t(ctx, M3D_KERNEL_NN, st);
    const RadiusScreen s = radius_screen(c, rn);
    nonmax_kernel<<<per_wave, kIssBlock, 0, st>>>(c->xyz64, c->xyz32, n, gn->dev, s.Rf, s.r2, s.bf, third, sig, count,
                                                  min_neighbors, keep);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  int32_t h[kTallyWords] = {0};
  if ((e = hipMemcpyAsync(h, tally, sizeof h, hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
  int64_t nkey = 0;
  {
    KTimer t(ctx, M3D_KERNEL_KABSCH, st);
    if ((e = select_flagged(keep, n, index_out, &nkey, clean_scratch, st)) != hipSuccess) return e;  // syncs
  }
  tally_out[0] = nkey;
  tally_out[1] = h[kTallySalient];
  tally_out[2] = h[kTallyCounted];
  return hipSuccess;
}

}  // namespace m3d
