// clean.hip — outlier removal on the device: exact unbounded k-NN (KDTreeFlann::SearchKNN for
// every point of a cloud), PointCloud::RemoveStatisticalOutliers and RemoveRadiusOutliers
// (Open3D 0.19 semantics), the kept indices compacted on the device in ascending order.
//
// All arithmetic is fp64 in the project's operation order (-ffp-contract=off), lists in ascending
// (d², index) order.  The scans — the cell-box walk, the fixed-radius scan, the wave-held sorted list
// of the k-NN ladder — and their exactness argument (the fp32 screen, the exact d²) live in
// knn_wave.h, shared with prep.hip, cluster.hip and iss.hip; radius_count_kernel is that header's
// fixed-radius scan written out.
//
// Unbounded k-NN = a radius ladder over uniform grids (knn_ladder).  Level ℓ searches the still
// pending queries on a grid of cell r_ℓ (r₀, then at least doubling) with the hybrid search's rule
// (the k best with strict d² < r²; one wave per query).  A query that holds kk = min(k, n) entries is FINISHED:
// every point it did not take has d² ≥ r² > each entry, or lost the (d², index) compare inside
// the radius, so the entries are its global kk nearest.  The others are appended to the next
// level's list (an integer atomic on a counter; the order of that list changes no result, every
// query writes only its own output row).  Termination: the ladder's last radius is beyond the
// fp32 bounding-box diagonal plus the centring error of two points (ladder_end), so there every
// one of the n points is strictly inside the radius of every query and cnt = kk by construction;
// the host loop is bounded by kMaxLevels on top of that and fails with a message if it is hit.
// r₀ comes from the cloud's density (a probe grid's occupancy, as prep.hip hybrid_fine_radius
// uses it) and only decides the cost, as does the box the grids span (robust_bounds: cut where a
// few far points would stretch it).  The ladder's grids are local to the call: none is cached on
// the cloud, their blocks go back to the block cache once the level that used them has synced.
//
// Reductions (cloud statistics) are fixed-order fp64: 256 consecutive points per block — each
// wave an xor butterfly, the four wave sums in wave order — then one block adds the partials,
// thread t taking t, t + 256, … in increasing order and a fixed LDS tree over the 256 sums.  No
// floating-point atomics, so two runs give the same bits.
#include <float.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include <hipcub/hipcub.hpp>

#include "m3d_internal.h"
#include "knn_wave.h"

namespace m3d {
namespace {

constexpr int kCleanBlock = 256;
constexpr int kMaxLevels = 64;     // host bound of the ladder (ladder radii span ≤ 2^41: see r0 clamp)
constexpr int kProbeMax = 6;       // density probe grids at most
constexpr uint32_t kFewPending = 1024;  // knn_ladder: so few unfinished queries speed the radius up

// One level of the ladder, ONE WAVE per pending query (kk ≤ 64·kS entries in a knn_wave.h
// WaveKnnList).  pend_in null: level 0, wave w takes the point at position w of the
// grid's cell order (neighbouring waves then read the same cell rows).  kMean: the output is the
// query's mean neighbour distance (Σ sqrt(d²) in list order from 0.0, divided by the count)
// instead of the list.
//
// kW = 1: four queries per 256-thread block (level 0: every point, small boxes).  kW > 1 (the
// levels above: few queries, each with a box that grows to the whole cloud): ONE query per block of
// kW waves; wave s takes the chunks s, s + kW, … of every cell row and builds the list of that
// subset, then wave 0 inserts the other waves' entries (sorted, so it stops at the first one not
// below its threshold) into its own.  The kk best of the union of the subsets' kk best are the kk
// best of the box, whichever wave saw them: the result is the single wave's list exactly.
template <int kS, bool kMean, int kW>
__global__ __launch_bounds__(kW == 1 ? kCleanBlock : kW * kWave) void knn_level_kernel(
    const double* __restrict__ xyz64, const float4* __restrict__ xyz32, GridDev g, float Rf, double r2,
    double eabs, int k, int kk, const int32_t* __restrict__ pend_in, int64_t npend,
    int32_t* __restrict__ pend_out, uint32_t* __restrict__ pend_cnt, int32_t* __restrict__ out_idx,
    double* __restrict__ out_d2, int32_t* __restrict__ out_cnt, double* __restrict__ out_avg) {
  constexpr int kWaves = kW == 1 ? kCleanBlock / kWave : kW;  // waves per block
  __shared__ double s_d[kWaves][kWave];
  __shared__ int32_t s_t[kWaves][kWave];
  __shared__ double m_d[kW > 1 ? kW : 1][kW > 1 ? kS * kWave : 1];  // kW > 1: the waves' lists
  __shared__ int32_t m_t[kW > 1 ? kW : 1][kW > 1 ? kS * kWave : 1];
  __shared__ int32_t m_c[kW > 1 ? kW : 1];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t wq = kW == 1 ? (int64_t)blockIdx.x * kWaves + w : (int64_t)blockIdx.x;
  const int sub = kW == 1 ? 0 : w;
  if (wq >= npend) return;  // wave-uniform (kW > 1: block-uniform)
  const int64_t i = pend_in != nullptr ? (int64_t)pend_in[wq] : (int64_t)__float_as_int(g.pts[wq].w);
  const double q[3] = {xyz64[3 * i], xyz64[3 * i + 1], xyz64[3 * i + 2]};
  const float4 qf = xyz32[i];
  WaveKnnList<kS> L;
  L.reset(r2, eabs);
  wave_knn_scan_box(L, xyz64, q, qf, g, Rf, r2, eabs, kk, 64 * sub, 64 * kW, s_d[w], s_t[w]);
  if constexpr (kW > 1) {
    if (w > 0) {
#pragma unroll
      for (int u = 0; u < kS; ++u) {
        const int e = u * 64 + lane;
        if (e < L.cnt) {
          m_d[w][e] = L.D[u];
          m_t[w][e] = L.T[u];
        }
      }
      if (lane == 0) m_c[w] = L.cnt;
    }
    __syncthreads();
    if (w > 0) return;
    for (int ww = 1; ww < kW; ++ww) {
      const int c = __builtin_amdgcn_readfirstlane(m_c[ww]);
      for (int e = 0; e < c; ++e) {
        const double x = readlane_f64(m_d[ww][e], 0);  // the same address in every lane
        const int32_t xt = __builtin_amdgcn_readfirstlane(m_t[ww][e]);
        if (!L.accepts(x, xt, kk)) break;  // sorted: the rest is not below the threshold either
        L.insert(x, xt, kk);
      }
    }
  }
  if (L.cnt < kk) {  // fewer than kk points strictly inside the radius: the next level's
    if (lane == 0) pend_out[atomicAdd(pend_cnt, 1u)] = (int32_t)i;
    return;
  }
  if constexpr (kMean) {
    double acc = 0.0;
#pragma unroll
    for (int u = 0; u < kS; ++u) {
      const double s = sqrt(L.D[u]);
      const int m = L.cnt - u * 64 < 64 ? L.cnt - u * 64 : 64;
      for (int l = 0; l < m; ++l) acc += readlane_f64(s, l);
    }
    if (lane == 0) out_avg[i] = acc / (double)L.cnt;
  } else {
#pragma unroll
    for (int u = 0; u < kS; ++u) {
      const int e = u * 64 + lane;
      if (e < k) {
        out_idx[i * k + e] = e < L.cnt ? L.T[u] : -1;
        out_d2[i * k + e] = e < L.cnt ? L.D[u] : INFINITY;
      }
    }
    if (lane == 0) out_cnt[i] = L.cnt;
  }
}

// count[i] = #{j : d²(i, j) < r²} on the grid of cell r, one wave per point in the grid's cell
// order; keep[i] = count > nb_points.  kFull: the whole box is counted and count_out written;
// otherwise the wave leaves the box once the count exceeds nb_points.
template <bool kFull>
__global__ __launch_bounds__(kCleanBlock) void radius_count_kernel(
    const double* __restrict__ xyz64, const float4* __restrict__ xyz32, int64_t n, GridDev g, float Rf,
    double r2, float bf, int32_t nb_points, int32_t* __restrict__ count_out, uint8_t* __restrict__ keep) {
  const int lane = threadIdx.x & 63;
  const int64_t wq = (int64_t)blockIdx.x * (kCleanBlock / kWave) + (threadIdx.x >> 6);
  if (wq >= n) return;  // wave-uniform
  const int64_t i = (int64_t)__float_as_int(g.pts[wq].w);
  const double q[3] = {xyz64[3 * i], xyz64[3 * i + 1], xyz64[3 * i + 2]};
  const float4 qf = xyz32[i];
  // knn_wave.h wave_scan_box's walk, screen and test written out: through the shared scan this
  // kernel's full count measured 0.2 % above the parent's range at large radii (EXPERIMENTS §R24)
  const int x0 = grid_coord(qf.x - Rf, g.o[0], g.inv_h, g.n[0]);
  const int x1 = grid_coord(qf.x + Rf, g.o[0], g.inv_h, g.n[0]);
  const int y0 = grid_coord(qf.y - Rf, g.o[1], g.inv_h, g.n[1]);
  const int y1 = grid_coord(qf.y + Rf, g.o[1], g.inv_h, g.n[1]);
  const int z0 = grid_coord(qf.z - Rf, g.o[2], g.inv_h, g.n[2]);
  const int z1 = grid_coord(qf.z + Rf, g.o[2], g.inv_h, g.n[2]);
  int32_t total = 0;
  bool stop = false;  // wave-uniform
  for (int cz = z0; cz <= z1 && !stop; ++cz)
    for (int cy = y0; cy <= y1 && !stop; ++cy) {
      const int64_t row = ((int64_t)cz * g.n[1] + cy) * g.n[0];
      const int32_t j0 = g.start[row + x0], j1 = g.start[row + x1 + 1];
      for (int32_t jb = j0; jb < j1 && !stop; jb += 64) {
        const int32_t j = jb + lane;
        bool in = false;
        if (j < j1) {
          const float4 tp = g.pts[j];
          const float fx = qf.x - tp.x, fy = qf.y - tp.y, fz = qf.z - tp.z;
          if ((fx * fx + fy * fy) + fz * fz <= bf)
            in = d2_exact(xyz64 + 3 * (int64_t)__float_as_int(tp.w), q) < r2;
        }
        total += (int32_t)__popcll(__ballot(in));
        if (!kFull && total > nb_points) stop = true;
      }
    }
  if (lane == 0) {
    keep[i] = total > nb_points ? 1 : 0;
    if (kFull) count_out[i] = total;
  }
}

// Per-axis histograms of the centred fp32 points over [lo, lo + kHistBins / s) (robust_bounds):
// LDS counts per block, integer atomics only; a point outside the range counts in the edge bin.
constexpr int kHistBins = 1024;
__global__ __launch_bounds__(kCleanBlock) void axis_hist_kernel(const float4* __restrict__ xyz32, int64_t n,
                                                                float lo0, float lo1, float lo2, float s0,
                                                                float s1, float s2, uint32_t* __restrict__ hist) {
  __shared__ uint32_t h[3 * kHistBins];
  for (int b = threadIdx.x; b < 3 * kHistBins; b += kCleanBlock) h[b] = 0;
  __syncthreads();
  auto bin = [](float x, float lo, float s) {
    const float f = fminf(fmaxf((x - lo) * s, 0.0f), (float)(kHistBins - 1));
    return (int)f;
  };
  for (int64_t i = (int64_t)blockIdx.x * kCleanBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kCleanBlock) {
    const float4 v = xyz32[i];
    atomicAdd(&h[bin(v.x, lo0, s0)], 1u);
    atomicAdd(&h[kHistBins + bin(v.y, lo1, s1)], 1u);
    atomicAdd(&h[2 * kHistBins + bin(v.z, lo2, s2)], 1u);
  }
  __syncthreads();
  for (int b = threadIdx.x; b < 3 * kHistBins; b += kCleanBlock)
    if (h[b] != 0) atomicAdd(&hist[b], h[b]);
}

// ------------------------------------------------------------------------------- statistics
// stats (device, kStatWords doubles): [0] valid, [1] mean, [2] std_dev, [3] threshold
constexpr int kStatWords = 4;

// level 1 of a fixed-order sum: the block's 256 values v → partials[blockIdx.x] (each wave an xor
// butterfly, the four wave sums in wave order)
__device__ __forceinline__ void block_sum_partial(double v, double* __restrict__ partials) {
  __shared__ double red[kCleanBlock / kWave];
  const double t = wave_sum(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = t;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (int k = 0; k < kCleanBlock / kWave; ++k) s += red[k];
    partials[blockIdx.x] = s;
  }
}

// level 2, one block: thread t adds partials t, t + 256, … in increasing order, then a fixed LDS
// tree over the 256 sums; thread 0 hands the total to done(sum)
template <class Done>
__device__ __forceinline__ void block_sum_final(const double* __restrict__ partials, int64_t nb, Done&& done) {
  __shared__ double red[kCleanBlock];
  double v = 0.0;
  for (int64_t b = threadIdx.x; b < nb; b += kCleanBlock) v += partials[b];
  red[threadIdx.x] = v;
  __syncthreads();
  for (int w = kCleanBlock / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) done(red[0]);
}

// pass 0: Σ avg over avg > 0; pass 1: Σ (avg − mean)² over avg > 0 (mean = stats[1])
__global__ __launch_bounds__(kCleanBlock) void stat_partial_kernel(const double* __restrict__ avg, int64_t n,
                                                                   int pass, const double* __restrict__ stats,
                                                                   double* __restrict__ partials) {
  const int64_t i = (int64_t)blockIdx.x * kCleanBlock + threadIdx.x;
  double v = 0.0;
  if (i < n) {
    const double a = avg[i];
    if (a > 0.0) {
      if (pass == 0) {
        v = a;
      } else {
        const double dm = a - stats[1];
        v = dm * dm;
      }
    }
  }
  block_sum_partial(v, partials);
}

__global__ __launch_bounds__(kCleanBlock) void stat_final_kernel(const double* __restrict__ partials, int64_t nb,
                                                                 int64_t n, int pass, double std_ratio,
                                                                 double* __restrict__ stats) {
  block_sum_final(partials, nb, [&](const double& sum) {
    const double valid = (double)n;  // every point's list holds at least the point itself
    if (pass == 0) {
      stats[0] = valid;
      stats[1] = sum / valid;
    } else {
      const double sd = sqrt(sum / (valid - 1.0));  // n = 1: 0 / 0 = NaN, nothing is kept
      stats[2] = sd;
      stats[3] = stats[1] + std_ratio * sd;
    }
  });
}

__global__ __launch_bounds__(kCleanBlock) void stat_flag_kernel(const double* __restrict__ avg, int64_t n,
                                                                const double* __restrict__ stats,
                                                                uint8_t* __restrict__ keep) {
  const int64_t i = (int64_t)blockIdx.x * kCleanBlock + threadIdx.x;
  if (i >= n) return;
  const double a = avg[i];
  keep[i] = (a > 0.0 && a < stats[3]) ? 1 : 0;
}

// Σ 2·avg over ALL n points (model_resolution: avg at k = 2 is half the distance to the nearest other
// point, doubling it is exact; a duplicate's 0 is a term like any other), the blocks of
// stat_partial_kernel; then res = the partials' fixed-order sum / n → stats[0]
__global__ __launch_bounds__(kCleanBlock) void res_partial_kernel(const double* __restrict__ avg, int64_t n,
                                                                  double* __restrict__ partials) {
  const int64_t i = (int64_t)blockIdx.x * kCleanBlock + threadIdx.x;
  block_sum_partial(i < n ? 2.0 * avg[i] : 0.0, partials);
}

__global__ __launch_bounds__(kCleanBlock) void res_final_kernel(const double* __restrict__ partials, int64_t nb,
                                                                int64_t n, double* __restrict__ stats) {
  block_sum_final(partials, nb, [&](const double& sum) { stats[0] = sum / (double)n; });
}

// ------------------------------------------------------------------------------- host side
// the pieces of a call's scratch for n points, placed onto `scratch` (null: the layout's size alone)
struct CleanScratch {
  int32_t *pend_a = nullptr, *pend_b = nullptr;
  uint32_t* cnt = nullptr;
  double* avg = nullptr;
  uint8_t* keep = nullptr;
  double *partials = nullptr, *stats = nullptr;
  int32_t* nsel = nullptr;
  char* tmp = nullptr;
  size_t tmp_bytes = 0, bytes = 0;
  CleanScratch(int64_t n, void* scratch) {
    size_t tb = 0;
    hipcub::DeviceSelect::Flagged(nullptr, tb, hipcub::CountingInputIterator<int32_t>(0), (uint8_t*)nullptr,
                                  (int32_t*)nullptr, (int32_t*)nullptr, (int)n, (hipStream_t)0);
    tmp_bytes = std::max<size_t>(tb, 1);
    Carve cv;
    cv.add(&pend_a, (size_t)n);
    cv.add(&pend_b, (size_t)n);
    cv.add(&cnt, kMaxLevels);
    cv.add(&avg, (size_t)n);
    cv.add(&keep, (size_t)n);
    cv.add(&partials, (size_t)((n + kCleanBlock - 1) / kCleanBlock));
    cv.add(&stats, kStatWords);
    cv.add(&nsel, 1);
    cv.add(&tmp, tmp_bytes);
    bytes = cv.bytes();
    if (scratch != nullptr) cv.place(scratch);
  }
};

// a grid of the call itself (not cached on the cloud); released after the stream has synced
hipError_t local_grid(m3d_ctx* ctx, const m3d_cloud* c, const float* lohi, double cell, hipStream_t st, Grid* g) {
  return grid_build(c->xyz32, c->n, cell, st, g, &ctx->tmp, lohi);
}
void local_grid_free(m3d_ctx* ctx, Grid* g) {
  ReleaseScope rs(ctx, ctx->id);  // the stream is idle: the block is reusable without a device sync
  grid_free(g);
}

// M3D_KNN_TRACE=1: one line per ladder on stderr (radius, queries in, queries left per level);
// read at every call so a tool can switch it on for one (tools/bench_clean.py)
bool knn_trace() {
  const char* e = std::getenv("M3D_KNN_TRACE");
  return e != nullptr && e[0] != '\0' && e[0] != '0';
}

// the first radius at which every query finishes by construction: beyond the largest fp64
// distance of two points, itself at most the fp32 box diagonal plus both points' centring error
double ladder_end(const m3d_cloud* c) {
  double diag = 3.4641016151377544 * c->rmax;  // 2·√3·rmax: without bounds
  if (c->has_bounds) {
    double s = 0.0;
    for (int a = 0; a < 3; ++a) {
      const double e = (double)c->hi[a] - (double)c->lo[a];
      s += e * e;
    }
    diag = std::sqrt(s);
  }
  return (diag + pair_eabs(c)) * (1.0 + 1e-6);
}

// The box the call's grids span.  A grid spans its bounds with at most 2²⁵ cells, so a few points far
// outside the scan (a scanner glitch at 10³ object sizes) would force cells so large that the
// whole scan sits in a handful of them and level 0 compares every point with every other.  The
// cell coordinate clamps to the grid (the one expression of nnkey.h) for points and for a query's box ends
// alike and stays monotone, so a grid over ANY box visits every point within the radius: points
// outside the box simply share its edge cells.  Per axis the box is cut where at most n / 256
// points lie beyond (1024-bin histograms, one bin of margin), and only if that halves an axis;
// repeated on the new box (a stray at 10⁶ object sizes needs two rounds), at most kRobustRounds.
constexpr int kRobustRounds = 4;
hipError_t robust_bounds(m3d_ctx* ctx, const m3d_cloud* c, hipStream_t st, float lohi[6], int* rounds) {
  *rounds = 0;
  const int64_t n = c->n;
  const uint64_t tail = (uint64_t)(n / 256);
  std::vector<uint32_t> h(3 * kHistBins);
  for (int it = 0; it < kRobustRounds; ++it) {
    float sc[3];
    double binw[3];
    for (int a = 0; a < 3; ++a) {
      const double ext = (double)lohi[3 + a] - (double)lohi[a];
      binw[a] = ext > 0.0 && std::isfinite(ext) ? ext / kHistBins : 0.0;
      sc[a] = binw[a] > 0.0 ? (float)(1.0 / binw[a]) : 0.0f;
      if (!std::isfinite(sc[a])) sc[a] = 0.0f, binw[a] = 0.0;
    }
    hipError_t e = ctx->tmp.reserve(sizeof(uint32_t) * 3 * kHistBins);
    if (e != hipSuccess) return e;
    uint32_t* hist = reinterpret_cast<uint32_t*>(ctx->tmp.base);
    if ((e = hipMemsetAsync(hist, 0, sizeof(uint32_t) * 3 * kHistBins, st)) != hipSuccess) return e;
    const unsigned blocks = (unsigned)std::min<int64_t>(1024, (n + kCleanBlock - 1) / kCleanBlock);
    axis_hist_kernel<<<blocks, kCleanBlock, 0, st>>>(c->xyz32, n, lohi[0], lohi[1], lohi[2], sc[0], sc[1], sc[2], hist);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = hipMemcpyAsync(h.data(), hist, sizeof(uint32_t) * 3 * kHistBins, hipMemcpyDeviceToHost, st)) != hipSuccess)
      return e;
    if ((e = hipStreamSynchronize(st)) != hipSuccess) return e;
    float nl[6];
    bool shrunk = false;
    for (int a = 0; a < 3; ++a) {
      nl[a] = lohi[a];
      nl[3 + a] = lohi[3 + a];
      if (binw[a] <= 0.0) continue;
      const uint32_t* ha = h.data() + a * kHistBins;
      int lo_bin = 0, hi_bin = kHistBins - 1;
      uint64_t acc = 0;
      for (; lo_bin < kHistBins - 1 && acc + ha[lo_bin] <= tail; ++lo_bin) acc += ha[lo_bin];
      acc = 0;
      for (; hi_bin > lo_bin && acc + ha[hi_bin] <= tail; --hi_bin) acc += ha[hi_bin];
      const double lo_new = std::max((double)lohi[a], (double)lohi[a] + (lo_bin - 1) * binw[a]);
      const double hi_new = std::min((double)lohi[3 + a], (double)lohi[a] + (hi_bin + 2) * binw[a]);
      if (hi_new - lo_new < 0.5 * ((double)lohi[3 + a] - (double)lohi[a])) {
        nl[a] = (float)lo_new;
        nl[3 + a] = (float)hi_new;
        shrunk = true;
      }
    }
    if (!shrunk) break;
    for (int a = 0; a < 6; ++a) lohi[a] = nl[a];
    ++*rounds;
  }
  return hipSuccess;
}

// r₀ from the cloud's density: a probe grid of cell ≈ extent / 64, refined (cell / 4) while an
// occupied cell holds far more points than a list needs or coarsened (cell · 4) while the cells
// hold hardly more than one point each (a small cloud).  A first probe that is far too dense is the
// sign of bounds stretched by far strays: robust_bounds then cuts the box (lohi, used by every
// grid of the call) and the probe starts again.  With m points per occupied cell of size h, a
// scanned surface has ≈ 8 m (ρ / h)² points within ρ (prep.hip hybrid_fine_radius), so
// ρ = h·√(kk / 2m) expects ≈ 4 kk.  Any positive r₀, and any box, gives the same lists.
hipError_t ladder_r0(m3d_ctx* ctx, const m3d_cloud* c, int kk, double end, hipStream_t st, float* lohi,
                     double* r0, int* probes, int* rounds) {
  auto extent = [&]() {
    double ext = 0.0;
    if (lohi != nullptr)
      for (int a = 0; a < 3; ++a) ext = std::max(ext, (double)lohi[3 + a] - (double)lohi[a]);
    else
      ext = 2.0 * c->rmax;
    return ext;
  };
  double ext = extent();
  double r = 0.0;
  *probes = 0;
  *rounds = 0;
  if (ext > 0.0 && std::isfinite(ext)) {
    double cell = ext / 64.0;
    int dir = 0;  // −1: refining, +1: coarsening (never both: the probe cannot oscillate)
    bool cut = lohi == nullptr;  // robust_bounds done (or no bounds to cut)
    for (int it = 0; it < kProbeMax; ++it) {
      Grid g;
      hipError_t e = local_grid(ctx, c, lohi, cell, st, &g);
      if (e == hipSuccess) e = grid_occupancy(&g, &ctx->tmp, st);  // one sync
      const double m = g.n_occ > 0 ? (double)c->n / (double)g.n_occ : (double)c->n;
      const double h = g.cell;
      local_grid_free(ctx, &g);
      if (e != hipSuccess) return e;
      ++*probes;
      r = h * std::sqrt(0.5 * (double)kk / m);
      if (m > 8.0 * (double)kk && !cut) {
        cut = true;
        if ((e = robust_bounds(ctx, c, st, lohi, rounds)) != hipSuccess) return e;
        if (*rounds > 0) {  // a smaller box: probe it from the start
          ext = extent();
          if (!(ext > 0.0)) break;
          cell = ext / 64.0;
          continue;
        }
      }
      if (h > cell * 1.01) break;  // the grid hit its cell budget and chose a larger cell
      if (m > 8.0 * (double)kk && dir <= 0) {  // far more points per cell than a list needs
        dir = -1;
        cell *= 0.25;
      } else if (m < 4.0 && dir >= 0 && (double)c->n >= 4.0) {  // nearly one point per cell: the
        dir = 1;                                                 // occupancy says nothing of density
        cell *= 4.0;
      } else {
        break;
      }
    }
  }
  // not below the fp32 resolution of the frame, nor so small that the ladder could not reach its
  // end within kMaxLevels doublings
  r = std::max(r, 4.0 * pair_eabs(c));
  r = std::max(r, end * 0x1p-40);
  if (!(r > 0.0) || !std::isfinite(r)) r = 1.0;
  *r0 = r;
  return hipSuccess;
}

constexpr int kTailWaves = 16;  // waves per query above level 0 (knn_level_kernel kW)

template <bool kMean>
hipError_t launch_level(const m3d_cloud* c, const Grid& g, double radius, int k, int kk, const int32_t* pend_in,
                        int64_t npend, int32_t* pend_out, uint32_t* pend_cnt, int32_t* idx, double* d2,
                        int32_t* cnt, double* avg, hipStream_t st) {
  const float Rf = box_half_width(c, radius);
  const double eabs = pair_eabs(c), r2 = radius * radius;
  const int kS = kk <= 64 ? 1 : (kk <= 128 ? 2 : 4);
#define M3D_KNN_LEVEL(S, W, blocks, threads)                                                                  \
  knn_level_kernel<S, kMean, W><<<(blocks), (threads), 0, st>>>(c->xyz64, c->xyz32, g.dev, Rf, r2, eabs, k, kk, \
                                                                pend_in, npend, pend_out, pend_cnt, idx, d2, cnt, avg)
  if (pend_in == nullptr) {  // level 0: every point, four per block
    const unsigned blocks = (unsigned)((npend + 3) / 4);
    if (kS == 1)
      M3D_KNN_LEVEL(1, 1, blocks, kCleanBlock);
    else if (kS == 2)
      M3D_KNN_LEVEL(2, 1, blocks, kCleanBlock);
    else
      M3D_KNN_LEVEL(4, 1, blocks, kCleanBlock);
  } else {  // the pending queries of the levels above: one per block of kTailWaves waves
    const unsigned blocks = (unsigned)npend;
    if (kS == 1)
      M3D_KNN_LEVEL(1, kTailWaves, blocks, kTailWaves * kWave);
    else if (kS == 2)
      M3D_KNN_LEVEL(2, kTailWaves, blocks, kTailWaves * kWave);
    else
      M3D_KNN_LEVEL(4, kTailWaves, blocks, kTailWaves * kWave);
  }
#undef M3D_KNN_LEVEL
  return hipGetLastError();
}

// the ladder: lists (idx, d2, cnt) or, with avg, the mean neighbour distances.  n ≥ 1,
// 1 ≤ k ≤ 256.  Returns after the last level has synced.
hipError_t knn_ladder(m3d_ctx* ctx, const m3d_cloud* c, int k, int32_t* idx, double* d2, int32_t* cnt,
                      double* avg, const CleanScratch& L, hipStream_t st, std::string* why) {
  const int64_t n = c->n;
  const int kk = (int)std::min<int64_t>(k, n);
  int32_t* pend[2] = {L.pend_a, L.pend_b};
  uint32_t* pcnt = L.cnt;
  const double end = ladder_end(c);
  float box[6];  // the box every grid of this call spans (the cloud's bounds, cut by robust_bounds)
  for (int a = 0; a < 3; ++a) {
    box[a] = c->lo[a];
    box[3 + a] = c->hi[a];
  }
  float* lohi = c->has_bounds ? box : nullptr;
  double r0 = 0.0;
  int probes = 0, rounds = 0;
  hipError_t e = ladder_r0(ctx, c, kk, end, st, lohi, &r0, &probes, &rounds);
  if (e != hipSuccess) return e;
  if ((e = hipMemsetAsync(pcnt, 0, sizeof(uint32_t) * kMaxLevels, st)) != hipSuccess) return e;
  int64_t npend = n;
  double radius = r0;
  const bool tr = knn_trace();
  std::string trace;
  double step = 2.0;
  int level = 0;
  for (; level < kMaxLevels && npend > 0; ++level) {
    const bool last = radius > end;  // every query finishes at this radius
    Grid g;
    e = local_grid(ctx, c, lohi, radius, st, &g);
    if (e == hipSuccess) {
      const int32_t* in = level == 0 ? nullptr : pend[(level - 1) & 1];
      e = avg != nullptr ? launch_level<true>(c, g, radius, k, kk, in, npend, pend[level & 1], pcnt + level, idx,
                                              d2, cnt, avg, st)
                         : launch_level<false>(c, g, radius, k, kk, in, npend, pend[level & 1], pcnt + level, idx,
                                               d2, cnt, avg, st);
    }
    uint32_t left = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(&left, pcnt + level, sizeof(left), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    local_grid_free(ctx, &g);
    if (e != hipSuccess) return e;
    if (tr) {
      char b[96];
      std::snprintf(b, sizeof b, " L%d r=%.6g in=%lld left=%u;", level, radius, (long long)npend, left);
      trace += b;
    }
    if (last && left != 0) {
      *why = "k-NN ladder: queries left pending at a radius beyond the cloud's extent";
      return hipErrorUnknown;
    }
    // the next radius: twice this one; while a FEW queries (≤ kFewPending) all stay pending the
    // factor itself doubles (4, 8, …: a handful of points far outside the cloud would otherwise pay
    // a grid build and a sync per doubling), back to 2 once any finishes.  The first radius past
    // `end` is the last: a step across it stops just beyond it.  Any increasing radii give the
    // same lists; at least doubling keeps the level bound.
    step = ((int64_t)left == npend && left <= kFewPending) ? std::min(2.0 * step, 1024.0) : 2.0;
    npend = (int64_t)left;
    const double next = radius * step;
    radius = (radius <= end && next > end) ? end * (1.0 + 1e-3) : next;
  }
  if (tr)
    std::fprintf(stderr, "m3d knn ladder: n=%lld k=%d probes=%d box_cuts=%d levels=%d%s\n", (long long)n, k, probes,
                 rounds, level, trace.c_str());
  if (npend > 0) {
    *why = "k-NN ladder: level bound reached with queries pending";
    return hipErrorUnknown;
  }
  return hipSuccess;
}

// keep flags → ascending kept indices (a stable select over 0 .. n − 1) and their number
hipError_t select_kept(const uint8_t* keep, int64_t n, int32_t* index_out, int64_t* n_out, const CleanScratch& L,
                       hipStream_t st) {
  int32_t* nsel = L.nsel;
  size_t tb = L.tmp_bytes;
  hipError_t e = hipcub::DeviceSelect::Flagged(L.tmp, tb, hipcub::CountingInputIterator<int32_t>(0), keep,
                                               index_out, nsel, (int)n, st);
  int32_t h = 0;
  if (e == hipSuccess) e = hipMemcpyAsync(&h, nsel, sizeof(h), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  *n_out = h;
  return e;
}

}  // namespace

size_t clean_scratch_bytes(int64_t n) { return n > 0 ? CleanScratch(n, nullptr).bytes : 0; }

hipError_t knn_search(m3d_ctx* ctx, const m3d_cloud* c, int k, int32_t* idx, double* d2, int32_t* cnt,
                      void* scratch, hipStream_t st, std::string* why) {
  if (c->n == 0) return hipSuccess;
  return knn_ladder(ctx, c, k, idx, d2, cnt, nullptr, CleanScratch(c->n, scratch), st, why);
}

hipError_t statistical_outliers(m3d_ctx* ctx, const m3d_cloud* c, int k, double std_ratio, int32_t* index_out,
                                int64_t* n_out, double stats_out[4], double* avg_out, void* scratch,
                                hipStream_t st, std::string* why) {
  const int64_t n = c->n;
  const CleanScratch L(n, scratch);
  double* avg = avg_out != nullptr ? avg_out : L.avg;
  hipError_t e = knn_ladder(ctx, c, k, nullptr, nullptr, nullptr, avg, L, st, why);
  if (e != hipSuccess) return e;
  double *partials = L.partials, *stats = L.stats;
  uint8_t* keep = L.keep;
  const unsigned nb = (unsigned)((n + kCleanBlock - 1) / kCleanBlock);
  for (int pass = 0; pass < 2; ++pass) {
    stat_partial_kernel<<<nb, kCleanBlock, 0, st>>>(avg, n, pass, stats, partials);
    stat_final_kernel<<<1, kCleanBlock, 0, st>>>(partials, (int64_t)nb, n, pass, std_ratio, stats);
  }
  stat_flag_kernel<<<nb, kCleanBlock, 0, st>>>(avg, n, stats, keep);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if ((e = hipMemcpyAsync(stats_out, stats, sizeof(double) * kStatWords, hipMemcpyDeviceToHost, st)) != hipSuccess)
    return e;
  return select_kept(keep, n, index_out, n_out, L, st);  // syncs: stats_out is complete too
}

hipError_t model_resolution(m3d_ctx* ctx, const m3d_cloud* c, double* res_out, void* scratch, hipStream_t st,
                            std::string* why) {
  const int64_t n = c->n;
  const CleanScratch L(n, scratch);
  double *avg = L.avg, *partials = L.partials, *stats = L.stats;
  hipError_t e = knn_ladder(ctx, c, 2, nullptr, nullptr, nullptr, avg, L, st, why);
  if (e != hipSuccess) return e;
  const unsigned nb = (unsigned)((n + kCleanBlock - 1) / kCleanBlock);
  res_partial_kernel<<<nb, kCleanBlock, 0, st>>>(avg, n, partials);
  res_final_kernel<<<1, kCleanBlock, 0, st>>>(partials, (int64_t)nb, n, stats);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if ((e = hipMemcpyAsync(res_out, stats, sizeof(double), hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
  return hipStreamSynchronize(st);
}

hipError_t select_flagged(const uint8_t* keep, int64_t n, int32_t* index_out, int64_t* n_out, void* scratch,
                          hipStream_t st) {
  return select_kept(keep, n, index_out, n_out, CleanScratch(n, scratch), st);
}

hipError_t radius_flags(const m3d_cloud* c, const Grid* g, int32_t nb_points, double radius, int32_t* count_out,
                        uint8_t* keep, hipStream_t st) {
  const int64_t n = c->n;
  const RadiusScreen s = radius_screen(c, radius);
  const unsigned blocks = (unsigned)((n + 3) / 4);
  if (count_out != nullptr)
    radius_count_kernel<true><<<blocks, kCleanBlock, 0, st>>>(c->xyz64, c->xyz32, n, g->dev, s.Rf, s.r2, s.bf,
                                                             nb_points, count_out, keep);
  else
    radius_count_kernel<false><<<blocks, kCleanBlock, 0, st>>>(c->xyz64, c->xyz32, n, g->dev, s.Rf, s.r2, s.bf,
                                                              nb_points, nullptr, keep);
  return hipGetLastError();
}

hipError_t radius_outliers(const m3d_cloud* c, const Grid* g, int32_t nb_points, double radius,
                           int32_t* index_out, int64_t* n_out, int32_t* count_out, void* scratch,
                           hipStream_t st) {
  const int64_t n = c->n;
  const CleanScratch L(n, scratch);
  hipError_t e = radius_flags(c, g, nb_points, radius, count_out, L.keep, st);
  if (e != hipSuccess) return e;
  return select_kept(L.keep, n, index_out, n_out, L, st);
}

}  // namespace m3d
