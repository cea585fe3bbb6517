// plane.hip — plane segmentation on the device: PointCloud::SegmentPlane (Open3D 0.19 semantics,
// restated in include/m3d.h and tests/plane_restatement.py) and the scoring of given planes.
//
// All arithmetic is fp64 on the cloud's original coordinates in the project's operation order
// (-ffp-contract=off): dist = |((a·x + b·y) + c·z) + d|, an inlier has dist < thr (strict).
//
// A batch of the loop is four launches, none of which the host waits for:
//   fit     one hypothesis per thread: its sample (the caller's, or the counter sampler), its
//           plane, its zero-plane flag
//   score   THE HOT PATH.  One hypothesis per LANE, its plane in eight VGPRs; a wave walks one
//           chunk of kPlaneChunk consecutive points, whose coordinates are the same for all 64
//           lanes and arrive through uniform (scalar) loads — 24 B per point per wave, no LDS, no
//           cross-lane operation.  Each lane keeps a private count and err; err is the
//           sequential sum of dist² in point order inside the chunk (a masked add of +0.0 for an
//           outlier leaves the bits alone).  Per (chunk, hypothesis) partials go to scratch.
//   reduce  per hypothesis the chunk partials in a fixed order (icp.hip reduce_kernel's scheme:
//           32 groups, group g adds chunks g, g + 32, … in increasing order, then the 32 group
//           sums in group order).  The chunk size and this order depend on n alone, so a plane's
//           err bits are the same for every H, every batch and both entry points.
//   scan    one wave applies the sequential best / break rule to the batch's rows, 64 rows per
//           step with ballots (a record change or the stop is the first set bit), and keeps the
//           state; a stop sets `done`, which every later launch reads first.
// The host enqueues batches in growing groups (1, 2, 4, …) and reads `done` between groups, as
// m3d_icp_run does.  After the loop: inlier flags + a stable select (ascending indices), then the
// refit — centroid and six sums over the inliers, each a fixed-order reduction (256 consecutive
// inliers per block: wave butterflies, the four wave sums in wave order; then one block adds the
// partials, thread t taking t, t + 256, … and a fixed LDS tree), a one-thread tail for the
// determinant formula.  No floating-point atomics anywhere: two runs give the same bits.
#include <algorithm>
#include <cmath>

#include <hipcub/hipcub.hpp>

#include "m3d_internal.h"
#include "sampler.h"

namespace m3d {
namespace {

constexpr int kPlaneBlock = 256;
constexpr int kScoreUnroll = 8;      // points per scalar-load group of the score kernel
constexpr int kReduceGroupsP = 32;   // reduce: groups of chunks
constexpr int kReduceHyps = 8;       // reduce: hypotheses per block
constexpr int64_t kPartialBudget = (int64_t)1 << 24;  // (chunk, hypothesis) partials per launch
constexpr int kMaxSample = 32;

struct PlaneState {
  double best_plane[4];
  double plane[4];     // the refit
  double centroid[3];  // of the inliers (refit pass 0)
  double best_rmse;
  double break_it;
  int64_t best_count, best_index, evaluated, iterations;
  int32_t done, bad;
};

// GetPlaneFromPoints' tail: centroid c, q = Σ (xx, xy, xz, yy, yz, zz) of r = p − c
__device__ void plane_from_moments(const double c[3], const double q[6], double pl[4]) {
  const double xx = q[0], xy = q[1], xz = q[2], yy = q[3], yz = q[4], zz = q[5];
  const double det_x = yy * zz - yz * yz;
  const double det_y = xx * zz - xz * xz;
  const double det_z = xx * yy - xy * xy;
  double a, b, e;
  if (det_x > det_y && det_x > det_z) {
    a = det_x, b = xz * yz - xy * zz, e = xy * yz - xz * yy;
  } else if (det_y > det_z) {
    a = xz * yz - xy * zz, b = det_y, e = xy * xz - yz * xx;
  } else {
    a = xy * yz - xz * yy, b = xy * xz - yz * xx, e = det_z;
  }
  const double norm = sqrt((a * a + b * b) + e * e);
  if (norm == 0.0) {
    pl[0] = pl[1] = pl[2] = pl[3] = 0.0;
    return;
  }
  a /= norm, b /= norm, e /= norm;
  pl[0] = a, pl[1] = b, pl[2] = e;
  pl[3] = -((a * c[0] + b * c[1]) + e * c[2]);
}

// the plane of a sample of m in-range indices
__device__ void plane_of_sample(const double* __restrict__ xyz64, const int32_t* id, int m, double pl[4]) {
  if (m == 3) {
    const double* p0 = xyz64 + 3 * (int64_t)id[0];
    const double* p1 = xyz64 + 3 * (int64_t)id[1];
    const double* p2 = xyz64 + 3 * (int64_t)id[2];
    const double x0 = p0[0], y0 = p0[1], z0 = p0[2];
    const double ax = p1[0] - x0, ay = p1[1] - y0, az = p1[2] - z0;
    const double bx = p2[0] - x0, by = p2[1] - y0, bz = p2[2] - z0;
    double a = ay * bz - az * by, b = az * bx - ax * bz, e = ax * by - ay * bx;
    const double norm = sqrt((a * a + b * b) + e * e);
    if (norm == 0.0) {
      pl[0] = pl[1] = pl[2] = pl[3] = 0.0;
      return;
    }
    a /= norm, b /= norm, e /= norm;
    pl[0] = a, pl[1] = b, pl[2] = e;
    pl[3] = -((a * x0 + b * y0) + e * z0);
    return;
  }
  double c[3] = {0.0, 0.0, 0.0};
  for (int k = 0; k < m; ++k)
    for (int a = 0; a < 3; ++a) c[a] += xyz64[3 * (int64_t)id[k] + a];
  for (int a = 0; a < 3; ++a) c[a] /= (double)m;
  double q[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int k = 0; k < m; ++k) {
    const double* p = xyz64 + 3 * (int64_t)id[k];
    const double rx = p[0] - c[0], ry = p[1] - c[1], rz = p[2] - c[2];
    q[0] += rx * rx, q[1] += rx * ry, q[2] += rx * rz;
    q[3] += ry * ry, q[4] += ry * rz, q[5] += rz * rz;
  }
  plane_from_moments(c, q, pl);
}

__global__ __launch_bounds__(kPlaneBlock) void plane_init_kernel(PlaneState* __restrict__ s, int64_t rows,
                                                                 int32_t* __restrict__ counts_out,
                                                                 double* __restrict__ err_out) {
  const int64_t t = (int64_t)blockIdx.x * kPlaneBlock + threadIdx.x;
  if (t == 0) {
    PlaneState z{};
    z.best_index = -1;
    z.break_it = INFINITY;
    *s = z;
  }
  for (int64_t r = t; r < rows; r += (int64_t)gridDim.x * kPlaneBlock) {
    if (counts_out != nullptr) counts_out[r] = -1;
    if (err_out != nullptr) err_out[r] = -1.0;
  }
}

// every supplied index inside [0, n), before any launch reads a point through one
__global__ __launch_bounds__(kPlaneBlock) void plane_check_samples_kernel(const int32_t* __restrict__ samples,
                                                                          int64_t count, int64_t n,
                                                                          PlaneState* __restrict__ s) {
  bool bad = false;
  for (int64_t k = (int64_t)blockIdx.x * kPlaneBlock + threadIdx.x; k < count; k += (int64_t)gridDim.x * kPlaneBlock) {
    const int32_t v = samples[k];
    bad |= v < 0 || (int64_t)v >= n;
  }
  if (bad) {
    s->bad = 1;
    s->done = 1;
  }
}

__global__ __launch_bounds__(kPlaneBlock) void plane_fit_kernel(const double* __restrict__ xyz64, int64_t n,
                                                                const int32_t* __restrict__ samples, uint64_t seed,
                                                                int64_t h0, int Hb, int rn,
                                                                double* __restrict__ planes,
                                                                int32_t* __restrict__ zflag,
                                                                const PlaneState* __restrict__ s) {
  if (s->done) return;
  const int t = blockIdx.x * kPlaneBlock + threadIdx.x;
  if (t >= Hb) return;
  const int64_t h = h0 + t;
  int32_t id[kMaxSample];
  double pl[4] = {0.0, 0.0, 0.0, 0.0};
  bool ok = true;
  if (samples != nullptr) {
    for (int k = 0; k < rn; ++k) {
      id[k] = samples[h * rn + k];
      ok &= id[k] >= 0 && (int64_t)id[k] < n;  // (plane_check_samples_kernel has flagged it)
    }
  } else {
    native_sample(seed, h, n, rn, id);
  }
  if (ok) plane_of_sample(xyz64, id, rn, pl);
  for (int k = 0; k < 4; ++k) planes[4 * (int64_t)t + k] = pl[k];
  zflag[t] = (pl[0] == 0.0 && pl[1] == 0.0 && pl[2] == 0.0 && pl[3] == 0.0) ? 1 : 0;
}

__device__ __forceinline__ void score_point(double a, double b, double c, double d, double thr, double x,
                                            double y, double z, int32_t& cnt, double& err) {
  const double dist = fabs(((a * x + b * y) + c * z) + d);
  const bool in = dist < thr;
  cnt += in ? 1 : 0;
  err += in ? dist * dist : 0.0;
}

// wave w of the launch: chunk w / ngroups, hypotheses 64·(w % ngroups) + lane.  H >= 1, n >= 1.
// pcnt / perr: [chunk][hstride] partials.  done: the loop's stop word, or null.
__global__ __launch_bounds__(kPlaneBlock) void plane_score_kernel(const double* __restrict__ xyz64, int64_t n,
                                                                  const double* __restrict__ planes, int H,
                                                                  int hstride, double thr,
                                                                  int32_t* __restrict__ pcnt,
                                                                  double* __restrict__ perr,
                                                                  const int32_t* __restrict__ done) {
  if (done != nullptr && *done) return;
  const int lane = threadIdx.x & 63;
  const int ngroups = (H + 63) >> 6;
  const int nchunks = (int)((n + kPlaneChunk - 1) / kPlaneChunk);
  const int w = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (kPlaneBlock / kWave) + (threadIdx.x >> 6)));
  if (w >= nchunks * ngroups) return;  // wave-uniform
  const int chunk = w / ngroups, grp = w - chunk * ngroups;
  const int h = grp * 64 + lane;
  double a = 0.0, b = 0.0, c = 0.0, d = 0.0;
  if (h < H) {
    const double* pl = planes + 4 * (int64_t)h;
    a = pl[0], b = pl[1], c = pl[2], d = pl[3];
  }
  const int64_t i0 = (int64_t)chunk * kPlaneChunk;
  const int m = (int)(n - i0 < kPlaneChunk ? n - i0 : kPlaneChunk);  // points of this chunk (>= 1)
  const double* __restrict__ p = xyz64 + 3 * i0;  // wave-uniform: scalar loads
  int32_t cnt = 0;
  double err = 0.0;
  int j = 0;
  for (; j + kScoreUnroll <= m; j += kScoreUnroll) {
    double q[3 * kScoreUnroll];
#pragma unroll
    for (int k = 0; k < 3 * kScoreUnroll; ++k) q[k] = p[3 * j + k];
#pragma unroll
    for (int u = 0; u < kScoreUnroll; ++u) score_point(a, b, c, d, thr, q[3 * u], q[3 * u + 1], q[3 * u + 2], cnt, err);
  }
  for (; j < m; ++j) score_point(a, b, c, d, thr, p[3 * j], p[3 * j + 1], p[3 * j + 2], cnt, err);
  if (h < H) {
    pcnt[(int64_t)chunk * hstride + h] = cnt;
    perr[(int64_t)chunk * hstride + h] = err;
  }
}

// counts[h], err[h] ← the chunk partials of hypothesis h in the fixed order of the header
__global__ __launch_bounds__(kReduceGroupsP* kReduceHyps) void plane_reduce_kernel(
    const int32_t* __restrict__ pcnt, const double* __restrict__ perr, int nchunks, int H, int hstride,
    int32_t* __restrict__ counts, double* __restrict__ err, const int32_t* __restrict__ done) {
  if (done != nullptr && *done) return;
  __shared__ double red_e[kReduceGroupsP][kReduceHyps];
  __shared__ int32_t red_c[kReduceGroupsP][kReduceHyps];
  const int slot = threadIdx.x % kReduceHyps, g = threadIdx.x / kReduceHyps;
  const int h = blockIdx.x * kReduceHyps + slot;
  double e = 0.0;
  int32_t k = 0;
  if (h < H) {
#pragma unroll 4
    for (int ch = g; ch < nchunks; ch += kReduceGroupsP) {
      e += perr[(int64_t)ch * hstride + h];
      k += pcnt[(int64_t)ch * hstride + h];
    }
  }
  red_e[g][slot] = e;
  red_c[g][slot] = k;
  __syncthreads();
  if (g == 0 && h < H) {
    double te = 0.0;
    int32_t tk = 0;
    for (int q = 0; q < kReduceGroupsP; ++q) {
      te += red_e[q][slot];
      tk += red_c[q][slot];
    }
    counts[h] = tk;
    if (err != nullptr) err[h] = te;
  }
}

__device__ __forceinline__ uint64_t bits_below(int k) { return k >= 64 ? ~0ull : ((1ull << k) - 1ull); }

// the sequential rule over rows h0 .. h0 + Hb − 1 (one wave)
__global__ __launch_bounds__(kWave) void plane_scan_kernel(PlaneState* __restrict__ s,
                                                           const int32_t* __restrict__ bcnt,
                                                           const double* __restrict__ berr,
                                                           const int32_t* __restrict__ zflag,
                                                           const double* __restrict__ planes, int64_t h0, int Hb,
                                                           int64_t n, int64_t num_iter, double probability,
                                                           int rn, int32_t* __restrict__ counts_out,
                                                           double* __restrict__ err_out) {
  if (s->done) return;
  const int lane = threadIdx.x;
  int64_t best_count = s->best_count, best_index = s->best_index, evaluated = s->evaluated;
  double best_rmse = s->best_rmse, break_it = s->break_it;
  bool stopped = false;
  int64_t stop_h = h0 + Hb;
  for (int base = 0; base < Hb && !stopped; base += 64) {
    const int r = base + lane;
    const int lim = Hb - base < 64 ? Hb - base : 64;  // rows of this step
    int32_t cnt = 0;
    double err = 0.0, rmse = 0.0;
    bool nz = false;
    if (lane < lim) {
      nz = zflag[r] == 0;
      cnt = bcnt[r];
      err = berr[r];
      rmse = cnt ? err / sqrt((double)cnt) : 0.0;
    }
    const uint64_t nzmask = __ballot(nz);
    int reached = lim;  // rows of this step the loop got to
    int pos = 0;
    while (pos < lim) {
      const bool act = lane >= pos && lane < lim;
      const int64_t evb = evaluated + (int64_t)__popcll(nzmask & bits_below(lane) & ~bits_below(pos));
      const uint64_t stopm = __ballot(act && (double)evb > break_it);
      const uint64_t beatm =
          __ballot(act && nz && ((int64_t)cnt > best_count || ((int64_t)cnt == best_count && rmse < best_rmse)));
      const int fs = stopm ? (int)__ffsll((unsigned long long)stopm) - 1 : 64;
      const int fb = beatm ? (int)__ffsll((unsigned long long)beatm) - 1 : 64;
      if (fs < 64 && fs <= fb) {  // the stop check of row fs comes before its evaluation
        evaluated += (int64_t)__popcll(nzmask & bits_below(fs) & ~bits_below(pos));
        stopped = true;
        stop_h = h0 + base + fs;
        reached = fs;
        break;
      }
      if (fb < 64) {  // a new best at row fb
        evaluated += (int64_t)__popcll(nzmask & bits_below(fb + 1) & ~bits_below(pos));
        best_count = (int64_t)__shfl(cnt, fb);
        best_rmse = __shfl(rmse, fb);
        best_index = h0 + base + fb;
        if (lane < 4) s->best_plane[lane] = planes[4 * (int64_t)(base + fb) + lane];
        const double f = (double)best_count / (double)n;
        break_it = f < 1.0 ? trunc(fmin(log(1.0 - probability) / log(1.0 - pow(f, (double)rn)), (double)num_iter)) : 0.0;
        pos = fb + 1;
      } else {
        evaluated += (int64_t)__popcll(nzmask & bits_below(lim) & ~bits_below(pos));
        pos = lim;
      }
    }
    if (lane < reached) {
      if (counts_out != nullptr) counts_out[h0 + r] = nz ? cnt : -1;
      if (err_out != nullptr) err_out[h0 + r] = nz ? err : -1.0;
    }
  }
  if (lane == 0) {
    s->best_count = best_count;
    s->best_index = best_index;
    s->best_rmse = best_rmse;
    s->break_it = break_it;
    s->evaluated = evaluated;
    s->iterations = stop_h;
    if (stopped) s->done = 1;
  }
}

__global__ __launch_bounds__(kPlaneBlock) void plane_flag_kernel(const double* __restrict__ xyz64, int64_t n,
                                                                 const PlaneState* __restrict__ s, double thr,
                                                                 uint8_t* __restrict__ keep) {
  const int64_t i = (int64_t)blockIdx.x * kPlaneBlock + threadIdx.x;
  if (i >= n) return;
  if (s->best_index < 0) {
    keep[i] = 0;
    return;
  }
  const double a = s->best_plane[0], b = s->best_plane[1], c = s->best_plane[2], d = s->best_plane[3];
  const double dist = fabs(((a * xyz64[3 * i] + b * xyz64[3 * i + 1]) + c * xyz64[3 * i + 2]) + d);
  keep[i] = dist < thr ? 1 : 0;
}

// refit pass 0: Σ p over the inliers; pass 1: Σ of the six products of r = p − centroid.
// partials: [block][6] (pass 0 uses three).
__global__ __launch_bounds__(kPlaneBlock) void plane_refit_partial_kernel(const double* __restrict__ xyz64,
                                                                          const int32_t* __restrict__ idx,
                                                                          int64_t m, int pass,
                                                                          const PlaneState* __restrict__ s,
                                                                          double* __restrict__ partials) {
  __shared__ double red[kPlaneBlock / kWave][6];
  const int64_t k = (int64_t)blockIdx.x * kPlaneBlock + threadIdx.x;
  double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (k < m) {
    const double* p = xyz64 + 3 * (int64_t)idx[k];
    if (pass == 0) {
      v[0] = p[0], v[1] = p[1], v[2] = p[2];
    } else {
      const double rx = p[0] - s->centroid[0], ry = p[1] - s->centroid[1], rz = p[2] - s->centroid[2];
      v[0] = rx * rx, v[1] = rx * ry, v[2] = rx * rz;
      v[3] = ry * ry, v[4] = ry * rz, v[5] = rz * rz;
    }
  }
#pragma unroll
  for (int q = 0; q < 6; ++q) {
    const double t = wave_sum(v[q]);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][q] = t;
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    double t = 0.0;
    for (int w = 0; w < kPlaneBlock / kWave; ++w) t += red[w][threadIdx.x];
    partials[(int64_t)blockIdx.x * 6 + threadIdx.x] = t;
  }
}

__global__ __launch_bounds__(kPlaneBlock) void plane_refit_final_kernel(const double* __restrict__ partials,
                                                                        int64_t nb, int64_t m, int pass,
                                                                        PlaneState* __restrict__ s) {
  __shared__ double red[6][kPlaneBlock];
  double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int64_t b = threadIdx.x; b < nb; b += kPlaneBlock)
    for (int q = 0; q < 6; ++q) v[q] += partials[b * 6 + q];
  for (int q = 0; q < 6; ++q) red[q][threadIdx.x] = v[q];
  __syncthreads();
  for (int w = kPlaneBlock / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w)
      for (int q = 0; q < 6; ++q) red[q][threadIdx.x] += red[q][threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    if (pass == 0) {
      for (int a = 0; a < 3; ++a) s->centroid[a] = red[a][0] / (double)m;
    } else {
      const double q[6] = {red[0][0], red[1][0], red[2][0], red[3][0], red[4][0], red[5][0]};
      double pl[4];
      plane_from_moments(s->centroid, q, pl);
      for (int k = 0; k < 4; ++k) s->plane[k] = pl[k];
    }
  }
}

int64_t chunks_of(int64_t n) { return (n + kPlaneChunk - 1) / kPlaneChunk; }

// the per-(chunk, plane) partials of a batch of hb planes over n points, placed onto `scratch`
// (null: the layout's size alone)
struct ScoreScratch {
  double* perr = nullptr;
  int32_t* pcnt = nullptr;
  size_t bytes = 0;
  ScoreScratch(int64_t n, int64_t hb, void* scratch) {
    const size_t cells = (size_t)chunks_of(n) * (size_t)std::max<int64_t>(hb, 1);
    Carve cv;
    cv.add(&perr, cells);
    cv.add(&pcnt, cells);
    bytes = cv.bytes();
    if (scratch != nullptr) cv.place(scratch);
  }
};

// score + reduce of H <= plane_batch_cap(n) planes; n >= 1, H >= 1
// (profiling: the score kernel under M3D_KERNEL_SCORE, the reduce under M3D_KERNEL_LOOP)
hipError_t score_batch(m3d_ctx* ctx, const double* xyz64, int64_t n, const double* planes, int H, double thr,
                       int32_t* counts, double* err, const ScoreScratch& L, const int32_t* done, hipStream_t st) {
  const int nchunks = (int)chunks_of(n);
  const int ngroups = (H + 63) / 64;
  int32_t* pcnt = L.pcnt;
  double* perr = L.perr;
  const int64_t waves = (int64_t)nchunks * ngroups;
  const unsigned blocks = (unsigned)((waves + kPlaneBlock / kWave - 1) / (kPlaneBlock / kWave));
  {
    KTimer t(ctx, M3D_KERNEL_SCORE, st);
    plane_score_kernel<<<blocks, kPlaneBlock, 0, st>>>(xyz64, n, planes, H, H, thr, pcnt, perr, done);
  }
  KTimer t(ctx, M3D_KERNEL_LOOP, st);
  plane_reduce_kernel<<<(unsigned)((H + kReduceHyps - 1) / kReduceHyps), kReduceGroupsP * kReduceHyps, 0, st>>>(
      pcnt, perr, nchunks, H, H, counts, err, done);
  return hipGetLastError();
}

// the pieces of a segment_plane call's scratch, placed onto `scratch` (null: the layout's size alone)
struct SegScratch {
  PlaneState* state = nullptr;
  double* planes = nullptr;
  int32_t *zflag = nullptr, *bcnt = nullptr;
  double* berr = nullptr;
  char* score = nullptr;  // a ScoreScratch of `batch` planes
  uint8_t* keep = nullptr;
  int32_t* nsel = nullptr;
  double* partials = nullptr;
  char* tmp = nullptr;
  size_t tmp_bytes = 0, bytes = 0;
  SegScratch(int64_t n, int batch, void* scratch) {
    size_t tb = 0;
    hipcub::DeviceSelect::Flagged(nullptr, tb, hipcub::CountingInputIterator<int32_t>(0), (uint8_t*)nullptr,
                                  (int32_t*)nullptr, (int32_t*)nullptr, (int)n, (hipStream_t)0);
    tmp_bytes = std::max<size_t>(tb, 1);
    const size_t B = (size_t)std::max(batch, 1);
    Carve cv;
    cv.add(&state, 1);
    cv.add(&planes, 4 * B);
    cv.add(&zflag, B);
    cv.add(&bcnt, B);
    cv.add(&berr, B);
    cv.add(&score, ScoreScratch(n, batch, nullptr).bytes);
    cv.add(&keep, (size_t)n);
    cv.add(&nsel, 1);
    cv.add(&partials, 6 * (size_t)((n + kPlaneBlock - 1) / kPlaneBlock));
    cv.add(&tmp, tmp_bytes);
    bytes = cv.bytes();
    if (scratch != nullptr) cv.place(scratch);
  }
};

}  // namespace

int64_t plane_batch_cap(int64_t n) {
  const int64_t per = kPartialBudget / std::max<int64_t>(chunks_of(n), 1);
  return std::max<int64_t>(64, std::min<int64_t>(4096, per / 64 * 64));
}

size_t plane_score_scratch_bytes(int64_t n, int64_t H) {
  return n > 0 && H > 0 ? ScoreScratch(n, std::min(H, plane_batch_cap(n)), nullptr).bytes : 0;
}

hipError_t plane_score(const m3d_cloud* c, const double* planes, int64_t H, double thr, int32_t* counts,
                       double* err, void* scratch, hipStream_t st) {
  const int64_t n = c->n;
  if (n <= 0 || H <= 0) return hipSuccess;  // nothing is launched: no array is touched
  const int64_t cap = plane_batch_cap(n);
  const ScoreScratch L(n, std::min(H, cap), scratch);
  for (int64_t h0 = 0; h0 < H; h0 += cap) {
    const int hb = (int)std::min(cap, H - h0);
    const hipError_t e = score_batch(c->ctx, c->xyz64, n, planes + 4 * h0, hb, thr, counts + h0,
                                     err != nullptr ? err + h0 : nullptr, L, nullptr, st);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

// automatic: enough hypotheses for ≈ 4096 waves (four per SIMD), whole lane groups, at most 1024 —
// an early stop throws away what the batch scored beyond it
int segment_plane_batch(int64_t n, const m3d_plane_params* p) {
  int64_t b = p->batch;
  if (b <= 0) {
    const int64_t nchunks = std::max<int64_t>(chunks_of(n), 1);
    b = 64 * std::min<int64_t>(16, std::max<int64_t>(1, (4096 + nchunks - 1) / nchunks));
  }
  b = std::min<int64_t>(b, std::max<int64_t>(p->num_iterations, 1));
  return (int)std::min<int64_t>(b, plane_batch_cap(n));
}

size_t segment_plane_scratch_bytes(int64_t n, int batch) { return SegScratch(n, batch, nullptr).bytes; }

hipError_t segment_plane(const m3d_cloud* c, const m3d_plane_params* p, int batch, const int32_t* samples,
                         m3d_plane_result* out, int32_t* inliers_out, int32_t* counts_out, double* err_out,
                         void* scratch, hipStream_t st, int* bad_sample) {
  const int64_t n = c->n;  // >= ransac_n >= 3 (api_prep.cpp)
  const int64_t H = p->num_iterations;
  const int rn = p->ransac_n;
  const double thr = p->distance_threshold;
  const SegScratch L(n, batch, scratch);
  const ScoreScratch Lsc(n, batch, L.score);
  PlaneState* s = L.state;
  double *planes = L.planes, *berr = L.berr, *partials = L.partials;
  int32_t *zflag = L.zflag, *bcnt = L.bcnt, *nsel = L.nsel;
  uint8_t* keep = L.keep;
  m3d_ctx* ctx = c->ctx;
  *bad_sample = 0;
  hipError_t e;

  {
    const unsigned blocks = (unsigned)std::max<int64_t>(1, std::min<int64_t>(1024, (H + kPlaneBlock - 1) / kPlaneBlock));
    plane_init_kernel<<<blocks, kPlaneBlock, 0, st>>>(s, H, counts_out, err_out);
    if (samples != nullptr && H > 0) {
      const int64_t cnt = H * rn;
      const unsigned cb = (unsigned)std::min<int64_t>(1024, (cnt + kPlaneBlock - 1) / kPlaneBlock);
      plane_check_samples_kernel<<<cb, kPlaneBlock, 0, st>>>(samples, cnt, n, s);
    }
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }

  // batches in growing groups (1, 2, 4, … batches) with a look at `done` in between
  int64_t h0 = 0;
  for (int64_t group = 1; h0 < H; group *= 2) {
    for (int64_t b = 0; b < group && h0 < H; ++b, h0 += batch) {
      const int hb = (int)std::min<int64_t>(batch, H - h0);
      {
        KTimer t(ctx, M3D_KERNEL_KABSCH, st);
        plane_fit_kernel<<<(unsigned)((hb + kPlaneBlock - 1) / kPlaneBlock), kPlaneBlock, 0, st>>>(
            c->xyz64, n, samples, p->seed, h0, hb, rn, planes, zflag, s);
      }
      if ((e = score_batch(ctx, c->xyz64, n, planes, hb, thr, bcnt, berr, Lsc, &s->done, st)) != hipSuccess)
        return e;
      {
        KTimer t(ctx, M3D_KERNEL_LOOP, st);
        plane_scan_kernel<<<1, kWave, 0, st>>>(s, bcnt, berr, zflag, planes, h0, hb, n, H, p->probability, rn,
                                               counts_out, err_out);
      }
      if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    if (h0 >= H) break;
    int32_t done = 0;
    if ((e = hipMemcpyAsync(&done, &s->done, sizeof(done), hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
    if ((e = hipStreamSynchronize(st)) != hipSuccess) return e;
    if (done) break;
  }

  // inliers of the best plane, ascending
  int32_t m32 = 0;
  {
    KTimer t(ctx, M3D_KERNEL_NN, st);
    plane_flag_kernel<<<(unsigned)((n + kPlaneBlock - 1) / kPlaneBlock), kPlaneBlock, 0, st>>>(c->xyz64, n, s, thr, keep);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    size_t tb = L.tmp_bytes;
    e = hipcub::DeviceSelect::Flagged(L.tmp, tb, hipcub::CountingInputIterator<int32_t>(0), keep, inliers_out,
                                      nsel, (int)n, st);
    if (e != hipSuccess) return e;
  }
  PlaneState hs;
  if ((e = hipMemcpyAsync(&m32, nsel, sizeof(m32), hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
  if ((e = hipMemcpyAsync(&hs, s, sizeof(hs), hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
  if ((e = hipStreamSynchronize(st)) != hipSuccess) return e;
  if (hs.bad) {
    *bad_sample = 1;
    return hipSuccess;
  }
  const int64_t m = m32;
  if (hs.best_index >= 0 && m >= 3) {  // the refit (else the zero plane of the init)
    KTimer t(ctx, M3D_KERNEL_TERMS, st);
    const int64_t nb = (m + kPlaneBlock - 1) / kPlaneBlock;
    for (int pass = 0; pass < 2; ++pass) {
      plane_refit_partial_kernel<<<(unsigned)nb, kPlaneBlock, 0, st>>>(c->xyz64, inliers_out, m, pass, s, partials);
      plane_refit_final_kernel<<<1, kPlaneBlock, 0, st>>>(partials, nb, m, pass, s);
    }
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = hipMemcpyAsync(&hs, s, sizeof(hs), hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
  }
  if ((e = hipStreamSynchronize(st)) != hipSuccess) return e;  // (the refit's timer has closed)
  for (int k = 0; k < 4; ++k) {
    out->plane[k] = hs.plane[k];
    out->ransac_plane[k] = hs.best_plane[k];
  }
  out->num_inliers = m;
  out->best_index = hs.best_index;
  out->best_count = hs.best_count;
  out->evaluated = hs.evaluated;
  out->iterations = hs.iterations;
  out->best_rmse = hs.best_rmse;
  return hipSuccess;
}

}  // namespace m3d
