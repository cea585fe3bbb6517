// fgr.hip — Fast Global Registration on the device (Zhou, Park, Koltun; Open3D 0.19
// FastGlobalRegistration.cpp as restated in include/m3d.h and tests/fgr_restatement.py).
//
// All arithmetic is fp64, every operation rounded on its own in the order written
// (-ffp-contract=off, IEEE division and sqrt).
//
// THE SUM ORDER.  Every sum of the feature (the two means, the 16 loop sums the 27 entries of JᵀJ
// and Jᵀr are made of) is taken in one order that depends on the element count n alone:
//   level 1  segment s holds elements [384·s, 384·s + 384): lane l of 64 adds its six elements
//            384·s + l + 64·k, k = 0 … 5, sequentially onto +0.0 (an element past n adds nothing),
//            then the 64 lane sums go through the xor butterfly 32, 16, 8, 4, 2, 1 (a + b and
//            b + a are the same bits, so every lane ends with the tree  v[:h] + v[h:], h = 32 … 1)
//   level 2  lane g adds the segment sums g, g + 64, g + 128, … sequentially onto +0.0, then the
//            same butterfly
// The one-workgroup loop keeps a segment per wave (six rows per lane in registers) and the segment
// sums in LDS; the multi-block loop keeps a segment per wave too and the segment sums in global
// memory, where the last block to finish (an integer ticket) runs level 2.  Both therefore return
// the same bits, as does a launch of any shape.  No floating-point atomics anywhere.
//
// Stages (api_prep.cpp m3d_fgr_*):
//   normalise  the two means in the order above, the largest centred norm by an integer atomic max
//              on the bit pattern of the non-negative fp64 norms, then each correspondence row's
//              two points centred and divided: (S[i] − m0) / g, (G[j] − m1) / g
//   tuple test one trial per lane in batches of kFgrTrialBatch trials in trial order: an accept
//              flag, a stable compaction (hipcub) and an append that stops at the cap; `done`
//              makes every later launch return at once and the host looks at it between growing
//              groups of batches (plane.hip's scheme)
//   loop       ≤ kFgrOneWgRows rows: ONE launch of one 512-thread workgroup runs every iteration —
//              terms → 16 sums → solve → move q — with p, q, T and par in registers, one barrier
//              per iteration (the segment sums are double-buffered in LDS) and the solve done by
//              every lane (the same bits everywhere: no second barrier for a broadcast);
//              more rows: one launch per iteration, each wave first applying the previous δ to
//              its q, the last block solving and publishing δ, T and par; no host sync in between
#include <algorithm>
#include <cmath>

#include <hipcub/hipcub.hpp>

#include "linalg.h"
#include "m3d_internal.h"
#include "sampler.h"

namespace m3d {
namespace {

constexpr int kSegK = kFgrSegRows / kWave;              // elements per lane of a segment
constexpr int kOneWgThreads = kFgrOneWgRows / kSegK;    // 512: a segment per wave
constexpr int kOneWgWaves = kOneWgThreads / kWave;      // 8
constexpr int kMultiBlock = 256;                        // four segments per block
constexpr int kNS = 16;                                 // distinct loop sums
static_assert(kFgrSegRows % kWave == 0 && kFgrOneWgRows % kFgrSegRows == 0, "whole segments");
static_assert(kOneWgWaves <= kWave, "level 2 of the one-workgroup path is one step");

struct FgrState {
  double mean[2][3];
  double g, par0, scale;
  double T[16], dT[16], par;
  double sums[kNS];
  unsigned long long scale_bits;
  int64_t trials;
  int32_t accepted, done, bad;
  uint32_t ticket;
};

struct LoopArgs {
  int32_t iters, decrease_mu;
  double maxcd, div;
};

__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
  return v;
}

__device__ __forceinline__ void st_wt(double* p, double v) {  // write-through (cross-XCD hand-off)
  __hip_atomic_store(reinterpret_cast<unsigned long long*>(p), (unsigned long long)__double_as_longlong(v),
                     __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ double ld_wt(const double* p) {
  return __longlong_as_double((long long)__hip_atomic_load(reinterpret_cast<const unsigned long long*>(p),
                                                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}

// ------------------------------------------------------------------------------- normalise
__global__ __launch_bounds__(kMultiBlock) void fgr_init_kernel(FgrState* __restrict__ s) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    FgrState z{};
    for (int k = 0; k < 16; ++k) z.T[k] = z.dT[k] = (k % 5 == 0) ? 1.0 : 0.0;
    *s = z;
  }
}

// level 1 of Σ xyz: part[seg][3]
__global__ __launch_bounds__(kMultiBlock) void fgr_mean_partial_kernel(const double* __restrict__ xyz, int64_t n,
                                                                       int64_t nseg, double* __restrict__ part) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t seg = (int64_t)blockIdx.x * (kMultiBlock / kWave) + (threadIdx.x >> 6);
  if (seg >= nseg) return;  // wave-uniform
  double a[3] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int k = 0; k < kSegK; ++k) {
    const int64_t i = seg * kFgrSegRows + lane + (int64_t)kWave * k;
    if (i < n) {
      a[0] += xyz[3 * i], a[1] += xyz[3 * i + 1], a[2] += xyz[3 * i + 2];
    }
  }
#pragma unroll
  for (int v = 0; v < 3; ++v) {
    const double t = wave_sum(a[v]);
    if (lane == 0) part[seg * 3 + v] = t;
  }
}

// level 2 and the division (one wave)
__global__ __launch_bounds__(kWave) void fgr_mean_final_kernel(const double* __restrict__ part, int64_t nseg,
                                                               int64_t n, FgrState* __restrict__ s, int which) {
  const int lane = threadIdx.x;
  double a[3] = {0.0, 0.0, 0.0};
  for (int64_t g = lane; g < nseg; g += kWave) {
    a[0] += part[g * 3], a[1] += part[g * 3 + 1], a[2] += part[g * 3 + 2];
  }
#pragma unroll
  for (int v = 0; v < 3; ++v) {
    const double t = wave_sum(a[v]);
    if (lane == 0) s->mean[which][v] = t / (double)n;
  }
}

// the largest √((x² + y²) + z²) of the centred cloud: a max of non-negative doubles is the max of
// their bit patterns as integers
__global__ __launch_bounds__(kMultiBlock) void fgr_maxnorm_kernel(const double* __restrict__ xyz, int64_t n,
                                                                  FgrState* __restrict__ s, int which) {
  const double mx = s->mean[which][0], my = s->mean[which][1], mz = s->mean[which][2];
  double best = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * kMultiBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kMultiBlock) {
    const double x = xyz[3 * i] - mx, y = xyz[3 * i + 1] - my, z = xyz[3 * i + 2] - mz;
    const double d = sqrt((x * x + y * y) + z * z);
    best = d > best ? d : best;  // (a NaN norm is never taken)
  }
  best = wave_max(best);
  if ((threadIdx.x & (kWave - 1)) == 0) atomicMax(&s->scale_bits, (unsigned long long)__double_as_longlong(best));
}

__global__ void fgr_scale_kernel(FgrState* __restrict__ s, int absolute) {
  const double scale = __longlong_as_double((long long)s->scale_bits);
  s->scale = scale;
  s->g = absolute ? 1.0 : scale;
  s->par0 = absolute ? scale : 1.0;
  s->par = s->par0;
}

// rows → the normalised pairs pr[r] = (S[i] − m0) / g, qr[r] = (G[j] − m1) / g; an index outside
// its cloud is flagged before any point is read through it
__global__ __launch_bounds__(kMultiBlock) void fgr_gather_kernel(const double* __restrict__ src, int64_t ns,
                                                                 const double* __restrict__ tgt, int64_t nt,
                                                                 const int32_t* __restrict__ corr, int64_t nc,
                                                                 FgrState* __restrict__ s, double* __restrict__ pr,
                                                                 double* __restrict__ qr) {
  const int64_t r = (int64_t)blockIdx.x * kMultiBlock + threadIdx.x;
  if (r >= nc) return;
  const int64_t i = corr[2 * r], j = corr[2 * r + 1];
  if (i < 0 || i >= ns || j < 0 || j >= nt) {
    s->bad = 1;
#pragma unroll
    for (int a = 0; a < 3; ++a) pr[3 * r + a] = qr[3 * r + a] = 0.0;
    return;
  }
  const double g = s->g;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    pr[3 * r + a] = (src[3 * i + a] - s->mean[0][a]) / g;
    qr[3 * r + a] = (tgt[3 * j + a] - s->mean[1][a]) / g;
  }
}

// ------------------------------------------------------------------------------- tuple test
__device__ __forceinline__ double edge_len(const double* __restrict__ a, int64_t u, int64_t v) {
  const double dx = a[3 * u] - a[3 * v], dy = a[3 * u + 1] - a[3 * v + 1], dz = a[3 * u + 2] - a[3 * v + 2];
  return sqrt((dx * dx + dy * dy) + dz * dz);
}

__global__ __launch_bounds__(kMultiBlock) void fgr_tuple_flag_kernel(const double* __restrict__ pr,
                                                                     const double* __restrict__ qr, int64_t n,
                                                                     uint64_t seed, int64_t h0, int count,
                                                                     double tuple_scale, uint8_t* __restrict__ flag,
                                                                     const FgrState* __restrict__ s) {
  if (s->done) return;
  const int t = blockIdx.x * kMultiBlock + threadIdx.x;
  if (t >= count) return;
  int64_t r[3];
  trial_rows(seed, h0 + t, n, r);
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int64_t u = r[k], v = r[(k + 1) % 3];
    const double li = edge_len(pr, u, v), lj = edge_len(qr, u, v);
    ok = ok && (li * tuple_scale < lj) && (lj < li / tuple_scale);
  }
  flag[t] = ok ? 1 : 0;
}

// the batch's accepted trials (ascending) onto the list, up to the cap; one block
__global__ __launch_bounds__(kMultiBlock) void fgr_tuple_append_kernel(const int64_t* __restrict__ sel,
                                                                       const int32_t* __restrict__ nsel,
                                                                       int64_t cap, int64_t* __restrict__ accepted,
                                                                       int64_t h_end, FgrState* __restrict__ s) {
  if (s->done) return;
  const int64_t have = s->accepted;
  const int64_t m = *nsel;
  const int64_t take = m < cap - have ? m : cap - have;
  __syncthreads();
  for (int64_t k = threadIdx.x; k < take; k += kMultiBlock) accepted[have + k] = sel[k];
  if (threadIdx.x == 0) {
    s->accepted = (int32_t)(have + take);
    if (have + take >= cap) {  // (cap ≥ 1: the stopping trial is this batch's take-th)
      s->done = 1;
      s->trials = sel[take - 1] + 1;
    } else {
      s->trials = h_end;
    }
  }
}

// the row set of the accepted trials: p, q (3 per trial) and the caller's (i, j) rows
__global__ __launch_bounds__(kMultiBlock) void fgr_tuple_rows_kernel(const double* __restrict__ pr,
                                                                     const double* __restrict__ qr,
                                                                     const int32_t* __restrict__ corr, int64_t n,
                                                                     uint64_t seed,
                                                                     const int64_t* __restrict__ accepted,
                                                                     const FgrState* __restrict__ s,
                                                                     double* __restrict__ p, double* __restrict__ q,
                                                                     int32_t* __restrict__ rows_out) {
  const int64_t t = (int64_t)blockIdx.x * kMultiBlock + threadIdx.x;
  if (t >= s->accepted) return;
  int64_t r[3];
  trial_rows(seed, accepted[t], n, r);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int64_t o = 3 * t + k;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      p[3 * o + a] = pr[3 * r[k] + a];
      q[3 * o + a] = qr[3 * r[k] + a];
    }
    if (rows_out != nullptr) {
      rows_out[2 * o] = corr[2 * r[k]];
      rows_out[2 * o + 1] = corr[2 * r[k] + 1];
    }
  }
}

// ------------------------------------------------------------------------------- the loop
// One row's terms onto the 16 sums.  With r = p − q, s = (par / (r·r + par))² and the Jacobian
// rows Jx = (0, −z, y, −1, 0, 0), Jy = (z, 0, −x, 0, −1, 0), Jz = (−y, x, 0, 0, 0, −1) of q = (x, y, z),
// every entry of Σ s·J Jᵀ and Σ s·J r is one of these sums, its negative or zero (expand_sums).
__device__ __forceinline__ void row_terms(double px, double py, double pz, double x, double y, double z,
                                          double par, double acc[kNS]) {
  const double rx = px - x, ry = py - y, rz = pz - z;
  const double rr = (rx * rx + ry * ry) + rz * rz;
  const double w = par / (rr + par);
  const double s = w * w;
  acc[0] += s * (y * y + z * z);
  acc[1] += s * (x * y);
  acc[2] += s * (x * z);
  acc[3] += s * (x * x + z * z);
  acc[4] += s * (y * z);
  acc[5] += s * (x * x + y * y);
  acc[6] += s * x;
  acc[7] += s * y;
  acc[8] += s * z;
  acc[9] += s;
  acc[10] += s * (z * ry - y * rz);
  acc[11] += s * (x * rz - z * rx);
  acc[12] += s * (y * rx - x * ry);
  acc[13] += s * rx;
  acc[14] += s * ry;
  acc[15] += s * rz;
}

}  // namespace

// the 21 upper-triangle entries of JᵀJ (row-major) and the 6 of Jᵀr from the 16 sums; a negative is
// 0 − S (never −0.0)
__host__ __device__ void fgr_expand_sums(const double S[16], double out[27]) {
  const double z = 0.0;
  const double v[27] = {S[0], z - S[1], z - S[2], z, z - S[8], S[7],   // row 0
                        S[3], z - S[4], S[8], z, z - S[6],            // row 1
                        S[5], z - S[7], S[6], z,                      // row 2
                        S[9], z, z, S[9], z, S[9],                    // rows 3, 4, 5
                        S[10], S[11], S[12], z - S[13], z - S[14], z - S[15]};
  for (int k = 0; k < 27; ++k) out[k] = v[k];
}

namespace {

// JᵀJ x = −Jᵀr by the ICP tail's rule (unpivoted while every pivot is safe, else Eigen's pivot
// order), δ = vec6_to_matrix(x); a non-finite δ is the identity
__device__ void solve_delta(const double S[kNS], double dT[16]) {
  double e[27], A[36], b[6], x[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  fgr_expand_sums(S, e);
  int k = 0;
#pragma unroll
  for (int a = 0; a < 6; ++a)
#pragma unroll
    for (int c = a; c < 6; ++c) {
      A[a * 6 + c] = e[k];
      A[c * 6 + a] = e[k];
      ++k;
    }
#pragma unroll
  for (int a = 0; a < 6; ++a) b[a] = 0.0 - e[21 + a];
  if (!ldlt6_solve_spd(A, b, x)) ldlt6_solve(A, b, x);
  vec6_to_matrix(x, dT);
  bool finite = true;
#pragma unroll
  for (int i = 0; i < 16; ++i) finite = finite && isfinite(dT[i]);
  if (!finite)
#pragma unroll
    for (int i = 0; i < 16; ++i) dT[i] = (i % 5 == 0) ? 1.0 : 0.0;
}

__device__ __forceinline__ void move_point(const double d[16], double& x, double& y, double& z) {
  const double nx = ((d[0] * x + d[1] * y) + d[2] * z) + d[3];
  const double ny = ((d[4] * x + d[5] * y) + d[6] * z) + d[7];
  const double nz = ((d[8] * x + d[9] * y) + d[10] * z) + d[11];
  x = nx, y = ny, z = nz;
}

__device__ __forceinline__ double next_par(double par, int itr, const LoopArgs& a) {
  return (a.decrease_mu && itr % 4 == 0 && par > a.maxcd) ? par / a.div : par;
}

// One workgroup, every iteration.  10 ≤ n ≤ kFgrOneWgRows (sums_only: 1 ≤ n, one terms pass at
// `par_in`, the 16 sums to s->sums).
__global__ __launch_bounds__(kOneWgThreads) void fgr_loop_one_kernel(const double* __restrict__ p,
                                                                     const double* __restrict__ q, int n,
                                                                     LoopArgs a, int sums_only, double par_in,
                                                                     FgrState* __restrict__ s) {
  __shared__ double part[2][kOneWgWaves][kNS];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
  double P[kSegK][3], Q[kSegK][3];
#pragma unroll
  for (int k = 0; k < kSegK; ++k) {
    const int r = wave * kFgrSegRows + lane + kWave * k;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      P[k][c] = r < n ? p[3 * r + c] : 0.0;
      Q[k][c] = r < n ? q[3 * r + c] : 0.0;
    }
  }
  double T[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) T[i] = (i % 5 == 0) ? 1.0 : 0.0;
  double par = sums_only ? par_in : s->par0;
  const int iters = sums_only ? 1 : a.iters;
  for (int itr = 0; itr < iters; ++itr) {
    double acc[kNS];
#pragma unroll
    for (int v = 0; v < kNS; ++v) acc[v] = 0.0;
#pragma unroll
    for (int k = 0; k < kSegK; ++k)
      if (wave * kFgrSegRows + lane + kWave * k < n)
        row_terms(P[k][0], P[k][1], P[k][2], Q[k][0], Q[k][1], Q[k][2], par, acc);
#pragma unroll
    for (int v = 0; v < kNS; ++v) {
      const double t = wave_sum(acc[v]);
      if (lane == 0) part[itr & 1][wave][v] = t;
    }
    __syncthreads();
    // level 2 in every wave: lane g holds segment g's sum (+0.0 + S_g), then the butterfly
    double S[kNS];
#pragma unroll
    for (int v = 0; v < kNS; ++v) {
      double t = 0.0;
      if (lane < kOneWgWaves) t += part[itr & 1][lane][v];
      S[v] = wave_sum(t);
    }
    if (sums_only) {
      if (threadIdx.x < kNS) {
        double mine = 0.0;
#pragma unroll
        for (int v = 0; v < kNS; ++v) mine = (int)threadIdx.x == v ? S[v] : mine;
        s->sums[threadIdx.x] = mine;
      }
      return;
    }
    double dT[16];
    solve_delta(S, dT);
    matmul4_affine(dT, T, T);
#pragma unroll
    for (int k = 0; k < kSegK; ++k) move_point(dT, Q[k][0], Q[k][1], Q[k][2]);
    par = next_par(par, itr, a);
  }
  if (threadIdx.x == 0) {
#pragma unroll
    for (int i = 0; i < 16; ++i) s->T[i] = T[i];
    s->par = par;
  }
}

// One iteration over any number of rows: wave = segment.  itr > 0: q ← δ·q first (the previous
// launch's δ).  The last block reduces the segment sums and publishes δ, T and par (sums_only:
// just the sums, at par_in).
__global__ __launch_bounds__(kMultiBlock) void fgr_loop_multi_kernel(const double* __restrict__ p,
                                                                     double* __restrict__ q, int64_t n,
                                                                     int64_t nseg, int itr, LoopArgs a,
                                                                     int sums_only, double par_in,
                                                                     double* __restrict__ part,
                                                                     FgrState* __restrict__ s) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t seg = (int64_t)blockIdx.x * (kMultiBlock / kWave) + (threadIdx.x >> 6);
  const double par = sums_only ? par_in : s->par;
  if (seg < nseg) {  // wave-uniform
    double d[12];
    const bool move = !sums_only && itr > 0;
    if (move)
#pragma unroll
      for (int i = 0; i < 12; ++i) d[i] = s->dT[i];
    double acc[kNS];
#pragma unroll
    for (int v = 0; v < kNS; ++v) acc[v] = 0.0;
#pragma unroll
    for (int k = 0; k < kSegK; ++k) {
      const int64_t r = seg * kFgrSegRows + lane + (int64_t)kWave * k;
      if (r < n) {
        double x = q[3 * r], y = q[3 * r + 1], z = q[3 * r + 2];
        if (move) {
          move_point(d, x, y, z);
          q[3 * r] = x, q[3 * r + 1] = y, q[3 * r + 2] = z;
        }
        row_terms(p[3 * r], p[3 * r + 1], p[3 * r + 2], x, y, z, par, acc);
      }
    }
#pragma unroll
    for (int v = 0; v < kNS; ++v) {
      const double t = wave_sum(acc[v]);
      if (lane == 0) st_wt(part + seg * kNS + v, t);
    }
  }
  // the segment sums went out write-through: every wave drains its stores, then one lane takes
  // the ticket; the block whose add returned the last number reads them with L1-bypassing loads
  __shared__ int last;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0)
    last = __hip_atomic_fetch_add(&s->ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1;
  __syncthreads();
  if (!last || threadIdx.x >= kWave) return;
  double S[kNS];
#pragma unroll
  for (int v = 0; v < kNS; ++v) S[v] = 0.0;
  for (int64_t g = lane; g < nseg; g += kWave)
#pragma unroll
    for (int v = 0; v < kNS; ++v) S[v] += ld_wt(part + g * kNS + v);
#pragma unroll
  for (int v = 0; v < kNS; ++v) S[v] = wave_sum(S[v]);
  if (lane == 0) s->ticket = 0;
  if (sums_only) {
    if (lane == 0)
#pragma unroll
      for (int v = 0; v < kNS; ++v) s->sums[v] = S[v];
    return;
  }
  double dT[16], T[16];
  solve_delta(S, dT);
#pragma unroll
  for (int i = 0; i < 16; ++i) T[i] = s->T[i];
  matmul4_affine(dT, T, T);
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      s->dT[i] = dT[i];
      s->T[i] = T[i];
    }
    s->par = next_par(par, itr, a);
  }
}

int64_t segs_of(int64_t n) { return (n + kFgrSegRows - 1) / kFgrSegRows; }

// the pieces of a call's scratch, placed onto `scratch` (null: the layout's size alone)
struct FgrScratch {
  FgrState* state = nullptr;
  double *mpart = nullptr, *pr = nullptr, *qr = nullptr;
  uint8_t* flag = nullptr;
  int64_t* sel = nullptr;
  int32_t* nsel = nullptr;
  int64_t* accepted = nullptr;
  double *p = nullptr, *q = nullptr, *lpart = nullptr;
  char* tmp = nullptr;
  size_t tmp_bytes = 0, bytes = 0;
  FgrScratch(int64_t ns, int64_t nt, int64_t nc, int64_t cap, void* scratch) {
    size_t tb = 0;
    hipcub::DeviceSelect::Flagged(nullptr, tb, hipcub::CountingInputIterator<int64_t>(0), (uint8_t*)nullptr,
                                  (int64_t*)nullptr, (int32_t*)nullptr, kFgrTrialBatch, (hipStream_t)0);
    tmp_bytes = std::max<size_t>(tb, 1);
    const size_t rows = (size_t)std::max<int64_t>(std::max<int64_t>(3 * cap, nc), 1);
    const size_t c1 = (size_t)std::max<int64_t>(nc, 1);
    Carve cv;
    cv.add(&state, 1);
    cv.add(&mpart, 3 * (size_t)segs_of(std::max(ns, nt)));
    cv.add(&pr, 3 * c1);
    cv.add(&qr, 3 * c1);
    cv.add(&flag, kFgrTrialBatch);
    cv.add(&sel, kFgrTrialBatch);
    cv.add(&nsel, 1);
    cv.add(&accepted, (size_t)cap);
    cv.add(&p, 3 * rows);
    cv.add(&q, 3 * rows);
    cv.add(&lpart, kNS * (size_t)segs_of((int64_t)rows));
    cv.add(&tmp, tmp_bytes);
    bytes = cv.bytes();
    if (scratch != nullptr) cv.place(scratch);
  }
};

// fgr_terms' scratch: the state and one row of partials per segment of n rows
struct FgrTermsScratch {
  FgrState* state = nullptr;
  double* part = nullptr;
  size_t bytes = 0;
  FgrTermsScratch(int64_t n, void* scratch) {
    Carve cv;
    cv.add(&state, 1);
    cv.add(&part, kNS * (size_t)segs_of(n));
    bytes = cv.bytes();
    if (scratch != nullptr) cv.place(scratch);
  }
};

hipError_t read_state(const FgrState* s, FgrState* h, hipStream_t st) {
  hipError_t e = hipMemcpyAsync(h, s, sizeof(FgrState), hipMemcpyDeviceToHost, st);
  return e != hipSuccess ? e : hipStreamSynchronize(st);
}

}  // namespace

// the tuples the test can keep: the first max(maximum_tuple_count, 1) accepted of at most 100·nc trials
int64_t fgr_tuple_cap(const m3d_fgr_params* p, int64_t nc) {
  if (!p->tuple_test) return 0;
  return std::min<int64_t>(std::max<int64_t>(p->maximum_tuple_count, 1), std::max<int64_t>(100 * nc, 1));
}

size_t fgr_scratch_bytes(int64_t ns, int64_t nt, int64_t nc, int64_t cap) {
  return FgrScratch(ns, nt, nc, cap, nullptr).bytes;
}

hipError_t fgr_rows(m3d_ctx* ctx, const double* src, int64_t ns, const double* tgt, int64_t nt,
                    const int32_t* corr, int64_t nc, const m3d_fgr_params* p, m3d_fgr_result* out,
                    int32_t* rows_out, void* scratch, hipStream_t st, int* bad_row) {
  const int64_t cap = fgr_tuple_cap(p, nc);
  const FgrScratch L(ns, nt, nc, cap, scratch);
  FgrState* s = L.state;
  double *mpart = L.mpart, *pr = L.pr, *qr = L.qr, *pp = L.p, *qq = L.q;
  uint8_t* flag = L.flag;
  int64_t *sel = L.sel, *accepted = L.accepted;
  int32_t* nsel = L.nsel;
  *bad_row = 0;
  hipError_t e;
  {  // step 2 (ns, nt ≥ 1)
    KTimer t(ctx, M3D_KERNEL_TERMS, st);
    fgr_init_kernel<<<1, kMultiBlock, 0, st>>>(s);
    for (int which = 0; which < 2; ++which) {
      const double* xyz = which ? tgt : src;
      const int64_t n = which ? nt : ns;
      const int64_t nseg = segs_of(n);
      const unsigned wb = (unsigned)((nseg + kMultiBlock / kWave - 1) / (kMultiBlock / kWave));
      fgr_mean_partial_kernel<<<wb, kMultiBlock, 0, st>>>(xyz, n, nseg, mpart);
      fgr_mean_final_kernel<<<1, kWave, 0, st>>>(mpart, nseg, n, s, which);
      const unsigned mb = (unsigned)std::min<int64_t>(1024, (n + kMultiBlock - 1) / kMultiBlock);
      fgr_maxnorm_kernel<<<mb, kMultiBlock, 0, st>>>(xyz, n, s, which);
    }
    fgr_scale_kernel<<<1, 1, 0, st>>>(s, p->use_absolute_scale ? 1 : 0);
    if (nc > 0)
      fgr_gather_kernel<<<(unsigned)((nc + kMultiBlock - 1) / kMultiBlock), kMultiBlock, 0, st>>>(src, ns, tgt, nt, corr,
                                                                                                   nc, s, pr, qr);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  FgrState hs;
  if (p->tuple_test && nc > 0) {  // step 3
    if ((e = read_state(s, &hs, st)) != hipSuccess) return e;  // (no trial reads a point of a bad row)
    if (hs.bad) {
      *bad_row = 1;
      return hipSuccess;
    }
    KTimer t(ctx, M3D_KERNEL_SCORE, st);
    const int64_t trials = 100 * nc;
    int64_t h0 = 0;
    for (int64_t group = 1; h0 < trials; group *= 2) {
      for (int64_t b = 0; b < group && h0 < trials; ++b, h0 += kFgrTrialBatch) {
        const int count = (int)std::min<int64_t>(kFgrTrialBatch, trials - h0);
        fgr_tuple_flag_kernel<<<(unsigned)((count + kMultiBlock - 1) / kMultiBlock), kMultiBlock, 0, st>>>(
            pr, qr, nc, p->seed, h0, count, p->tuple_scale, flag, s);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        size_t tb = L.tmp_bytes;
        e = hipcub::DeviceSelect::Flagged(L.tmp, tb, hipcub::CountingInputIterator<int64_t>(h0), flag, sel, nsel,
                                          count, st);
        if (e != hipSuccess) return e;
        fgr_tuple_append_kernel<<<1, kMultiBlock, 0, st>>>(sel, nsel, cap, accepted, h0 + count, s);
        if ((e = hipGetLastError()) != hipSuccess) return e;
      }
      if (h0 >= trials) break;
      int32_t done = 0;
      if ((e = hipMemcpyAsync(&done, &s->done, sizeof(done), hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
      if ((e = hipStreamSynchronize(st)) != hipSuccess) return e;
      if (done) break;
    }
    fgr_tuple_rows_kernel<<<(unsigned)((cap + kMultiBlock - 1) / kMultiBlock), kMultiBlock, 0, st>>>(
        pr, qr, corr, nc, p->seed, accepted, s, pp, qq, rows_out);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  } else if (nc > 0) {
    if ((e = hipMemcpyAsync(pp, pr, sizeof(double) * 3 * (size_t)nc, hipMemcpyDeviceToDevice, st)) != hipSuccess) return e;
    if ((e = hipMemcpyAsync(qq, qr, sizeof(double) * 3 * (size_t)nc, hipMemcpyDeviceToDevice, st)) != hipSuccess) return e;
    if (rows_out != nullptr &&
        (e = hipMemcpyAsync(rows_out, corr, sizeof(int32_t) * 2 * (size_t)nc, hipMemcpyDeviceToDevice, st)) != hipSuccess)
      return e;
  }
  if ((e = read_state(s, &hs, st)) != hipSuccess) return e;
  if (hs.bad) {
    *bad_row = 1;
    return hipSuccess;
  }
  out->n_input = nc;
  out->tuples = p->tuple_test ? hs.accepted : 0;
  out->trials = p->tuple_test ? hs.trials : 0;
  out->n_rows = p->tuple_test ? 3 * (int64_t)hs.accepted : nc;
  out->scale_global = hs.g;
  out->par_final = hs.par0;
  for (int a = 0; a < 3; ++a) {
    out->mean_src[a] = hs.mean[0][a];
    out->mean_tgt[a] = hs.mean[1][a];
  }
  return hipSuccess;
}

namespace {
// path: 0 auto, 1 one workgroup, 2 multi-block (the caller has checked that 1 fits)
hipError_t run_loop(m3d_ctx* ctx, const double* p, double* q, int64_t n, const LoopArgs& a, int path, double* part,
                    FgrState* s, hipStream_t st) {
  KTimer t(ctx, M3D_KERNEL_LOOP, st);
  if (path == 1 || (path == 0 && n <= kFgrOneWgRows)) {
    fgr_loop_one_kernel<<<1, kOneWgThreads, 0, st>>>(p, q, (int)n, a, 0, 0.0, s);
    return hipGetLastError();
  }
  const int64_t nseg = segs_of(n);
  const unsigned blocks = (unsigned)((nseg + kMultiBlock / kWave - 1) / (kMultiBlock / kWave));
  for (int itr = 0; itr < a.iters; ++itr)
    fgr_loop_multi_kernel<<<blocks, kMultiBlock, 0, st>>>(p, q, n, nseg, itr, a, 0, 0.0, part, s);
  return hipGetLastError();
}
}  // namespace

hipError_t fgr_optimise(m3d_ctx* ctx, int64_t ns, int64_t nt, int64_t nc, const m3d_fgr_params* p,
                        m3d_fgr_result* out, void* scratch, hipStream_t st) {
  const FgrScratch L(ns, nt, nc, fgr_tuple_cap(p, nc), scratch);
  FgrState* s = L.state;
  const int64_t n = out->n_rows;
  for (int k = 0; k < 16; ++k) out->T_norm[k] = (k % 5 == 0) ? 1.0 : 0.0;
  if (n < 10 || p->iteration_number <= 0) return hipSuccess;  // T = I, par = par₀
  const LoopArgs a{p->iteration_number, p->decrease_mu ? 1 : 0, p->maximum_correspondence_distance, p->division_factor};
  hipError_t e = run_loop(ctx, L.p, L.q, n, a, p->path, L.lpart, s, st);
  if (e != hipSuccess) return e;
  FgrState hs;
  if ((e = read_state(s, &hs, st)) != hipSuccess) return e;
  for (int k = 0; k < 16; ++k) out->T_norm[k] = hs.T[k];
  out->par_final = hs.par;
  return hipSuccess;
}

size_t fgr_terms_scratch_bytes(int64_t n) { return FgrTermsScratch(n, nullptr).bytes; }

hipError_t fgr_terms(m3d_ctx* ctx, const double* p, const double* q, int64_t n, double par, int path,
                     double sums27[27], void* scratch, hipStream_t st) {
  const FgrTermsScratch L(n, scratch);
  FgrState* s = L.state;
  double* part = L.part;
  const LoopArgs a{1, 0, 0.0, 1.0};
  fgr_init_kernel<<<1, kMultiBlock, 0, st>>>(s);
  {
    KTimer t(ctx, M3D_KERNEL_TERMS, st);
    if (path == 1 || (path == 0 && n <= kFgrOneWgRows)) {
      fgr_loop_one_kernel<<<1, kOneWgThreads, 0, st>>>(p, q, (int)n, a, 1, par, s);
    } else {
      const int64_t nseg = segs_of(n);
      const unsigned blocks = (unsigned)((nseg + kMultiBlock / kWave - 1) / (kMultiBlock / kWave));
      // (sums_only never writes q)
      fgr_loop_multi_kernel<<<blocks, kMultiBlock, 0, st>>>(p, const_cast<double*>(q), n, nseg, 0, a, 1, par, part, s);
    }
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  FgrState hs;
  if ((e = read_state(s, &hs, st)) != hipSuccess) return e;
  fgr_expand_sums(hs.sums, sums27);
  return hipSuccess;
}

}  // namespace m3d
