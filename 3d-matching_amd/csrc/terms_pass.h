// terms_pass.h — the skeleton of a side terms pass: a terms pass of its own beside the
// RegistrationICP loop's NN scan and solve (three launches per iteration: scan, terms + reduce,
// solve), as Generalized ICP (gicp.hip), the robust kernels (robust.hip) and Colored ICP
// (colored.hip) run one.  Everything such a pass shares is here, once; a translation unit adds its
// estimator, a small functor passed to the kernel by value.
//
// One evaluation, source slot i (side_terms_kernel, in this order):
//   the `done` return; nnkey.h slot_winner (Q = dT·p, the winner gj, its fp64 d², valid, hit);
//   est.prepare — every lane, valid or not, a lane past ns with slot 0's loads (no early return
//   before block_partial); valid: Q, the estimator's own state and corr written back
//   (pcd.Transform(update) moves the source); the 30 values zeroed; hit: est.rows, then slot 28 += 1
//   and slot 29 += d²; nnkey.h block_partial.  launch_side_terms adds launch_reduce over the block
//   partials: the loop's fixed order, so two runs, and the brute-force and grid scans, give the
//   same bits.  Slots: 0..20 JᵀJ (upper, row-major), 21..26 Jᵀr, 27 Σr², 28 count, 29 Σd² — icp.hip's
//   point-to-plane layout, so launch_icp_solve consumes the sums unchanged.
//
// An estimator Est is trivially copyable and has
//   Slot                                   its per-slot state (NoSlot: none)
//   Slot prepare(const double* dT, i)      the state of slot i under the evaluation's transform
//   void write_back(i, const Slot&)        that state stored (valid lanes only)
//   void rows(v, sw, tq, const Slot&)      the matched pair's terms added to v[0 .. 28); tq = the
//                                          winner's point
// Pointer members are __restrict__: as kernel parameters they were, and the code generated from
// them is to stay what it was.
//
// Also here, for the estimators that weight their rows (robust.hip, colored.hip): the weight of a
// residual, the weighted row added to the 30 sums, and the dispatch on a checked kernel kind.  The
// operation order of each is stated in robust.hip's header.
#pragma once

#include <type_traits>

#include "m3d_internal.h"
#include "nnkey.h"

namespace m3d {

constexpr int kTermsUsed = 30;

// the loop fields every side terms pass receives
struct TermsLoop {
  double* __restrict__ pcd64;
  const float4* __restrict__ src32;
  int64_t ns;
  const double* __restrict__ tgt64;
  int64_t nt;
  GridDev g;
  const IcpState* __restrict__ state;
  const int64_t* __restrict__ keys;
  const uint32_t* __restrict__ near2;
  int32_t* __restrict__ corr;
};
inline TermsLoop terms_loop_of(const m3d_icp* s) {
  return {s->pcd64, s->src->xyz32, s->src->n, s->tgt->xyz64, s->tgt->n,
          s->tgrid->dev, s->state, s->keys, s->near2, s->corr};
}

// an estimator without per-slot state derives from this
struct NoSlot {};
struct NoSlotState {
  using Slot = NoSlot;
  __device__ __forceinline__ Slot prepare(const double*, int64_t) const { return {}; }
  __device__ __forceinline__ void write_back(int64_t, const Slot&) const {}
};

// Cs ← R·Cs·Rᵀ (R = T's rotation; covariances as upper triangles, gicp.hip): A = R·Cs, then the
// upper triangle of A·Rᵀ
__device__ __forceinline__ void rotate_cov6(const double* __restrict__ T, const double (&cs)[6], double (&Cs)[6]) {
  const double R[3][3] = {{T[0], T[1], T[2]}, {T[4], T[5], T[6]}, {T[8], T[9], T[10]}};
  const double C[3][3] = {{cs[0], cs[1], cs[2]}, {cs[1], cs[3], cs[4]}, {cs[2], cs[4], cs[5]}};
  double A[3][3];
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) A[a][b] = (R[a][0] * C[0][b] + R[a][1] * C[1][b]) + R[a][2] * C[2][b];
  int k = 0;
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = a; b < 3; ++b) Cs[k++] = (A[a][0] * R[b][0] + A[a][1] * R[b][1]) + A[a][2] * R[b][2];
}

// the per-slot state of the two Generalized ICP estimators: the source covariance, rotated in
// place by every evaluation.  cov_s: the loop's source covariances in slot order, cov_t: the
// target's in index order, 6 doubles per point
struct CovState {
  double* __restrict__ cov_s;
  const double* __restrict__ cov_t;
  struct Slot {
    double Cs[6];
  };
  __device__ __forceinline__ Slot prepare(const double* __restrict__ dT, int64_t i) const {
    double cs[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) cs[k] = cov_s[6 * i + k];
    Slot o;
    rotate_cov6(dT, cs, o.Cs);
    return o;
  }
  __device__ __forceinline__ void write_back(int64_t i, const Slot& o) const {
#pragma unroll
    for (int k = 0; k < 6; ++k) cov_s[6 * i + k] = o.Cs[k];
  }
};

// ns > 0 and nt > 0 (launch_side_terms keeps the empty cases away: no slot 0, no target 0 to load)
template <class Est>
__global__ __launch_bounds__(kSideBlock) void side_terms_kernel(TermsLoop L, Est est, double* __restrict__ partials) {
  const IcpState* __restrict__ s = L.state;
  if (s->done) return;
  const SlotWinner sw = slot_winner((int64_t)blockIdx.x * kSideBlock + threadIdx.x, L.pcd64, L.src32, L.ns, L.tgt64,
                                    L.nt, L.g, s, L.keys, L.near2);
  const typename Est::Slot own = est.prepare(s->dT, sw.i);
  if (sw.valid) {
#pragma unroll
    for (int k = 0; k < 3; ++k) L.pcd64[3 * sw.i + k] = sw.Q[k];
    est.write_back(sw.i, own);
    L.corr[sw.i] = sw.hit ? (int32_t)sw.gj : -1;
  }
  double v[kTermsUsed];
#pragma unroll
  for (int k = 0; k < kTermsUsed; ++k) v[k] = 0.0;
  if (sw.hit) {
    est.rows(v, sw, L.tgt64 + 3 * sw.gj, own);
    v[28] = 1.0;
    v[29] = sw.d;
  }
  block_partial<kTermSlots, kTermsUsed, kSideBlock>(v, partials);
}

// The estimator's terms of the loop's current evaluation (its NN scan must have been enqueued on
// st) and their reduction into sums (kTermSlots doubles).  partials: side_terms_blocks(ns) ×
// kTermSlots doubles.  sums[0 .. 30) = the sums over the partials (no blocks: zeros), all the
// solve reads; with_defer: the last two words carry the grid scan's deferral count and fault word
// (else, and for brute force, zeros), so that a one-evaluation call gets its result and the fault
// word in one read.
template <class Est>
hipError_t launch_side_terms(const m3d_icp* s, Est est, double* partials, double* sums, bool with_defer,
                             hipStream_t st) {
  static_assert(std::is_trivially_copyable<Est>::value, "an estimator travels as a kernel argument");
  const int64_t ns = s->src->n, nt = s->tgt->n;
  const int64_t nb = (ns == 0 || nt == 0) ? 0 : side_terms_blocks(ns);
  if (nb > 0) side_terms_kernel<Est><<<(unsigned)nb, kSideBlock, 0, st>>>(terms_loop_of(s), est, partials);
  return launch_reduce(partials, nb, kTermSlots, sums, s->state, with_defer ? s->hcnt : nullptr, st);
}

template <int K>
__device__ __forceinline__ double robust_weight(double r, double k) {
  if (K == M3D_KERNEL_L1) return 1.0 / fabs(r);
  if (K == M3D_KERNEL_HUBER) return k / fmax(fabs(r), k);
  if (K == M3D_KERNEL_CAUCHY) return 1.0 / (1.0 + (r / k) * (r / k));
  if (K == M3D_KERNEL_GM) return k / ((k + r * r) * (k + r * r));
  if (K == M3D_KERNEL_TUKEY) {
    const double t = fmin(1.0, fabs(r / k));
    const double u = 1.0 - t * t;
    return u * u;
  }
  return 1.0;
}

// v += the weighted row (J, r)
__device__ __forceinline__ void add_row(double (&v)[kTermsUsed], const double (&J)[6], double r, double w) {
  int k = 0;
#pragma unroll
  for (int a = 0; a < 6; ++a) {
    const double wa = w * J[a];
#pragma unroll
    for (int c = a; c < 6; ++c) v[k++] += wa * J[c];
    v[21 + a] += wa * r;
  }
  v[27] += r * r;
}

// f(integral_constant<int, kind>) for a checked kind
template <class F>
void with_kind(int32_t kind, F f) {
  switch (kind) {
    case M3D_KERNEL_L1: f(std::integral_constant<int, M3D_KERNEL_L1>{}); break;
    case M3D_KERNEL_HUBER: f(std::integral_constant<int, M3D_KERNEL_HUBER>{}); break;
    case M3D_KERNEL_CAUCHY: f(std::integral_constant<int, M3D_KERNEL_CAUCHY>{}); break;
    case M3D_KERNEL_GM: f(std::integral_constant<int, M3D_KERNEL_GM>{}); break;
    case M3D_KERNEL_TUKEY: f(std::integral_constant<int, M3D_KERNEL_TUKEY>{}); break;
    default: f(std::integral_constant<int, M3D_KERNEL_L2>{}); break;
  }
}

}  // namespace m3d
