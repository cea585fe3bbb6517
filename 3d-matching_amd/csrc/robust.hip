// robust.hip — Open3D's robust kernels (Open3D 0.19 RobustKernel.cpp) inside the point-to-plane
// and the Generalized ICP estimators: two estimators (RobustPlaneEst, RobustGicpEst) of the side
// terms pass of terms_pass.h, as gicp.hip's.  Only a call that names a kernel other than L2
// reaches this file (and m3d_robust_terms, which runs L2 through it too: the check of this pass
// against the point-to-plane oracle); the fused point-to-plane tail (icp.hip) and gicp.hip's
// GicpEst are what a call without a kernel runs.
//
// Weight w(r) of a residual r, k the kernel's scale, in exactly these fp64 operations:
//   L2      1
//   L1      1 / |r|                         (r = 0: +inf, literally — see below)
//   Huber   k / max(|r|, k)
//   Cauchy  1 / (1 + (r/k)·(r/k))
//   GM      k / ((k + r·r)·(k + r·r))
//   Tukey   (1 − min(1, |r/k|)²)²
//
// A row (J, r) with weight w adds w·J·Jᵀ to JᵀJ, w·J·r to Jᵀr and r·r — unweighted, as Open3D's
// ComputeJTJandJTr — to Σr²; each product is (w·J_a)·J_c, (w·J_a)·r.
//   Point-to-plane, one row per matched pair:  r = (vs − vt)·nt,  J = [vs × nt | nt].
//   Generalized ICP, three rows per matched pair, each weighted on its own:  M = Ct + Cs,
//   W = M^(−1/2) (linalg.h sym3_inv_sqrt: the unit-weight M⁻¹ shortcut of gicp.hip does not
//   apply),  r_j = W.row(j)·d,  J_j = (W·J₀).row(j),  J₀ = [−[vs]× | I],  rows added in the order
//   j = 0, 1, 2.
// A non-finite weight (L1 at r = 0) makes the sums, hence the update, non-finite; the solve
// (icp.hip solve_state) replaces a non-finite update by the identity.
//
// Everything else — the winner, the moved point, the rotated covariance (one rotate_cov6 for this
// file and gicp.hip) and corr written back, the slots and the fixed-order sum — is terms_pass.h's.
//
// Bytes per source a pass must move.  Point-to-plane: the point read and written (24 + 24), key,
// runner-up and correspondence (8 + 4 + 4), the winner's point and normal (24 + 24): 112 B.
// Generalized ICP: gicp.hip's 232 B.
#include "linalg.h"
#include "m3d_internal.h"
#include "nnkey.h"
#include "terms_pass.h"

namespace m3d {

namespace {

// point-to-plane, one weighted row per matched pair
template <int K>
struct RobustPlaneEst : NoSlotState {
  const double* __restrict__ nrm_t;
  double kk;
  __device__ __forceinline__ void rows(double (&v)[kTermsUsed], const SlotWinner& sw, const double* __restrict__ tq,
                                       const Slot&) const {
    const double(&Q)[3] = sw.Q;
    const double* tn = nrm_t + 3 * sw.gj;
    const double nx = tn[0], ny = tn[1], nz = tn[2];
    const double x = Q[0], y = Q[1], z = Q[2];
    const double r = ((x - tq[0]) * nx + (y - tq[1]) * ny) + (z - tq[2]) * nz;
    const double J[6] = {y * nz - z * ny, z * nx - x * nz, x * ny - y * nx, nx, ny, nz};
    add_row(v, J, r, robust_weight<K>(r, kk));
  }
};

// Generalized ICP, three rows per matched pair, each weighted on its own
template <int K>
struct RobustGicpEst : CovState {
  double kk;
  __device__ __forceinline__ void rows(double (&v)[kTermsUsed], const SlotWinner& sw, const double* __restrict__ tq,
                                       const Slot& own) const {
    const double(&Q)[3] = sw.Q;
    const double(&Cs)[6] = own.Cs;
    const double* ct = cov_t + 6 * sw.gj;
    const double d0 = Q[0] - tq[0], d1 = Q[1] - tq[1], d2 = Q[2] - tq[2];
    const double M[6] = {ct[0] + Cs[0], ct[1] + Cs[1], ct[2] + Cs[2], ct[3] + Cs[3], ct[4] + Cs[4], ct[5] + Cs[5]};
    double W[6];
    sym3_inv_sqrt(M, W);
    const double x = Q[0], y = Q[1], z = Q[2];
    const double Wr[3][3] = {{W[0], W[1], W[2]}, {W[1], W[3], W[4]}, {W[2], W[4], W[5]}};
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const double g0 = Wr[j][0], g1 = Wr[j][1], g2 = Wr[j][2];
      const double r = (g0 * d0 + g1 * d1) + g2 * d2;
      // W.row(j)·J₀: column a < 3 of J₀ is e_a × vs
      const double J[6] = {y * g2 - z * g1, z * g0 - x * g2, x * g1 - y * g0, g0, g1, g2};
      add_row(v, J, r, robust_weight<K>(r, kk));
    }
  }
};

}  // namespace

// The robust terms of the loop's current evaluation and their reduction into sums (terms_pass.h
// launch_side_terms); kind: a checked M3D_KERNEL_*, k its scale.  cov_s null: point-to-plane (the
// target has normals: icp_create's check); else Generalized ICP, cov_s / cov_t as
// launch_gicp_terms takes them.
hipError_t launch_robust_terms(const m3d_icp* s, int32_t kind, double k, double* cov_s, const double* cov_t,
                               double* partials, double* sums, bool with_defer, hipStream_t st) {
  hipError_t e = hipSuccess;
  with_kind(kind, [&](auto K) {
    constexpr int kK = decltype(K)::value;
    e = cov_s == nullptr
            ? launch_side_terms(s, RobustPlaneEst<kK>{{}, s->tgt->nrm64, k}, partials, sums, with_defer, st)
            : launch_side_terms(s, RobustGicpEst<kK>{{cov_s, cov_t}, k}, partials, sums, with_defer, st);
  });
  return e;
}

}  // namespace m3d
