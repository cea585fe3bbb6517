// robust.hip — Open3D's robust kernels (Open3D 0.19 RobustKernel.cpp) inside the point-to-plane
// and the Generalized ICP estimators: terms passes of their own beside the RegistrationICP loop's
// NN scan and solve, as gicp.hip's — three launches per iteration (scan, terms + reduce, solve).
// Only a call that names a kernel other than L2 reaches this file (and m3d_robust_terms, which
// runs L2 through it too: the check of this pass against the point-to-plane oracle); the fused
// point-to-plane tail (icp.hip) and gicp_terms_kernel are what a call without a kernel runs.
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
// Everything else is the loop's: slot_winner (nnkey.h) opens both kernels, the moved point (and
// the rotated covariance, in gicp_terms_kernel's own operation order) and corr are written back,
// the 30 values per thread go through block_partial and launch_reduce in the loop's fixed order
// (two runs, and the brute-force and grid scans, give the same bits), slots 0..20 JᵀJ (upper,
// row-major), 21..26 Jᵀr, 27 Σr², 28 count, 29 Σd².
//
// Bytes per source a pass must move.  Point-to-plane: the point read and written (24 + 24), key,
// runner-up and correspondence (8 + 4 + 4), the winner's point and normal (24 + 24): 112 B.
// Generalized ICP: gicp.hip's 232 B.
#include "linalg.h"
#include "m3d_internal.h"
#include "nnkey.h"
#include "robust_rows.h"

namespace m3d {

namespace {

constexpr int kRobustBlock = 256;

// ns > 0 and nt > 0 (the launchers keep the empty cases away: no slot 0, no target 0 to load)
template <int K>
__global__ __launch_bounds__(kRobustBlock) void robust_plane_terms_kernel(
    double* __restrict__ pcd64, const float4* __restrict__ src32, int64_t ns, const double* __restrict__ tgt64,
    const double* __restrict__ nrm_t, int64_t nt, GridDev g, const IcpState* __restrict__ s,
    const int64_t* __restrict__ keys, const uint32_t* __restrict__ near2, int32_t* __restrict__ corr, double kk,
    double* __restrict__ partials) {
  if (s->done) return;
  const SlotWinner sw = slot_winner((int64_t)blockIdx.x * kRobustBlock + threadIdx.x, pcd64, src32, ns, tgt64, nt, g,
                                    s, keys, near2);
  const double(&Q)[3] = sw.Q;
  if (sw.valid) {
#pragma unroll
    for (int k = 0; k < 3; ++k) pcd64[3 * sw.i + k] = Q[k];
    corr[sw.i] = sw.hit ? (int32_t)sw.gj : -1;
  }
  double v[kRobustUsed];
#pragma unroll
  for (int k = 0; k < kRobustUsed; ++k) v[k] = 0.0;
  if (sw.hit) {
    const double* tq = tgt64 + 3 * sw.gj;
    const double* tn = nrm_t + 3 * sw.gj;
    const double nx = tn[0], ny = tn[1], nz = tn[2];
    const double x = Q[0], y = Q[1], z = Q[2];
    const double r = ((x - tq[0]) * nx + (y - tq[1]) * ny) + (z - tq[2]) * nz;
    const double J[6] = {y * nz - z * ny, z * nx - x * nz, x * ny - y * nx, nx, ny, nz};
    add_row(v, J, r, robust_weight<K>(r, kk));
    v[28] = 1.0;
    v[29] = sw.d;
  }
  block_partial<kTermSlots, kRobustUsed, kRobustBlock>(v, partials);
}

template <int K>
__global__ __launch_bounds__(kRobustBlock) void robust_gicp_terms_kernel(
    double* __restrict__ pcd64, double* __restrict__ cov_s, const float4* __restrict__ src32, int64_t ns,
    const double* __restrict__ tgt64, const double* __restrict__ cov_t, int64_t nt, GridDev g,
    const IcpState* __restrict__ s, const int64_t* __restrict__ keys, const uint32_t* __restrict__ near2,
    int32_t* __restrict__ corr, double kk, double* __restrict__ partials) {
  if (s->done) return;
  const SlotWinner sw = slot_winner((int64_t)blockIdx.x * kRobustBlock + threadIdx.x, pcd64, src32, ns, tgt64, nt, g,
                                    s, keys, near2);
  const int64_t i = sw.i;
  const double(&Q)[3] = sw.Q;
  // Cs ← R·Cs·Rᵀ in gicp_terms_kernel's order: A = R·Cs, then the upper triangle of A·Rᵀ
  double Cs[6];
  {
    const double* T = s->dT;
    const double* c = cov_s + 6 * i;
    const double R[3][3] = {{T[0], T[1], T[2]}, {T[4], T[5], T[6]}, {T[8], T[9], T[10]}};
    const double C[3][3] = {{c[0], c[1], c[2]}, {c[1], c[3], c[4]}, {c[2], c[4], c[5]}};
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
  if (sw.valid) {
#pragma unroll
    for (int k = 0; k < 3; ++k) pcd64[3 * i + k] = Q[k];
#pragma unroll
    for (int k = 0; k < 6; ++k) cov_s[6 * i + k] = Cs[k];
    corr[i] = sw.hit ? (int32_t)sw.gj : -1;
  }
  double v[kRobustUsed];
#pragma unroll
  for (int k = 0; k < kRobustUsed; ++k) v[k] = 0.0;
  if (sw.hit) {
    const double* tq = tgt64 + 3 * sw.gj;
    const double* ct = cov_t + 6 * sw.gj;
    const double d0 = Q[0] - tq[0], d1 = Q[1] - tq[1], d2 = Q[2] - tq[2];
    const double M[6] = {ct[0] + Cs[0], ct[1] + Cs[1], ct[2] + Cs[2], ct[3] + Cs[3], ct[4] + Cs[4], ct[5] + Cs[5]};
    double W[6];
    sym3_inv_sqrt(M, W);
    const double x = Q[0], y = Q[1], z = Q[2];
    const double rows[3][3] = {{W[0], W[1], W[2]}, {W[1], W[3], W[4]}, {W[2], W[4], W[5]}};
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const double g0 = rows[j][0], g1 = rows[j][1], g2 = rows[j][2];
      const double r = (g0 * d0 + g1 * d1) + g2 * d2;
      // W.row(j)·J₀: column a < 3 of J₀ is e_a × vs
      const double J[6] = {y * g2 - z * g1, z * g0 - x * g2, x * g1 - y * g0, g0, g1, g2};
      add_row(v, J, r, robust_weight<K>(r, kk));
    }
    v[28] = 1.0;
    v[29] = sw.d;
  }
  block_partial<kTermSlots, kRobustUsed, kRobustBlock>(v, partials);
}

}  // namespace

int64_t robust_blocks(int64_t ns) { return ns > 0 ? (ns + kRobustBlock - 1) / kRobustBlock : 0; }

// The robust point-to-plane terms of the loop's current evaluation (its NN scan must have been
// enqueued on st) and their reduction into sums, as launch_gicp_terms.  partials:
// robust_blocks(ns) × kTermSlots doubles; the target has normals (icp_create's check).
hipError_t launch_robust_plane_terms(const m3d_icp* s, int32_t kind, double k, double* partials, double* sums,
                                     bool with_defer, hipStream_t st) {
  const int64_t ns = s->src->n, nt = s->tgt->n;
  const int64_t nb = (ns == 0 || nt == 0) ? 0 : robust_blocks(ns);
  if (nb > 0)
    with_kind(kind, [&](auto K) {
      robust_plane_terms_kernel<decltype(K)::value><<<(unsigned)nb, kRobustBlock, 0, st>>>(
          s->pcd64, s->src->xyz32, ns, s->tgt->xyz64, s->tgt->nrm64, nt, s->tgrid->dev, s->state, s->keys, s->near2,
          s->corr, k, partials);
    });
  return launch_reduce(partials, nb, kTermSlots, sums, s->state, with_defer ? s->hcnt : nullptr, st);
}

// The same for Generalized ICP; cov_s / cov_t / partials as launch_gicp_terms takes them
hipError_t launch_robust_gicp_terms(const m3d_icp* s, int32_t kind, double k, double* cov_s, const double* cov_t,
                                    double* partials, double* sums, bool with_defer, hipStream_t st) {
  const int64_t ns = s->src->n, nt = s->tgt->n;
  const int64_t nb = (ns == 0 || nt == 0) ? 0 : robust_blocks(ns);
  if (nb > 0)
    with_kind(kind, [&](auto K) {
      robust_gicp_terms_kernel<decltype(K)::value><<<(unsigned)nb, kRobustBlock, 0, st>>>(
          s->pcd64, cov_s, s->src->xyz32, ns, s->tgt->xyz64, cov_t, nt, s->tgrid->dev, s->state, s->keys, s->near2,
          s->corr, k, partials);
    });
  return launch_reduce(partials, nb, kTermSlots, sums, s->state, with_defer ? s->hcnt : nullptr, st);
}

}  // namespace m3d
