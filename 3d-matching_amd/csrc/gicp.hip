// gicp.hip — Generalized ICP (Open3D 0.19 GeneralizedICP.cpp, plane-to-plane): per-point
// covariances from normals, and the terms pass that replaces icp.hip's point-to-plane terms in the
// RegistrationICP loop.  The NN scan before it, the solve after it (icp.hip solve_state, the
// point-to-plane slot layout) and the convergence rule are the loop's own.
//
// Covariance of a point with unit normal n (InitializePointCloudForGeneralizedICP):
//   C = Rx·diag(ε, 1, 1)·Rxᵀ,  Rx = GetRotationFromE1ToX(n):  v = e1 × n = (0, −nz, ny), c = nx,
//   Rx = I when c < −0.99, else I + [v]× + [v]×²·(1 / (1 + c)).
// Every covariance is held as its upper triangle, 6 doubles (xx, xy, xz, yy, yz, zz): the lower
// one is its mirror by definition, so a covariance is symmetric in every bit.
//
// One evaluation, source slot i (its point p, covariance Cs; dT = the transform the evaluation
// applies, IcpState::dT — the init, then each update):
//   vs = dT·p (nnkey.h q64_of), Cs ← R·Cs·Rᵀ (R = dT's rotation), both written back
//   (pcd.Transform(update) moves points and covariances); winner t = nnkey.h winner_fp64;
//   d = vs − vt, M = Ct + Cs, B = M⁻¹ (closed form: cofactors over the determinant),
//   J₀ = [−[vs]× | I] (3×6):  JᵀJ += J₀ᵀ·B·J₀, Jᵀr += J₀ᵀ·B·d, Σr² += dᵀ·B·d, count += 1, Σd² += d².
// With unit weights this equals Open3D's rows W·d, W·J₀ with W = M^(−1/2): no square root needed.
// Slots: 0..20 JᵀJ (upper, row-major), 21..26 Jᵀr, 27 Σr², 28 count, 29 Σd² — icp.hip's
// point-to-plane layout, so launch_icp_solve consumes the sums unchanged.
//
// Order of summation: the loop's fixed order (icp.hip, "reduce"; nnkey.h block_partial per block
// of 256 consecutive slots, launch_reduce over the block partials) — two runs, and the brute-force
// and grid scans, give the same bits.
//
// Bytes per source the terms pass must move: its point read and written (24 + 24), its
// covariance read and written (48 + 48), key, runner-up and correspondence (8 + 4 + 4), and the
// gathered winner's point and covariance (24 + 48): 232 B.
#include "m3d_internal.h"
#include "nnkey.h"

namespace m3d {

constexpr int kGicpBlock = 256;
constexpr int kGicpUsed = 30;

// upper triangle of Rx·diag(ε, 1, 1)·Rxᵀ for the normal (nx, ny, nz)
__device__ __forceinline__ void cov6_of_normal(double nx, double ny, double nz, double eps, double (&C)[6]) {
  double R[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
  if (!(nx < -0.99)) {
    const double f = 1.0 / (1.0 + nx);
    // [v]× = [[0, −ny, −nz], [ny, 0, 0], [nz, 0, 0]],  [v]×² = [[−(ny² + nz²), 0, 0], [0, −ny², −ny·nz], [0, −ny·nz, −nz²]]
    R[0][0] = 1.0 - (ny * ny + nz * nz) * f;
    R[0][1] = -ny;
    R[0][2] = -nz;
    R[1][0] = ny;
    R[1][1] = 1.0 - (ny * ny) * f;
    R[1][2] = -((ny * nz) * f);
    R[2][0] = nz;
    R[2][1] = -((ny * nz) * f);
    R[2][2] = 1.0 - (nz * nz) * f;
  }
  int k = 0;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = i; j < 3; ++j) C[k++] = ((eps * R[i][0]) * R[j][0] + R[i][1] * R[j][1]) + R[i][2] * R[j][2];
}

// width 9: the full row-major 3×3 (m3d_covariances_from_normals); width 6: the upper triangle
__global__ __launch_bounds__(256) void cov_from_normals_kernel(const double* __restrict__ nrm, int64_t n,
                                                               double eps, double* __restrict__ out, int width) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double C[6];
  cov6_of_normal(nrm[3 * i], nrm[3 * i + 1], nrm[3 * i + 2], eps, C);
  if (width == 6) {
#pragma unroll
    for (int k = 0; k < 6; ++k) out[6 * i + k] = C[k];
  } else {
    double* o = out + 9 * i;
    o[0] = C[0];
    o[1] = o[3] = C[1];
    o[2] = o[6] = C[2];
    o[4] = C[3];
    o[5] = o[7] = C[4];
    o[8] = C[5];
  }
}

// out6[k] = the upper triangle of the caller's row-major 3×3 of point slot[k] (slot null: k)
__global__ __launch_bounds__(256) void cov_pack_kernel(const double* __restrict__ cov9,
                                                       const int32_t* __restrict__ slot, int64_t n,
                                                       double* __restrict__ out6) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= n) return;
  const double* c = cov9 + 9 * (slot != nullptr ? (int64_t)slot[k] : k);
  double* o = out6 + 6 * k;
  o[0] = c[0];
  o[1] = c[1];
  o[2] = c[2];
  o[3] = c[4];
  o[4] = c[5];
  o[5] = c[8];
}

// (J₀[:, a])·g for a 3-vector g: a < 3 the column (e_a × vs), i.e. (vs × g)_a; a ≥ 3 the unit column
template <int a>
__device__ __forceinline__ double j0_dot(double x, double y, double z, const double (&g)[3]) {
  if (a == 0) return y * g[2] - z * g[1];
  if (a == 1) return z * g[0] - x * g[2];
  if (a == 2) return x * g[1] - y * g[0];
  return g[a >= 3 ? a - 3 : 0];
}

// slot of JᵀJ[a][c], a ≤ c, in the upper row-major layout
constexpr int jtj_slot(int a, int c) { return a * 6 - a * (a - 1) / 2 + (c - a); }

template <int a, int c>
__device__ __forceinline__ void jtj_row(double (&v)[kGicpUsed], double x, double y, double z,
                                        const double (&G)[6][3]) {
  if constexpr (c < 6) {
    v[jtj_slot(a, c)] = j0_dot<a>(x, y, z, G[c]);
    jtj_row<a, c + 1>(v, x, y, z, G);
  }
}
template <int a>
__device__ __forceinline__ void jtj_rows(double (&v)[kGicpUsed], double x, double y, double z,
                                         const double (&G)[6][3], const double (&w)[3]) {
  if constexpr (a < 6) {
    jtj_row<a, a>(v, x, y, z, G);
    v[21 + a] = j0_dot<a>(x, y, z, w);
    jtj_rows<a + 1>(v, x, y, z, G, w);
  }
}

// ns > 0 and nt > 0 (launch_gicp_terms keeps the empty cases away: no slot 0, no target 0 to load)
__global__ __launch_bounds__(kGicpBlock) void gicp_terms_kernel(
    double* __restrict__ pcd64, double* __restrict__ cov_s, const float4* __restrict__ src32, int64_t ns,
    const double* __restrict__ tgt64, const double* __restrict__ cov_t, int64_t nt, GridDev g,
    const IcpState* __restrict__ s, const int64_t* __restrict__ keys, const uint32_t* __restrict__ near2,
    int32_t* __restrict__ corr, double* __restrict__ partials) {
  if (s->done) return;
  const SlotWinner sw = slot_winner((int64_t)blockIdx.x * kGicpBlock + threadIdx.x, pcd64, src32, ns, tgt64, nt, g, s,
                                    keys, near2);
  const bool valid = sw.valid, hit = sw.hit;
  const int64_t i = sw.i, gj = sw.gj;
  const double(&Q)[3] = sw.Q;
  // Cs ← R·Cs·Rᵀ: A = R·Cs, then the upper triangle of A·Rᵀ
  double cs[6], Cs[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) cs[k] = cov_s[6 * i + k];
  {
    const double* T = s->dT;
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
  if (valid) {
#pragma unroll
    for (int k = 0; k < 3; ++k) pcd64[3 * i + k] = Q[k];
#pragma unroll
    for (int k = 0; k < 6; ++k) cov_s[6 * i + k] = Cs[k];
  }
  if (valid) corr[i] = hit ? (int32_t)gj : -1;
  double v[kGicpUsed];
#pragma unroll
  for (int k = 0; k < kGicpUsed; ++k) v[k] = 0.0;
  if (hit) {
    const double* tq = tgt64 + 3 * gj;
    const double* ct = cov_t + 6 * gj;
    const double d[3] = {Q[0] - tq[0], Q[1] - tq[1], Q[2] - tq[2]};
    const double ma = ct[0] + Cs[0], mb = ct[1] + Cs[1], mc = ct[2] + Cs[2];
    const double md = ct[3] + Cs[3], me = ct[4] + Cs[4], mf = ct[5] + Cs[5];
    // M⁻¹ = cofactors / det (M symmetric positive definite)
    const double c00 = md * mf - me * me, c01 = mc * me - mb * mf, c02 = mb * me - mc * md;
    const double c11 = ma * mf - mc * mc, c12 = mb * mc - ma * me, c22 = ma * md - mb * mb;
    const double rdet = 1.0 / ((ma * c00 + mb * c01) + mc * c02);
    const double b00 = c00 * rdet, b01 = c01 * rdet, b02 = c02 * rdet;
    const double b11 = c11 * rdet, b12 = c12 * rdet, b22 = c22 * rdet;
    const double x = Q[0], y = Q[1], z = Q[2];
    // G[c] = B·J₀[:, c]
    const double G[6][3] = {{y * b02 - z * b01, y * b12 - z * b11, y * b22 - z * b12},
                            {z * b00 - x * b02, z * b01 - x * b12, z * b02 - x * b22},
                            {x * b01 - y * b00, x * b11 - y * b01, x * b12 - y * b02},
                            {b00, b01, b02},
                            {b01, b11, b12},
                            {b02, b12, b22}};
    const double w[3] = {(b00 * d[0] + b01 * d[1]) + b02 * d[2], (b01 * d[0] + b11 * d[1]) + b12 * d[2],
                         (b02 * d[0] + b12 * d[1]) + b22 * d[2]};
    jtj_rows<0>(v, x, y, z, G, w);
    v[27] = (d[0] * w[0] + d[1] * w[1]) + d[2] * w[2];
    v[28] = 1.0;
    v[29] = sw.d;
  }
  block_partial<kTermSlots, kGicpUsed, kGicpBlock>(v, partials);
}

int64_t gicp_blocks(int64_t ns) { return ns > 0 ? (ns + kGicpBlock - 1) / kGicpBlock : 0; }

hipError_t launch_cov_from_normals(const double* nrm, int64_t n, double eps, double* out, int width,
                                   hipStream_t st) {
  if (n == 0) return hipSuccess;
  cov_from_normals_kernel<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(nrm, n, eps, out, width);
  return hipGetLastError();
}

hipError_t launch_cov_pack(const double* cov9, const int32_t* slot, int64_t n, double* out6, hipStream_t st) {
  if (n == 0) return hipSuccess;
  cov_pack_kernel<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(cov9, slot, n, out6);
  return hipGetLastError();
}

// The plane-to-plane terms of the loop's current evaluation (its NN scan must have been enqueued
// on st) and their reduction into sums (kTermSlots doubles).  cov_s: the loop's source covariances
// in slot order, 6 per point, rotated in place; cov_t: the target's in index order; partials:
// gicp_blocks(ns) × kTermSlots doubles.  sums[0 .. 30) = the sums over the partials (no blocks:
// zeros), all the solve reads; with_defer: the last two words carry the grid scan's deferral count
// and fault word (else, and for brute force, zeros), so that a one-evaluation call gets its result
// and the fault word in one read.
hipError_t launch_gicp_terms(const m3d_icp* s, double* cov_s, const double* cov_t, double* partials,
                             double* sums, bool with_defer, hipStream_t st) {
  const int64_t ns = s->src->n, nt = s->tgt->n;
  const int64_t nb = (ns == 0 || nt == 0) ? 0 : gicp_blocks(ns);
  if (nb > 0)
    gicp_terms_kernel<<<(unsigned)nb, kGicpBlock, 0, st>>>(s->pcd64, cov_s, s->src->xyz32, ns, s->tgt->xyz64,
                                                          cov_t, nt, s->tgrid->dev, s->state, s->keys,
                                                          s->near2, s->corr, partials);
  return launch_reduce(partials, nb, kTermSlots, sums, s->state, with_defer ? s->hcnt : nullptr, st);
}

}  // namespace m3d
