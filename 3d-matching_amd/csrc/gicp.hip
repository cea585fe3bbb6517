// gicp.hip — Generalized ICP (Open3D 0.19 GeneralizedICP.cpp, plane-to-plane): per-point
// covariances from normals, and the estimator (GicpEst) of the side terms pass that replaces
// icp.hip's point-to-plane terms in the RegistrationICP loop.  The pass itself — winner,
// write-back, the 30 slots, the fixed-order sum — is terms_pass.h's; the NN scan before it, the
// solve after it (icp.hip solve_state, the point-to-plane slot layout) and the convergence rule
// are the loop's own.
//
// Covariance of a point with unit normal n (InitializePointCloudForGeneralizedICP):
//   C = Rx·diag(ε, 1, 1)·Rxᵀ,  Rx = GetRotationFromE1ToX(n):  v = e1 × n = (0, −nz, ny), c = nx,
//   Rx = I when c < −0.99, else I + [v]× + [v]×²·(1 / (1 + c)).
// Every covariance is held as its upper triangle, 6 doubles (xx, xy, xz, yy, yz, zz): the lower
// one is its mirror by definition, so a covariance is symmetric in every bit.
//
// One evaluation, source slot i (its point p, covariance Cs; dT = the transform the evaluation
// applies, IcpState::dT — the init, then each update):
//   vs = dT·p (nnkey.h q64_of), Cs ← R·Cs·Rᵀ (R = dT's rotation; terms_pass.h rotate_cov6, shared
//   with robust.hip), both written back (pcd.Transform(update) moves points and covariances);
//   winner t = nnkey.h winner_fp64;
//   d = vs − vt, M = Ct + Cs, B = M⁻¹ (closed form: cofactors over the determinant),
//   J₀ = [−[vs]× | I] (3×6):  JᵀJ += J₀ᵀ·B·J₀, Jᵀr += J₀ᵀ·B·d, Σr² += dᵀ·B·d, count += 1, Σd² += d².
// With unit weights this equals Open3D's rows W·d, W·J₀ with W = M^(−1/2): no square root needed.
// Slots and order of summation: terms_pass.h.
//
// Bytes per source the terms pass must move: its point read and written (24 + 24), its
// covariance read and written (48 + 48), key, runner-up and correspondence (8 + 4 + 4), and the
// gathered winner's point and covariance (24 + 48): 232 B.
#include "m3d_internal.h"
#include "nnkey.h"
#include "terms_pass.h"

namespace m3d {

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
__device__ __forceinline__ void jtj_row(double (&v)[kTermsUsed], double x, double y, double z,
                                        const double (&G)[6][3]) {
  if constexpr (c < 6) {
    v[jtj_slot(a, c)] = j0_dot<a>(x, y, z, G[c]);
    jtj_row<a, c + 1>(v, x, y, z, G);
  }
}
template <int a>
__device__ __forceinline__ void jtj_rows(double (&v)[kTermsUsed], double x, double y, double z,
                                         const double (&G)[6][3], const double (&w)[3]) {
  if constexpr (a < 6) {
    jtj_row<a, a>(v, x, y, z, G);
    v[21 + a] = j0_dot<a>(x, y, z, w);
    jtj_rows<a + 1>(v, x, y, z, G, w);
  }
}

// The plane-to-plane terms of a matched pair (the file header's formulas, expression for expression)
struct GicpEst : CovState {
  __device__ __forceinline__ void rows(double (&v)[kTermsUsed], const SlotWinner& sw, const double* __restrict__ tq,
                                       const Slot& own) const {
    const double(&Q)[3] = sw.Q;
    const double(&Cs)[6] = own.Cs;
    const double* ct = cov_t + 6 * sw.gj;
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
  }
};

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

// The plane-to-plane terms of the loop's current evaluation and their reduction into sums
// (terms_pass.h launch_side_terms)
hipError_t launch_gicp_terms(const m3d_icp* s, double* cov_s, const double* cov_t, double* partials,
                             double* sums, bool with_defer, hipStream_t st) {
  return launch_side_terms(s, GicpEst{{cov_s, cov_t}}, partials, sums, with_defer, st);
}

}  // namespace m3d
