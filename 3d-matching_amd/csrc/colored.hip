// colored.hip — Colored ICP (Open3D 0.19 ColoredICP.cpp; Park, Zhou, Koltun 2017): the colour
// gradient of every target point, built once per call, and the two-row estimator (ColoredEst) of
// the side terms pass (terms_pass.h) that replaces icp.hip's point-to-plane terms in the
// RegistrationICP loop.  The NN scan before it, the solve after it (icp.hip solve_state, the
// point-to-plane slot layout), fitness, the geometric inlier_rmse and the convergence rule are
// the loop's own, as for gicp.hip and robust.hip.
//
// Intensity of a colour (r, g, b):  I = ((r + g) + b) / 3.0.
//
// Gradient of target point k (point vt, unit normal nt, intensity it), radius r, max_nn ≤ 64:
//   the hybrid list = the max_nn nearest with d² < r² (strict, the query itself included), ordered
//   by (d², index): knn_wave.h wave_knn_scan_box, the list of m3d_hybrid_search.  nn = its length.
//   nn < 4: the gradient is 0.  Else entry 0 is skipped, whatever it is (Open3D's loop starts at 1;
//   among exact duplicates of the query FLANN's order is unpinned, here the lowest index leads), and
//   entry e = 1 .. nn − 1 with neighbour p, intensity ip gives the row
//     d = p − vt,  s = (d0·n0 + d1·n1) + d2·n2,  proj = p − s·nt,  A_e = proj − vt,  b_e = ip − it.
//   AᵀA (upper, 6) and Aᵀb (3) are sums of the products A_a·A_c, A_a·b over the entries, one per
//   lane, in wave_sum's xor butterfly (32, 16, …, 1; a lane without an entry adds 0.0; taken
//   through nnkey.h wave_sum_dpp, the same tree with DPP moves for the short strides).  Then the
//   constraint row c·nt, c = (double)(nn − 1), b = 0:  AᵀA_ac += (c·n_a)·(c·n_c).
//   Solve (AᵀA)·x = Aᵀb by an unpivoted LDLᵀ (Open3D: SolveLinearSystemPSD, A.ldlt().solve):
//     d0 = a00, l10 = a01/d0, l20 = a02/d0, d1 = a11 − l10·a01, m = a12 − l20·a01, l21 = m/d1,
//     d2 = (a22 − l20·a02) − l21·m;  y0 = b0, y1 = b1 − l10·y0, y2 = (b2 − l20·y0) − l21·y1;
//     x2 = y2/d2, x1 = y1/d1 − l21·x2, x0 = (y0/d0 − l10·x1) − l20·x2.
//   Departure, deliberate: a pivot that is not positive and finite, or a non-finite x, gives the
//   gradient 0 (Eigen's pivoted LDLT would return whatever it computes).
//   One 32-byte record per target: {gx, gy, gz, it}.
//
// Terms of a matched pair, sg = sqrt(λ), sp = sqrt(1 − λ) (both formed on the host), moved source
// vs = (x, y, z) with intensity is, target vt, nt and record {dit, it}:
//   d = vs − vt,  s = (d0·n0 + d1·n1) + d2·n2
//   row 0:  r0 = sg·s,  J0 = [sg·(vs × nt) | sg·nt]
//   row 1:  proj = vs − s·nt,  e = proj − vt,  is0 = ((g0·e0 + g1·e1) + g2·e2) + it,
//           M = I − nt·ntᵀ (M_aa = 1.0 − n_a·n_a, M_ac = −(n_a·n_c)),
//           m_c = −((g0·M_0c + g1·M_1c) + g2·M_2c)   (ditM = −ditᵀ·M),
//           r1 = sp·(is − is0),  J1 = [sp·(vs × m) | sp·m]
//   each row added by terms_pass.h add_row with its own weight w(r) (robust.hip's table; no
//   kernel or L2: 1): (w·J_a)·J_c, (w·J_a)·r and the unweighted r·r into slot 27.  Count, Σd², the
//   slots and the order of summation: terms_pass.h.  No floating-point atomics anywhere in this
//   file.
//
// Bytes per source the terms pass must move: its point read and written (24 + 24), key,
// runner-up and correspondence (8 + 4 + 4), its intensity (8), and the gathered winner's point,
// normal and record (24 + 24 + 32): 152 B.  The gradient pass never writes the N × max_nn
// neighbour lists: a wave keeps its list in registers and writes 32 B per target.
#include "knn_wave.h"
#include "m3d_internal.h"
#include "nnkey.h"
#include "terms_pass.h"

namespace m3d {

namespace {

__device__ __forceinline__ double intensity_of(const double* __restrict__ c) { return ((c[0] + c[1]) + c[2]) / 3.0; }

__device__ __forceinline__ bool good_pivot(double d) { return d > 0.0 && isfinite(d); }

// ONE WAVE per target point: the hybrid list as prep.hip hybrid_search_wave_kernel fills it (the
// same two-stage fine-grid shortcut), kept in registers; lane e holds entry e and forms its row.
// rec (n × 4) and out3 (n × 3): either may be null.
__global__ __launch_bounds__(256) void color_gradient_kernel(
    const double* __restrict__ xyz64, const float4* __restrict__ xyz32, const double* __restrict__ nrm,
    const double* __restrict__ colors, int64_t n, GridDev g, float Rf, double r2, double eabs, int k, GridDev gf,
    float Hf, double h2safe, double* __restrict__ rec, double* __restrict__ out3) {
  __shared__ double s_d[4][64];  // merge_chunk's row per wave
  __shared__ int32_t s_t[4][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t i = (int64_t)blockIdx.x * 4 + w;
  if (i >= n) return;  // wave-uniform
  const double q[3] = {xyz64[3 * i], xyz64[3 * i + 1], xyz64[3 * i + 2]};
  const float4 qf = xyz32[i];
  WaveKnnList<1> L;
  L.reset(r2, eabs);
  bool done = false;
  if (gf.ncells > 0) {
    wave_knn_scan_box(L, xyz64, q, qf, gf, Hf, r2, eabs, k, 0, 64, s_d[w], s_t[w]);
    done = L.cnt == k && L.thr < h2safe;  // wave-uniform
    if (!done) L.reset(r2, eabs);
  }
  if (!done && g.ncells > 0) wave_knn_scan_box(L, xyz64, q, qf, g, Rf, r2, eabs, k, 0, 64, s_d[w], s_t[w]);
  const int nn = L.cnt;  // wave-uniform
  const double it = intensity_of(colors + 3 * i);
  double gx = 0.0, gy = 0.0, gz = 0.0;
  if (nn >= 4) {
    const double n0 = nrm[3 * i], n1 = nrm[3 * i + 1], n2 = nrm[3 * i + 2];
    double A0 = 0.0, A1 = 0.0, A2 = 0.0, b = 0.0;
    if (lane >= 1 && lane < nn) {
      const int64_t t = L.T[0];
      const double* p = xyz64 + 3 * t;
      const double p0 = p[0], p1 = p[1], p2 = p[2];
      const double d0 = p0 - q[0], d1 = p1 - q[1], d2 = p2 - q[2];
      const double s = (d0 * n0 + d1 * n1) + d2 * n2;
      A0 = (p0 - s * n0) - q[0];
      A1 = (p1 - s * n1) - q[1];
      A2 = (p2 - s * n2) - q[2];
      b = intensity_of(colors + 3 * t) - it;
    }
    // wave_sum's tree with its short strides as DPP moves (nnkey.h): the same bits
    double a00 = wave_sum_dpp(A0 * A0), a01 = wave_sum_dpp(A0 * A1), a02 = wave_sum_dpp(A0 * A2);
    double a11 = wave_sum_dpp(A1 * A1), a12 = wave_sum_dpp(A1 * A2), a22 = wave_sum_dpp(A2 * A2);
    const double b0 = wave_sum_dpp(A0 * b), b1 = wave_sum_dpp(A1 * b), b2 = wave_sum_dpp(A2 * b);
    // the constraint row (nn − 1)·nt, b = 0, last
    const double c = (double)(nn - 1);
    const double c0 = c * n0, c1 = c * n1, c2 = c * n2;
    a00 += c0 * c0;
    a01 += c0 * c1;
    a02 += c0 * c2;
    a11 += c1 * c1;
    a12 += c1 * c2;
    a22 += c2 * c2;
    // unpivoted LDLᵀ (every lane holds the same sums; lane 0's result is written)
    const double e0 = a00;
    const double l10 = a01 / e0, l20 = a02 / e0;
    const double e1 = a11 - l10 * a01;
    const double m = a12 - l20 * a01;
    const double l21 = m / e1;
    const double e2 = (a22 - l20 * a02) - l21 * m;
    const double y0 = b0, y1 = b1 - l10 * y0, y2 = (b2 - l20 * y0) - l21 * y1;
    const double x2 = y2 / e2;
    const double x1 = y1 / e1 - l21 * x2;
    const double x0 = (y0 / e0 - l10 * x1) - l20 * x2;
    if (good_pivot(e0) && good_pivot(e1) && good_pivot(e2) && isfinite(x0) && isfinite(x1) && isfinite(x2)) {
      gx = x0;
      gy = x1;
      gz = x2;
    }
  }
  if (lane == 0) {
    if (rec != nullptr) {
      double* o = rec + 4 * i;
      o[0] = gx;
      o[1] = gy;
      o[2] = gz;
      o[3] = it;
    }
    if (out3 != nullptr) {
      double* o = out3 + 3 * i;
      o[0] = gx;
      o[1] = gy;
      o[2] = gz;
    }
  }
}

// rec[k] = {grad[k], I(colors[k])}: a caller's gradients (n × 3) as the terms pass reads them
__global__ __launch_bounds__(256) void color_rec_pack_kernel(const double* __restrict__ grad,
                                                             const double* __restrict__ colors, int64_t n,
                                                             double* __restrict__ rec) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= n) return;
  double* o = rec + 4 * k;
  o[0] = grad[3 * k];
  o[1] = grad[3 * k + 1];
  o[2] = grad[3 * k + 2];
  o[3] = intensity_of(colors + 3 * k);
}

// out[k] = the intensity of point slot[k] (slot null: k): the source's in the loop's slot order
__global__ __launch_bounds__(256) void intensity_pack_kernel(const double* __restrict__ colors,
                                                             const int32_t* __restrict__ slot, int64_t n,
                                                             double* __restrict__ out) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= n) return;
  out[k] = intensity_of(colors + 3 * (slot != nullptr ? (int64_t)slot[k] : k));
}

// the two weighted rows of a matched pair (the file header's formulas); sg = sqrt(λ), sp = sqrt(1 − λ)
template <int K>
struct ColoredEst : NoSlotState {
  const double* __restrict__ nrm_t;
  const double* __restrict__ rec_t;
  const double* __restrict__ is_s;
  double sg, sp, kk;
  __device__ __forceinline__ void rows(double (&v)[kTermsUsed], const SlotWinner& sw, const double* __restrict__ tq,
                                       const Slot&) const {
    const double(&Q)[3] = sw.Q;
    const double* tn = nrm_t + 3 * sw.gj;
    const double* tr = rec_t + 4 * sw.gj;
    const double is = is_s[sw.i];
    const double t0 = tq[0], t1 = tq[1], t2 = tq[2];
    const double nx = tn[0], ny = tn[1], nz = tn[2];
    const double g0 = tr[0], g1 = tr[1], g2 = tr[2], it = tr[3];
    const double x = Q[0], y = Q[1], z = Q[2];
    const double sd = ((x - t0) * nx + (y - t1) * ny) + (z - t2) * nz;
    {
      const double r0 = sg * sd;
      const double J[6] = {sg * (y * nz - z * ny), sg * (z * nx - x * nz), sg * (x * ny - y * nx),
                           sg * nx,                sg * ny,                sg * nz};
      add_row(v, J, r0, robust_weight<K>(r0, kk));
    }
    {
      const double e0 = (x - sd * nx) - t0, e1 = (y - sd * ny) - t1, e2 = (z - sd * nz) - t2;
      const double is0 = ((g0 * e0 + g1 * e1) + g2 * e2) + it;
      const double M00 = 1.0 - nx * nx, M11 = 1.0 - ny * ny, M22 = 1.0 - nz * nz;
      const double M01 = -(nx * ny), M02 = -(nx * nz), M12 = -(ny * nz);
      const double m0 = -((g0 * M00 + g1 * M01) + g2 * M02);
      const double m1 = -((g0 * M01 + g1 * M11) + g2 * M12);
      const double m2 = -((g0 * M02 + g1 * M12) + g2 * M22);
      const double r1 = sp * (is - is0);
      const double J[6] = {sp * (y * m2 - z * m1), sp * (z * m0 - x * m2), sp * (x * m1 - y * m0),
                           sp * m0,                sp * m1,                sp * m2};
      add_row(v, J, r1, robust_weight<K>(r1, kk));
    }
  }
};

}  // namespace

// The colour gradients of every point of c (its normals nrm, colours n × 3): g / gf / hfine as
// hybrid_search takes them, 1 ≤ k ≤ 64.  rec (n × 4: gradient, intensity) and out3 (n × 3): either
// may be null.  n == 0 launches nothing.
hipError_t launch_color_gradients(const m3d_cloud* c, const double* nrm, const double* colors, const Grid* g,
                                  double radius, int k, double* rec, double* out3, hipStream_t st, const Grid* gf,
                                  double hfine) {
  if (c->n == 0) return hipSuccess;
  const float Rf = box_half_width(c, radius);
  GridDev gfd{};
  gfd.ncells = 0;
  float Hf = 0.0f;
  double h2safe = 0.0;
  if (gf != nullptr && hfine > 0.0 && hfine < radius) {
    gfd = gf->dev;
    Hf = box_half_width(c, hfine);
    h2safe = hfine * hfine * (1.0 - 1e-12);
  }
  const unsigned wb = (unsigned)((c->n + 3) / 4);  // 4 waves (targets) per 256-thread block
  color_gradient_kernel<<<wb, 256, 0, st>>>(c->xyz64, c->xyz32, nrm, colors, c->n, g->dev, Rf, radius * radius,
                                            pair_eabs(c), k, gfd, Hf, h2safe, rec, out3);
  return hipGetLastError();
}

hipError_t launch_color_rec_pack(const double* grad, const double* colors, int64_t n, double* rec, hipStream_t st) {
  if (n == 0) return hipSuccess;
  color_rec_pack_kernel<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(grad, colors, n, rec);
  return hipGetLastError();
}

hipError_t launch_intensity_pack(const double* colors, const int32_t* slot, int64_t n, double* out, hipStream_t st) {
  if (n == 0) return hipSuccess;
  intensity_pack_kernel<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(colors, slot, n, out);
  return hipGetLastError();
}

// The colored terms of the loop's current evaluation and their reduction into sums (terms_pass.h
// launch_side_terms).  rec_t: the target's records in index order; is_s: the source's intensities
// in slot order; kind: a checked M3D_KERNEL_* (L2: unit weights); the target has normals.
hipError_t launch_colored_terms(const m3d_icp* s, const double* rec_t, const double* is_s, double lambda,
                                int32_t kind, double k, double* partials, double* sums, bool with_defer,
                                hipStream_t st) {
  const double sg = std::sqrt(lambda), sp = std::sqrt(1.0 - lambda);
  hipError_t e = hipSuccess;
  with_kind(kind, [&](auto K) {
    e = launch_side_terms(s, ColoredEst<decltype(K)::value>{{}, s->tgt->nrm64, rec_t, is_s, sg, sp, k}, partials, sums,
                          with_defer, st);
  });
  return e;
}

}  // namespace m3d
