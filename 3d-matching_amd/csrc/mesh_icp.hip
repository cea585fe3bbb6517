// mesh_icp.hip — point-to-plane ICP of a point cloud against the SURFACE of a triangle mesh: the
// RegistrationICP loop (Open3D Registration.cpp) with the closest triangle of mesh.hip's contract
// in the place of the nearest target point, and the triangle's face normal in the place of the
// target's normal.  Device resident: scan, terms + reduce and solve are three launches per
// evaluation, no host sync in between.
//
// CONTRACT (restated in numpy by tests/mesh_icp_restatement.py).  All arithmetic is fp64, one
// operation at a time (-ffp-contract=off), every dot product x·y = (x0*y0 + x1*y1) + x2*y2.
//
// One EVALUATION of the loop's points P (the loop's own fp64 copy of the source, as m3d_icp's:
// `init` applied unless it isIdentity(), every update applied by the NEXT evaluation's query):
// p = q64_of(dT, P[i]) (nnkey.h), written back to P[i].
//   Winner.  mesh.hip's contract winner, unchanged: the smallest (d², triangle index) under
//     key_less over ALL usable triangles whose d² is not NaN, d² and the closest point q from
//     tri_closest (mesh_tri.h), the one function every kernel here and in mesh.hip calls.
//   Match.  p is MATCHED iff the winner exists and d² < max_dist·max_dist in fp64, strictly; a NaN
//     point is never matched.  Unmatched: triangle −1, d² +inf.
//   Row of a matched p, winner triangle (a, b, c), ab = b − a, ac = c − a:
//     (cx, cy, cz) = (ab1*ac2 − ab2*ac1, ab2*ac0 − ab0*ac2, ab0*ac1 − ab1*ac0)   (mesh_pack_kernel's
//     usable test: not three zeros), len = sqrt((cx*cx + cy*cy) + cz*cz), n = (cx/len, cy/len, cz/len)
//     the face normal (point-to-plane does not depend on its sign);
//     r = ((px − qx)*nx + (py − qy)*ny) + (pz − qz)*nz;
//     J = [p × n | n] = (py*nz − pz*ny, pz*nx − px*nz, px*ny − py*nx, nx, ny, nz)   (RobustPlaneEst's order);
//     w = robust_weight<K>(r, k); add_row(v, J, r, w) (terms_pass.h); slot 28 += 1, slot 29 += d².
//   Reduction.  block_partial over kSideBlock consecutive slots, then launch_reduce: the fixed order
//     of every loop here (icp.hip, "reduce"); no floating-point atomics.  The source runs in the
//     Morton slot order of its cloud (cell = 1.001·max_dist, as m3d_icp), whichever path scans.
//   Solve.  Not here: icp.hip's solve_state<M3D_EST_POINT_TO_PLANE>, the cloud loops' own kernel
//     (launch_icp_solve_state), on this loop's IcpState.  fitness = count / ns, rmse =
//     sqrt(Σd² / count), 0 / 0 → 0; stop when evals > 0 and |Δfitness| < relative_fitness and
//     |Δrmse| < relative_rmse (converged), or when max_iteration updates are applied; else
//     JᵀJ·x = −Jᵀr by ldlt6_solve_spd, a failed one by the pivoted ldlt6_solve, x → matrix by
//     vec6_to_matrix_wave (all linalg.h), a non-finite update is the identity, T ← ΔT·T by
//     matmul4_affine, dT ← ΔT.  That kernel also refreshes the fp32 search fields of the state
//     for the frame it is given; this loop hands it mesh_icp_frame() (m3d_internal.h) and reads none
//     of them.
//   State.  Reset by icp.hip's icp_init_kernel (launch_icp_state_init), as m3d_icp_reset: T = init
//     with the bottom row (0, 0, 0, 1), dT = init unless it isIdentity().
//   ns = 0: fitness 0, T = init, no pairs — not an error.
//
// SCAN, grid path: one wave per point over the mesh's triangle grid (mesh.hip builds it), ONE box
// of half-width Rf = max_dist rounded up to fp32, cut with below / above; no radius ladder.
//   Why one box suffices.  By mesh.hip's covering argument (2), a triangle NOT referenced from the
//   box cut with Rf has d² ≥ (double)Rf² — with that argument's proviso: its computed closest point
//   lies inside its own box widened by the margin m, which only a sliver thinner than m can miss
//   (the brute path is the definition).  Rf ≥ max_dist as reals, Rf² is exact in fp64 (48 bits) and
//   rounding is monotone, so Rf² ≥ max_dist·max_dist as computed: every unscanned triangle is
//   unmatched by itself.  If the contract's winner has d² < max_dist² it was scanned, and it is the
//   minimum of the scanned ones; if not, no scanned triangle is below max_dist² either.  So "the
//   minimum over the box, kept when d² < max_dist²" IS the contract's winner filtered by the radius.
//   Seeded box.  With `seed`, a point first evaluates the triangle it matched in the last
//   evaluation (or the caller's, in the one-evaluation call) at its moved position.  If that
//   d²_s < max_dist², the box shrinks to R = min(Rf, sqrt(d²_s)·(1 + 2^-20) rounded up to fp32) — the
//   ladder's rule: R² ≥ d²_s, so by the same argument every triangle outside the smaller box has
//   d² ≥ R² ≥ d²_s, strictly greater unless d²_s = 0, where an unscanned triangle's closest point
//   differs from p and its d² is positive.  The seed's triangle takes part in the minimum, so the
//   winner, its d² and its point are the unseeded scan's, bit for bit; a seed that names no usable
//   triangle is ignored.
// SCAN, brute path: one thread per point, the triangles staged through LDS in tiles of
// kMeshBruteTile: the definition, and the path for small meshes.
// Both scans are mesh.hip's searches (mesh_tri.h: tri_min_brute, tri_min_box); a kernel here keeps
// the query (dT applied, written back), the box's rule and the record (write_rec).
//
// Both paths, seed on and off, and two runs give the same bits in the records, the sums, the pose
// and the pairs: a point's record depends on its own scan alone, and the sums are added in the
// fixed order above.
//
// NOT HERE: point-to-point estimation against a mesh, Generalized and Colored ICP against a mesh,
// multi-GPU sharding, the step-wise driver, HIP-graph replay, pseudo-normals on edge and vertex
// regions (a point whose closest point lies on an edge or a vertex still gets the winning
// triangle's face normal).
#include <float.h>

#include <cmath>

#include "m3d_internal.h"
#include "knn_wave.h"
#include "mesh_tri.h"
#include "nnkey.h"
#include "terms_pass.h"

namespace m3d {
namespace {

constexpr int kScanBlock = 256;

// a point's record: what the scan leaves for the terms pass and the caller
struct MeshRec {
  int32_t* __restrict__ tri;  // the matched triangle, −1 none
  double* __restrict__ d2;    // its d², +inf none
  double* __restrict__ pt;    // its closest point (unwritten when unmatched)
};

// the record of point i from the scan's minimum (bd, bt), and the moved point written back
__device__ __forceinline__ void write_rec(const MeshRec& o, double* __restrict__ pcd64, int64_t i,
                                          const double* __restrict__ tri9, const double q[3], double bd, int32_t bt,
                                          double r2) {
  const bool hit = bt >= 0 && bd < r2;
  o.tri[i] = hit ? bt : -1;
  o.d2[i] = hit ? bd : INFINITY;
  if (hit) {
    // the winner's closest point evaluated again: the same function on the same operands
    const double* t9 = tri9 + 9 * (int64_t)bt;
    TriHit h;
    tri_closest(t9, t9 + 3, t9 + 6, q, h);
    o.pt[3 * i] = h.pt[0];
    o.pt[3 * i + 1] = h.pt[1];
    o.pt[3 * i + 2] = h.pt[2];
  }
  pcd64[3 * i] = q[0];
  pcd64[3 * i + 1] = q[1];
  pcd64[3 * i + 2] = q[2];
}

__global__ __launch_bounds__(kScanBlock) void mesh_icp_brute_kernel(double* __restrict__ pcd64, int64_t ns,
                                                                    const double* __restrict__ tri9,
                                                                    const uint8_t* __restrict__ ok, int64_t nf,
                                                                    const IcpState* __restrict__ s, MeshRec out) {
  if (s->done) return;  // uniform
  __shared__ double s9[kMeshBruteTile * 9];
  __shared__ uint8_t sok[kMeshBruteTile];
  const int64_t i = (int64_t)blockIdx.x * kScanBlock + threadIdx.x;
  const bool valid = i < ns;
  double q[3] = {0.0, 0.0, 0.0};
  if (valid) {
    const double p[3] = {pcd64[3 * i], pcd64[3 * i + 1], pcd64[3 * i + 2]};
    q64_of(s->dT, p, q);
  }
  double bd;
  int32_t bt;
  tri_min_brute<kScanBlock>(tri9, ok, nf, q, valid, s9, sok, bd, bt);
  if (valid) write_rec(out, pcd64, i, tri9, q, bd, bt, s->r2);
}

// ONE WAVE per point, one box (header).  use_seed: out.tri[i] holds the point's seed triangle.
__global__ __launch_bounds__(kScanBlock) void mesh_icp_grid_kernel(double* __restrict__ pcd64, int64_t ns,
                                                                   const double* __restrict__ tri9,
                                                                   const uint8_t* __restrict__ ok, int64_t nf,
                                                                   TriGridDev g, const IcpState* __restrict__ s,
                                                                   float Rf0, int use_seed, MeshRec out) {
  if (s->done) return;  // uniform
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * (kScanBlock / kWave) + (threadIdx.x >> 6);
  if (i >= ns) return;  // wave-uniform
  double q[3];
  {
    const double p[3] = {pcd64[3 * i], pcd64[3 * i + 1], pcd64[3 * i + 2]};
    q64_of(s->dT, p, q);
  }
  const double r2 = s->r2;
  double bd = INFINITY;
  int32_t bt = -1;
  float Rf = Rf0;
  if (use_seed) {  // every lane the same triangle: the same (bd, bt) in every lane
    const int32_t t = out.tri[i];
    if (t >= 0 && t < nf && ok[t]) {
      const double* t9 = tri9 + 9 * (int64_t)t;
      TriHit h;
      tri_closest(t9, t9 + 3, t9 + 6, q, h);
      if (h.d2 < r2) {
        take_min(bd, bt, h.d2, t);
        Rf = fminf(Rf0, __double2float_ru(sqrt(h.d2) * (1.0 + 0x1p-20)));
      }
    }
  }
  // a point that is not finite matches nothing (every d² is NaN or +inf): no cell is read
  const bool finite = fabs(q[0]) <= DBL_MAX && fabs(q[1]) <= DBL_MAX && fabs(q[2]) <= DBL_MAX;
  // a point outside fp32's comfortable range, or a half-width near its top, takes the whole grid
  const bool all = !(fabs(q[0]) <= 0x1p120 && fabs(q[1]) <= 0x1p120 && fabs(q[2]) <= 0x1p120) || !(Rf < 0x1p122f);
  if (finite) {
    int c0[3], c1[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      c0[k] = all ? 0 : grid_coord(below(q[k], Rf), g.o[k], g.inv_h, g.n[k]);
      c1[k] = all ? g.n[k] - 1 : grid_coord(above(q[k], Rf), g.o[k], g.inv_h, g.n[k]);
    }
    tri_box_walk(tri9, g, c0, c1, lane, q, bd, bt);
  }
  tri_wave_min(bd, bt);
  if (lane == 0) write_rec(out, pcd64, i, tri9, q, bd, bt, r2);
}

// One thread per slot: the matched point's row (header) into the 30 sums.  No thread returns
// before block_partial (`done` is uniform).
template <int K>
__global__ __launch_bounds__(kSideBlock) void mesh_icp_terms_kernel(const double* __restrict__ pcd64, int64_t ns,
                                                                    const double* __restrict__ tri9,
                                                                    const IcpState* __restrict__ s,
                                                                    const int32_t* __restrict__ rtri,
                                                                    const double* __restrict__ rd2,
                                                                    const double* __restrict__ rpt, double kk,
                                                                    double* __restrict__ partials) {
  if (s->done) return;
  const int64_t i = (int64_t)blockIdx.x * kSideBlock + threadIdx.x;
  double v[kTermsUsed];
#pragma unroll
  for (int k = 0; k < kTermsUsed; ++k) v[k] = 0.0;
  const int32_t t = i < ns ? rtri[i] : -1;
  if (t >= 0) {
    const double* t9 = tri9 + 9 * (int64_t)t;
    const double ab[3] = {t9[3] - t9[0], t9[4] - t9[1], t9[5] - t9[2]};
    const double ac[3] = {t9[6] - t9[0], t9[7] - t9[1], t9[8] - t9[2]};
    const double cx = ab[1] * ac[2] - ab[2] * ac[1];
    const double cy = ab[2] * ac[0] - ab[0] * ac[2];
    const double cz = ab[0] * ac[1] - ab[1] * ac[0];
    const double len = sqrt((cx * cx + cy * cy) + cz * cz);
    const double nx = cx / len, ny = cy / len, nz = cz / len;
    const double x = pcd64[3 * i], y = pcd64[3 * i + 1], z = pcd64[3 * i + 2];
    const double r = ((x - rpt[3 * i]) * nx + (y - rpt[3 * i + 1]) * ny) + (z - rpt[3 * i + 2]) * nz;
    const double J[6] = {y * nz - z * ny, z * nx - x * nz, x * ny - y * nx, nx, ny, nz};
    add_row(v, J, r, robust_weight<K>(r, kk));
    v[28] = 1.0;
    v[29] = rd2[i];
  }
  block_partial<kTermSlots, kTermsUsed, kSideBlock>(v, partials);
}

unsigned blocks_of(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

}  // namespace

hipError_t launch_mesh_icp_scan(const m3d_mesh* m, const MeshIcpLoop& L, bool brute, bool seed, hipStream_t st) {
  if (L.ns == 0) return hipSuccess;
  const MeshRec rec{L.tri, L.d2, L.pt};
  if (brute) {
    mesh_icp_brute_kernel<<<blocks_of(L.ns, kScanBlock), kScanBlock, 0, st>>>(L.pcd64, L.ns, m->tri9, m->ok, m->nf,
                                                                               L.state, rec);
    return hipGetLastError();
  }
  float rf = float_up(L.max_dist);
  if (!(rf > 0.0f)) rf = FLT_MIN;
  if (!(rf <= FLT_MAX)) rf = FLT_MAX;
  mesh_icp_grid_kernel<<<blocks_of(L.ns, kScanBlock / kWave), kScanBlock, 0, st>>>(
      L.pcd64, L.ns, m->tri9, m->ok, m->nf, m->grid, L.state, rf, seed ? 1 : 0, rec);
  return hipGetLastError();
}

hipError_t launch_mesh_icp_terms(const m3d_mesh* m, const MeshIcpLoop& L, int32_t kind, double k, double* sums,
                                 hipStream_t st) {
  const int64_t nb = side_terms_blocks(L.ns);
  if (nb > 0)
    with_kind(kind, [&](auto K) {
      mesh_icp_terms_kernel<decltype(K)::value><<<(unsigned)nb, kSideBlock, 0, st>>>(
          L.pcd64, L.ns, m->tri9, L.state, L.tri, L.d2, L.pt, k, L.partials);
    });
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? launch_reduce(L.partials, nb, kTermSlots, sums, L.state, nullptr, st) : e;
}

}  // namespace m3d
