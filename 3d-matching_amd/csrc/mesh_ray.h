// mesh_ray.h — the ray–triangle test of the ray-casting contract (mesh_ray.hip's header), restated
// in numpy by tests/mesh_ray_restatement.py.  ray_tri is the ONE function every kernel calls; the
// per-ray constants are computed once by ray_setup.
//
// All arithmetic is fp64, one operation at a time (-ffp-contract=off).  A ray is (o, d), six
// doubles; the test is the watertight test of Woop, Benthin and Wald (Journal of Computer Graphics
// Techniques 2(1), 2013) in fp64.
//   per ray       kz = the axis of the largest |d| (the lowest axis wins a tie), kx = (kz+1)%3,
//                 ky = (kx+1)%3, kx and ky swapped when d[kz] < 0;
//                 Sx = d[kx]/d[kz], Sy = d[ky]/d[kz], Sz = 1/d[kz].
//                 A ray with a component that is not finite, or with d == 0, hits nothing.
//   per triangle  A = a − o (B, C alike); Ax = A[kx] − Sx*A[kz], Ay = A[ky] − Sy*A[kz];
//                 U = Cx*By − Cy*Bx, V = Ax*Cy − Ay*Cx, W = Bx*Ay − By*Ax;
//                 miss if (U<0 || V<0 || W<0) && (U>0 || V>0 || W>0);
//                 det = (U+V)+W, miss if det == 0;
//                 Az = Sz*A[kz] (Bz, Cz alike); t = ((U*Az + V*Bz) + W*Cz) / det;
//                 hit iff tnear ≤ t && t ≤ tfar (a NaN t misses);
//                 (u, v) = (V/det, W/det): point ≈ (1−u−v)·a + u·b + v·c.
// Both orientations hit.  The two triangles of a shared edge compute that edge's value from the same
// two products in opposite order, so the values are exact negatives of each other: a ray whose edge
// values are all non-zero crosses a closed mesh with exact parity.  An edge value that is exactly
// zero counts for BOTH triangles (Woop's own rule, as Embree without its robust mode).
#pragma once

#include <cmath>

#include "m3d_internal.h"

namespace m3d {

struct RaySetup {
  int kx, ky, kz;
  double ox, oy, oz;  // o[kx], o[ky], o[kz]
  double dz;          // d[kz]
  double Sx, Sy, Sz;
  bool ok;            // six finite components and d != 0
};

struct RayHit {
  double t, u, v;
};

__device__ __forceinline__ double pick3(const double* x, int k) { return k == 0 ? x[0] : (k == 1 ? x[1] : x[2]); }

__device__ __forceinline__ void ray_setup(const double o[3], const double d[3], RaySetup& s) {
  const double a0 = fabs(d[0]), a1 = fabs(d[1]), a2 = fabs(d[2]);
  bool fin = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) fin = fin && isfinite(o[k]) && isfinite(d[k]);
  s.ok = fin && !(d[0] == 0.0 && d[1] == 0.0 && d[2] == 0.0);
  int kz = 0;
  double am = a0;
  if (a1 > am) kz = 1, am = a1;
  if (a2 > am) kz = 2;
  int kx = kz == 2 ? 0 : kz + 1;
  int ky = kx == 2 ? 0 : kx + 1;
  const double dz = pick3(d, kz);
  if (dz < 0.0) {
    const int tmp = kx;
    kx = ky;
    ky = tmp;
  }
  s.kx = kx, s.ky = ky, s.kz = kz;
  s.ox = pick3(o, kx), s.oy = pick3(o, ky), s.oz = pick3(o, kz);
  s.dz = dz;
  s.Sx = pick3(d, kx) / dz;
  s.Sy = pick3(d, ky) / dz;
  s.Sz = 1.0 / dz;
}

// the contract's test of the ray s against the triangle (a, b, c); h is written on a hit only
__device__ __forceinline__ bool ray_tri(const RaySetup& s, const double* a, const double* b, const double* c,
                                        double tnear, double tfar, RayHit& h) {
  const double Akz = a[s.kz] - s.oz, Bkz = b[s.kz] - s.oz, Ckz = c[s.kz] - s.oz;
  const double Ax = (a[s.kx] - s.ox) - s.Sx * Akz, Ay = (a[s.ky] - s.oy) - s.Sy * Akz;
  const double Bx = (b[s.kx] - s.ox) - s.Sx * Bkz, By = (b[s.ky] - s.oy) - s.Sy * Bkz;
  const double Cx = (c[s.kx] - s.ox) - s.Sx * Ckz, Cy = (c[s.ky] - s.oy) - s.Sy * Ckz;
  const double U = Cx * By - Cy * Bx;
  const double V = Ax * Cy - Ay * Cx;
  const double W = Bx * Ay - By * Ax;
  if ((U < 0.0 || V < 0.0 || W < 0.0) && (U > 0.0 || V > 0.0 || W > 0.0)) return false;
  const double det = (U + V) + W;
  if (det == 0.0) return false;
  const double Az = s.Sz * Akz, Bz = s.Sz * Bkz, Cz = s.Sz * Ckz;
  const double t = ((U * Az + V * Bz) + W * Cz) / det;
  if (!(tnear <= t && t <= tfar)) return false;
  h.t = t;
  h.u = V / det;
  h.v = W / det;
  return true;
}

}  // namespace m3d
