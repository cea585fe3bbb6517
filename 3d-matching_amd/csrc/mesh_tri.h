// mesh_tri.h — the pieces of the point-to-mesh contract (mesh.hip's header) that more than one
// translation unit evaluates: closest(p, triangle), the running (d², index) minimum, the two
// searches for it — the brute-force sweep over all triangles and the wave's walk over a cell box of
// the triangle grid —, the outward fp32 roundings of the covering argument and a triangle's cell
// range.  mesh.hip (the distance query) and mesh_icp.hip (ICP against a mesh) include it;
// tri_closest is the ONE function every kernel calls and the two searches exist once, so no two
// kernels can disagree on a winner.  A kernel keeps its query load, its rule for the box and its
// own record write.
#pragma once

#include <string.h>

#include <algorithm>
#include <cmath>

#include "m3d_internal.h"
#include "knn_wave.h"

namespace m3d {

// order-preserving map of a double onto unsigned integers (integer atomic min / max of coordinates
// in mesh.hip, of the triangles' doubled areas in mesh_sample.hip)
__host__ __device__ inline uint64_t ord_of(double x) {
  uint64_t b;
  memcpy(&b, &x, sizeof b);
  return (b >> 63) != 0 ? ~b : (b | 0x8000000000000000ull);
}
inline double ord_inv(uint64_t k) {
  const uint64_t b = (k >> 63) != 0 ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k;
  double x;
  memcpy(&x, &b, sizeof x);
  return x;
}

struct TriHit {
  double d2, pt[3], v, w;
  int region;
};

// the contract's dot product: (x0*y0 + x1*y1) + x2*y2
__device__ __forceinline__ double tri_dot3(const double* x, const double* y) {
  return (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2];
}

// closest(p, (a, b, c)) of the contract
__device__ __forceinline__ void tri_closest(const double* a, const double* b, const double* c, const double* p,
                                            TriHit& h) {
  const double ab[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]};
  const double ac[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
  const double ap[3] = {p[0] - a[0], p[1] - a[1], p[2] - a[2]};
  const double d1 = tri_dot3(ab, ap), d2 = tri_dot3(ac, ap);
  auto done = [&](int region, double x, double y, double z, double v, double w) {
    h.pt[0] = x, h.pt[1] = y, h.pt[2] = z;
    h.v = v, h.w = w, h.region = region;
    h.d2 = d2_exact(h.pt, p);
  };
  if (d1 <= 0.0 && d2 <= 0.0) return done(0, a[0], a[1], a[2], 0.0, 0.0);
  const double bp[3] = {p[0] - b[0], p[1] - b[1], p[2] - b[2]};
  const double d3 = tri_dot3(ab, bp), d4 = tri_dot3(ac, bp);
  if (d3 >= 0.0 && d4 <= d3) return done(1, b[0], b[1], b[2], 1.0, 0.0);
  const double vc = d1 * d4 - d3 * d2;
  if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) {
    const double v = d1 / (d1 - d3);
    return done(3, a[0] + ab[0] * v, a[1] + ab[1] * v, a[2] + ab[2] * v, v, 0.0);
  }
  const double cp[3] = {p[0] - c[0], p[1] - c[1], p[2] - c[2]};
  const double d5 = tri_dot3(ab, cp), d6 = tri_dot3(ac, cp);
  if (d6 >= 0.0 && d5 <= d6) return done(2, c[0], c[1], c[2], 0.0, 1.0);
  const double vb = d5 * d2 - d1 * d6;
  if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) {
    const double w = d2 / (d2 - d6);
    return done(4, a[0] + ac[0] * w, a[1] + ac[1] * w, a[2] + ac[2] * w, 0.0, w);
  }
  const double va = d3 * d6 - d5 * d4;
  if (va <= 0.0 && (d4 - d3) >= 0.0 && (d5 - d6) >= 0.0) {
    const double w = (d4 - d3) / ((d4 - d3) + (d5 - d6));
    return done(5, b[0] + (c[0] - b[0]) * w, b[1] + (c[1] - b[1]) * w, b[2] + (c[2] - b[2]) * w, 1.0 - w, w);
  }
  const double s = (va + vb) + vc;
  const double v = vb / s, w = vc / s;
  return done(6, (a[0] + ab[0] * v) + ac[0] * w, (a[1] + ab[1] * v) + ac[1] * w, (a[2] + ab[2] * v) + ac[2] * w, v,
              w);
}

// a running (d², index) minimum: a NaN d² never enters, the first candidate always does
__device__ __forceinline__ void take_min(double& bd, int32_t& bt, double d, int32_t t) {
  if (t >= 0 && d == d && (bt < 0 || key_less(d, t, bd, bt))) {
    bd = d;
    bt = t;
  }
}

// an fp32 at or below the real x − w / at or above the real x + w (w ≥ 0; mesh.hip's header, (1))
__device__ __forceinline__ float below(double x, float w) {
  return nextafterf(__double2float_rd(x - (double)w), -INFINITY);
}
__device__ __forceinline__ float above(double x, float w) {
  return nextafterf(__double2float_ru(x + (double)w), INFINITY);
}

// a triangle's cell range: its box's fp32 ends rounded outward and widened by the margin (mesh.hip's
// header, (1))
__device__ __forceinline__ void tri_cells(const double* __restrict__ t9, const TriGridDev& g, int lo[3], int hi[3]) {
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double mn = fmin(fmin(t9[k], t9[3 + k]), t9[6 + k]);
    const double mx = fmax(fmax(t9[k], t9[3 + k]), t9[6 + k]);
    lo[k] = grid_coord(below(mn, g.margin), g.o[k], g.inv_h, g.n[k]);
    hi[k] = grid_coord(above(mx, g.margin), g.o[k], g.inv_h, g.n[k]);
  }
}

// THE BRUTE-FORCE SWEEP: the minimum (bd, bt) of one thread's query q over all nf triangles, the
// usable ones (ok), staged through LDS in tiles of kMeshBruteTile by the kBlock threads of the block.
// Every thread of the block calls it; one without a query (valid false) stages and takes no minimum.
// s9: kMeshBruteTile × 9 doubles of LDS, sok: kMeshBruteTile bytes.  nf == 0: no tile is read.
template <int kBlock>
__device__ __forceinline__ void tri_min_brute(const double* __restrict__ tri9, const uint8_t* __restrict__ ok,
                                              int64_t nf, const double q[3], bool valid, double* s9, uint8_t* sok,
                                              double& bd, int32_t& bt) {
  bd = INFINITY;
  bt = -1;
  for (int64_t f0 = 0; f0 < nf; f0 += kMeshBruteTile) {
    const int cnt = (int)std::min<int64_t>(kMeshBruteTile, nf - f0);
    __syncthreads();
    for (int k = threadIdx.x; k < cnt * 9; k += kBlock) s9[k] = tri9[9 * f0 + k];
    for (int k = threadIdx.x; k < cnt; k += kBlock) sok[k] = ok[f0 + k];
    __syncthreads();
    if (!valid) continue;
    for (int j = 0; j < cnt; ++j) {
      if (!sok[j]) continue;
      TriHit h;
      tri_closest(s9 + 9 * j, s9 + 9 * j + 3, s9 + 9 * j + 6, q, h);
      take_min(bd, bt, h.d2, (int32_t)(f0 + j));
    }
  }
}

// THE BOX WALK: one wave's minimum of its query q over the triangles referenced from the cells
// [c0, c1] of the grid g, in two steps.  tri_box_walk: the cell rows of the box, lanes over a row's
// references, each lane folding what it meets into its own (bd, bt) — which comes in as (+inf, −1)
// or as a candidate all lanes hold alike (a seed).  tri_wave_min: the butterfly that leaves the
// wave's minimum in EVERY lane.  tri_min_box is both; a kernel that walks no box for some queries
// (mesh_icp.hip: a point that is not finite) calls the steps.  The order of the references changes
// nothing under the minimum, nor does a triangle met more than once.
__device__ __forceinline__ void tri_box_walk(const double* __restrict__ tri9, const TriGridDev& g, const int c0[3],
                                             const int c1[3], int lane, const double q[3], double& bd, int32_t& bt) {
  for (int cz = c0[2]; cz <= c1[2]; ++cz)
    for (int cy = c0[1]; cy <= c1[1]; ++cy) {
      const int64_t row = ((int64_t)cz * g.n[1] + cy) * g.n[0];
      const int32_t j0 = g.start[row + c0[0]], j1 = g.start[row + c1[0] + 1];
      for (int32_t j = j0 + lane; j < j1; j += kWave) {
        const int32_t t = g.refs[j];
        const double* t9 = tri9 + 9 * (int64_t)t;
        TriHit h;
        tri_closest(t9, t9 + 3, t9 + 6, q, h);
        take_min(bd, bt, h.d2, t);
      }
    }
}
__device__ __forceinline__ void tri_wave_min(double& bd, int32_t& bt) {
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) {
    const double od = xor_lane_f64(bd, o);
    const int32_t ot = xor_lane(bt, o, kWave);
    take_min(bd, bt, od, ot);
  }
}
__device__ __forceinline__ void tri_min_box(const double* __restrict__ tri9, const TriGridDev& g, const int c0[3],
                                            const int c1[3], int lane, const double q[3], double& bd, int32_t& bt) {
  tri_box_walk(tri9, g, c0, c1, lane, q, bd, bt);
  tri_wave_min(bd, bt);
}

// (float)x rounded toward −inf / +inf on the host
inline float float_down(double x) {
  float f = (float)x;
  if ((double)f > x) f = std::nextafterf(f, -INFINITY);
  return f;
}
inline float float_up(double x) {
  float f = (float)x;
  if ((double)f < x) f = std::nextafterf(f, INFINITY);
  return f;
}

}  // namespace m3d
