// mesh_ray.hip — ray casting against a mesh on the device: for every ray its first hit (t, the
// triangle, the barycentric (u, v)) or the number of triangles it hits (Open3D
// t.geometry.RaycastingScene.cast_rays / count_intersections; occupancy and the sign of the signed
// distance are ray parity on top of the count).
//
// CONTRACT (mesh_ray.h, restated in numpy by tests/mesh_ray_restatement.py).  fp64, one operation at
// a time; ray_tri (mesh_ray.h) is the ONE function every kernel calls: Woop, Benthin and Wald's
// watertight test.  Unusable triangles (mesh.hip's ok flags) are skipped.  FIRST HIT: the smallest
// (t, triangle) under key_less over the usable triangles that hit; a miss gives t = +inf, triangle
// −1, NaN uv.  COUNT: the number of usable triangles that hit, int32.  A ray with a component that
// is not finite, with d == 0, or called with !(tnear ≤ tfar), hits nothing.
//
// BRUTE PATH (ray_brute_kernel), the definition: one thread per ray, the triangles staged through
// LDS in tiles of kMeshBruteTile × 9 doubles, as mesh.hip's brute kernel stages them.
//
// GRID PATH (ray_grid_kernel) on the mesh's triangle grid (mesh_grid_build), one ray per lane.
// Write z for the coordinate on the ray's dominant axis kz, x and y for the other two, and
// L(z) = (ox + Sx·(z − oz), oy + Sy·(z − oz), z) for the line through the ray with the fp64 slopes
// Sx, Sy taken as exact numbers (|Sx|, |Sy| ≤ 1).  The z-range of interest is
//   [zlo, zhi] = [min(oz + tnear·dz, oz + tfar·dz) − 2m, max(…) + 2m] ∩ [box_lo − 2m, box_hi + 2m],
// m the grid's margin and box the usable triangles' box.  It is cut into SLABS by the faces
// B(k) = (float)(go + k·h) (go the grid's origin on kz, h its cell; a non-decreasing sequence of
// fp32 numbers): slab k is [max(B(k), zlo), min(B(k+1), zhi)], the first slab starting at zlo and
// the last ending at zhi, k from floor((zlo − go)/h) to floor((zhi − go)/h), both clamped to the
// grid.  Consecutive slabs share a face, so the slabs cover [zlo, zhi] whatever the rounding of the
// two floors did (a slab that comes out inverted is empty and its neighbour starts at zlo).  For a
// slab [za, zb] the RECTANGLE of cells (slab_rect, the one function the walk and the count rule
// call) is
//   on kz:   [cell(rd(za)), cell(prev(B(k+1)))], or [cell(rd(za)), cell(rd(zb))] where zb = zhi
//            (rd: fp64 → fp32 rounded down, prev: one fp32 step down): every real z of [za, zb) has
//            rd(z) between those two numbers, and z = B(k+1) itself belongs to the next slab;
//   on x, y: [cell(below(min(xa, xb), m)), cell(above(max(xa, xb), m))] with xa, xb the computed
//            x of L at za and zb — L is linear, so its extent over the slab is the extent of its
//            two ends, and below / above (mesh_tri.h) widen it by m, which pays for the rounding of
//            the two evaluations (a few 2^-53·(|o| + box), see the proviso);
//   cell is grid_coord (nnkey.h), as for the triangles' ranges.  A slab whose widened x or y extent
//   lies wholly outside the box widened by 2m holds no cell.
// The ray walks its slabs in the order of increasing t and tests every reference of every cell of
// each rectangle with ray_tri.
//
// Covering argument.  Let a triangle T be accepted by the COMPUTED test with the computed t, and
// P = L(oz + t·dz) the point of the line at that parameter.
//  (1) Provided P lies inside T's box widened by m on every axis (the proviso below), T is
//      referenced from a cell of a visited rectangle.  T's range on an axis is [cell(lo_f),
//      cell(hi_f)] with lo_f ≤ box_min − m and hi_f ≥ box_max + m (mesh.hip's header, (1)), so
//      lo_f ≤ P ≤ hi_f per axis.  tnear ≤ t ≤ tfar puts Pz between oz + tnear·dz and oz + tfar·dz,
//      and the proviso puts it inside the mesh's box widened by m, so Pz ∈ [zlo, zhi] (the 2m pay
//      for the rounding of the two products and sums) and Pz lies in some slab [za, zb].  On kz:
//      rd(Pz) is an fp32 with lo_f ≤ rd(Pz) ≤ hi_f and rect_lo ≤ rd(Pz) ≤ rect_hi (if Pz = zb the
//      next slab's rectangle has it), so by the monotonicity of cell both ranges contain
//      cell(rd(Pz)).  On x (y alike): Px lies between the real x of L at za and zb, which the
//      rectangle's fp32 ends enclose; lo_f ≤ Px ≤ rect_hi_f and rect_lo_f ≤ Px ≤ hi_f give
//      cell(lo_f) ≤ cell(rect_hi_f) and cell(rect_lo_f) ≤ cell(hi_f): two integer ranges of which
//      neither ends before the other begins meet.  So some cell of the rectangle references T.
//  (2) First hit, early stop.  After the slab whose face in the direction of travel is ze the walk
//      stops once z_best = oz + t_best·dz (computed) is on the near side of ze by more than m.  A
//      triangle the remaining slabs alone reference has, by (1), its P in none of the visited slabs:
//      Pz is at or beyond ze, so its t is strictly greater than t_best (z grows strictly with t
//      along the direction of travel; m pays for the rounding of z_best).  Strictly greater, so no
//      tie with a lower index is lost either.  Duplicates are harmless under the minimum.
//  (3) Count.  A triangle is referenced from several cells and may be met in several rectangles; a
//      hit counts only at the FIRST cell, in the order of the walk, that lies both in a rectangle
//      and in the triangle's own cell range (tri_cells, recomputed): the cell must be the
//      component-wise larger of the two ranges' lower ends in its own rectangle, and no earlier
//      slab's rectangle (slab_rect, recomputed) may meet the triangle's range.  The rule is integer
//      only and ray_tri gives the same answer wherever it is called, so each accepted triangle that
//      (1) covers counts exactly once.
//  The proviso.  The computed t is a weighted mean of the three Az = Sz·(a − o)[kz] with weights
//  U, V, W of one sign, and the accepted (U, V, W) place L within a few 2^-53·|a − o| of the
//  triangle, times the triangle's aspect.  The kernel keeps |o| ≤ 2^18·S (S = 2^24·m ≥ the largest
//  |coordinate| of the mesh), so those errors are about 2^-33·S against m = 2^-24·S: 2^9 to spare
//  for the aspect.  A sliver so thin that an accepted hit's P leaves its own box by more than m may
//  be missed by the grid path; the brute path is the definition.
//
// WHOLE-GRID FALLBACK.  A ray whose origin is farther than 2^18·S, or whose origin or direction is
// outside fp32's comfortable range (the 0x1p120 test of mesh_grid_kernel), takes one rectangle: the
// whole grid, each cell's references once, with the same count rule (a hit counts in the first cell
// of the triangle's range).  Every usable triangle is referenced from some cell, so the fallback is
// the brute path in another order.  Fallback rays are counted (an integer atomic) and reported by
// m3d_mesh_ray_info.
//
// No floating-point atomics, no device-side spinning, no dependence between rays: two calls give the
// same bits.
#include <float.h>

#include <algorithm>
#include <cmath>
#include <string>

#include "m3d_internal.h"
#include "knn_wave.h"
#include "mesh_tri.h"
#include "mesh_ray.h"

namespace m3d {
namespace {

constexpr int kRayBlock = 256;      // brute path: the block that stages a tile
constexpr int kRayGridBlock = 64;   // grid path: one wave, rays over lanes

struct RayOut {
  double* t;
  int32_t* tri;
  double* uv;
  int32_t* count;
};

// ray i of the call; a thread without a ray gets one that hits nothing
__device__ __forceinline__ void load_ray(const double* __restrict__ rays, int64_t i, bool valid, RaySetup& s) {
  double o[3] = {0.0, 0.0, 0.0}, d[3] = {0.0, 0.0, 0.0};
  if (valid) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      o[k] = rays[6 * i + k];
      d[k] = rays[6 * i + 3 + k];
    }
  }
  ray_setup(o, d, s);
}

// the first-hit outputs of ray i from its winner bt (−1: none), the winner's test evaluated again
// (the same function on the same operands: the same bits as in the scan)
__device__ __forceinline__ void write_first(const RayOut& o, int64_t i, const double* __restrict__ tri9,
                                            const RaySetup& s, double tnear, double tfar, int32_t bt) {
  const double nan = __longlong_as_double(0x7FF8000000000000ll);
  RayHit h{INFINITY, nan, nan};
  if (bt >= 0) {
    const double* t9 = tri9 + 9 * (int64_t)bt;
    ray_tri(s, t9, t9 + 3, t9 + 6, tnear, tfar, h);
  }
  if (o.t != nullptr) o.t[i] = h.t;
  if (o.tri != nullptr) o.tri[i] = bt;
  if (o.uv != nullptr) {
    o.uv[2 * i] = h.u;
    o.uv[2 * i + 1] = h.v;
  }
}

// ------------------------------------------------------------------------------- brute path
template <bool kCount>
__global__ __launch_bounds__(kRayBlock) void ray_brute_kernel(const double* __restrict__ rays, int64_t n, double tnear,
                                                              double tfar, const double* __restrict__ tri9,
                                                              const uint8_t* __restrict__ ok, int64_t nf, RayOut out) {
  __shared__ double s9[kMeshBruteTile * 9];
  __shared__ uint8_t sok[kMeshBruteTile];
  const int64_t i = (int64_t)blockIdx.x * kRayBlock + threadIdx.x;
  const bool valid = i < n;
  RaySetup s;
  load_ray(rays, i, valid, s);
  const bool live = valid && s.ok && tnear <= tfar;
  double bd = INFINITY;
  int32_t bt = -1, cnt = 0;
  for (int64_t f0 = 0; f0 < nf; f0 += kMeshBruteTile) {
    const int tile = (int)std::min<int64_t>(kMeshBruteTile, nf - f0);
    __syncthreads();
    for (int k = threadIdx.x; k < tile * 9; k += kRayBlock) s9[k] = tri9[9 * f0 + k];
    for (int k = threadIdx.x; k < tile; k += kRayBlock) sok[k] = ok[f0 + k];
    __syncthreads();
    if (!live) continue;
    for (int j = 0; j < tile; ++j) {
      if (!sok[j]) continue;
      RayHit h;
      if (!ray_tri(s, s9 + 9 * j, s9 + 9 * j + 3, s9 + 9 * j + 6, tnear, tfar, h)) continue;
      if (kCount)
        ++cnt;
      else
        take_min(bd, bt, h.t, (int32_t)(f0 + j));
    }
  }
  if (!valid) return;
  if (kCount)
    out.count[i] = cnt;
  else
    write_first(out, i, tri9, s, tnear, tfar, bt);
}

// ------------------------------------------------------------------------------- grid path
// what the walk needs of the mesh beside its grid: the usable triangles' box widened by 2m, and the
// bound on |o| of the proviso
struct RayGridArgs {
  double blo[3], bhi[3];
  double far;
};

__device__ __forceinline__ int picki(const int* x, int k) { return k == 0 ? x[0] : (k == 1 ? x[1] : x[2]); }
__device__ __forceinline__ float pickf(const float* x, int k) { return k == 0 ? x[0] : (k == 1 ? x[1] : x[2]); }

// a ray's walk: everything in the order (kz, kx, ky) of the ray's axes
struct RayWalk {
  bool whole;          // the fallback: one rectangle, the whole grid
  bool fwd;            // z grows with t
  int nsteps, k0, k1;  // slabs k0..k1, walked from k0 (fwd) or from k1
  double zlo, zhi;
  double goz, hd, md;  // the grid's origin on kz, its cell and margin as doubles
  float fz, fx, fy;    // the grid's origin per axis
  int nz, nx, ny;
  int64_t sz, sx, sy;  // a cell's stride per axis
  double bxlo, bxhi, bylo, byhi;
};
struct CellRect {
  int z0, z1, x0, x1, y0, y1;
};

__device__ __forceinline__ float slab_face(const RayWalk& w, int k) {
  return __double2float_rn(w.goz + (double)k * w.hd);
}

__device__ __forceinline__ void ray_walk_setup(const RaySetup& s, const TriGridDev& g, const RayGridArgs& a,
                                               double tnear, double tfar, RayWalk& w) {
  w.fz = pickf(g.o, s.kz), w.fx = pickf(g.o, s.kx), w.fy = pickf(g.o, s.ky);
  w.nz = picki(g.n, s.kz), w.nx = picki(g.n, s.kx), w.ny = picki(g.n, s.ky);
  const int64_t st[3] = {1, (int64_t)g.n[0], (int64_t)g.n[0] * g.n[1]};
  w.sz = s.kz == 0 ? st[0] : (s.kz == 1 ? st[1] : st[2]);
  w.sx = s.kx == 0 ? st[0] : (s.kx == 1 ? st[1] : st[2]);
  w.sy = s.ky == 0 ? st[0] : (s.ky == 1 ? st[1] : st[2]);
  w.goz = (double)w.fz;
  w.hd = 1.0 / (double)g.inv_h;
  w.md = (double)g.margin;
  w.bxlo = pick3(a.blo, s.kx), w.bxhi = pick3(a.bhi, s.kx);
  w.bylo = pick3(a.blo, s.ky), w.byhi = pick3(a.bhi, s.ky);
  w.fwd = s.dz > 0.0;
  // the proviso's bound on the origin, and fp32's comfortable range for origin and direction
  // (|d[kx]|, |d[ky]| ≤ |d[kz]| = |dz|)
  const bool near = fabs(s.ox) <= a.far && fabs(s.oy) <= a.far && fabs(s.oz) <= a.far && fabs(s.ox) <= 0x1p120 &&
                    fabs(s.oy) <= 0x1p120 && fabs(s.oz) <= 0x1p120 && fabs(s.dz) <= 0x1p120;
  w.whole = !near;
  if (w.whole) {
    w.nsteps = 1, w.k0 = w.k1 = 0;
    w.zlo = w.zhi = 0.0;
    return;
  }
  const double zA = s.oz + tnear * s.dz, zB = s.oz + tfar * s.dz;
  w.zlo = fmax(fmin(zA, zB) - 2.0 * w.md, pick3(a.blo, s.kz));
  w.zhi = fmin(fmax(zA, zB) + 2.0 * w.md, pick3(a.bhi, s.kz));
  if (!(w.zlo <= w.zhi)) {
    w.nsteps = 0, w.k0 = w.k1 = 0;
    return;
  }
  const double top = (double)(w.nz - 1);
  w.k0 = (int)fmin(fmax(floor((w.zlo - w.goz) / w.hd), 0.0), top);
  w.k1 = (int)fmin(fmax(floor((w.zhi - w.goz) / w.hd), 0.0), top);
  w.nsteps = w.k1 - w.k0 + 1;
}

// the rectangle of cells of step `step` of the walk (the header's slab and rectangle); ze: the
// slab's face in the direction of travel.  false: the slab holds no cell.
__device__ __forceinline__ bool slab_rect(const RaySetup& s, const RayWalk& w, const TriGridDev& g, int step,
                                          CellRect& r, double& ze) {
  if (w.whole) {
    r.z0 = r.x0 = r.y0 = 0;
    r.z1 = w.nz - 1, r.x1 = w.nx - 1, r.y1 = w.ny - 1;
    ze = 0.0;
    return true;
  }
  const int k = w.fwd ? w.k0 + step : w.k1 - step;
  const float f1 = slab_face(w, k + 1);
  const double za = k == w.k0 ? w.zlo : fmax((double)slab_face(w, k), w.zlo);
  const double zb = k == w.k1 ? w.zhi : fmin((double)f1, w.zhi);
  ze = w.fwd ? zb : za;
  if (!(za <= zb)) return false;
  const double da = za - s.oz, db = zb - s.oz;
  const double xa = s.ox + s.Sx * da, xb = s.ox + s.Sx * db;
  const double ya = s.oy + s.Sy * da, yb = s.oy + s.Sy * db;
  const double xmin = fmin(xa, xb), xmax = fmax(xa, xb), ymin = fmin(ya, yb), ymax = fmax(ya, yb);
  if (xmax + w.md < w.bxlo || xmin - w.md > w.bxhi || ymax + w.md < w.bylo || ymin - w.md > w.byhi) return false;
  r.z0 = grid_coord(__double2float_rd(za), w.fz, g.inv_h, w.nz);
  r.z1 = grid_coord(zb == w.zhi ? __double2float_rd(zb) : nextafterf(f1, -INFINITY), w.fz, g.inv_h, w.nz);
  r.x0 = grid_coord(below(xmin, g.margin), w.fx, g.inv_h, w.nx);
  r.x1 = grid_coord(above(xmax, g.margin), w.fx, g.inv_h, w.nx);
  r.y0 = grid_coord(below(ymin, g.margin), w.fy, g.inv_h, w.ny);
  r.y1 = grid_coord(above(ymax, g.margin), w.fy, g.inv_h, w.ny);
  return true;
}

// the count rule: whether the cell (cz, cx, cy) of rectangle r, at step `step`, is the first cell
// of the walk inside the cell range of the triangle t9
__device__ __forceinline__ bool first_meeting(const RaySetup& s, const RayWalk& w, const TriGridDev& g,
                                              const double* __restrict__ t9, int step, const CellRect& r, int cz,
                                              int cx, int cy) {
  int tl[3], th[3];
  tri_cells(t9, g, tl, th);
  const int lz = picki(tl, s.kz), lx = picki(tl, s.kx), ly = picki(tl, s.ky);
  const int hz = picki(th, s.kz), hx = picki(th, s.kx), hy = picki(th, s.ky);
  if (cz != max(r.z0, lz) || cx != max(r.x0, lx) || cy != max(r.y0, ly)) return false;
  for (int p = 0; p < step; ++p) {
    CellRect q;
    double ze;
    if (!slab_rect(s, w, g, p, q, ze)) continue;
    if (max(q.z0, lz) <= min(q.z1, hz) && max(q.x0, lx) <= min(q.x1, hx) && max(q.y0, ly) <= min(q.y1, hy))
      return false;
  }
  return true;
}

template <bool kCount>
__global__ __launch_bounds__(kRayGridBlock) void ray_grid_kernel(const double* __restrict__ rays, int64_t n,
                                                                 double tnear, double tfar,
                                                                 const double* __restrict__ tri9, TriGridDev g,
                                                                 RayGridArgs args, uint32_t* __restrict__ fallback,
                                                                 RayOut out) {
  const int64_t i = (int64_t)blockIdx.x * kRayGridBlock + threadIdx.x;
  const bool valid = i < n;
  RaySetup s;
  load_ray(rays, i, valid, s);
  const bool live = valid && s.ok && tnear <= tfar;
  RayWalk w;
  ray_walk_setup(s, g, args, tnear, tfar, w);
  if (!live) w.nsteps = 0;
  const uint64_t fb = __ballot(live && w.whole);
  if (fb != 0 && (threadIdx.x & 63) == 0) atomicAdd(fallback, (uint32_t)__popcll(fb));
  double bd = INFINITY;
  int32_t bt = -1, cnt = 0;
  for (int step = 0; step < w.nsteps; ++step) {
    CellRect r;
    double ze;
    if (!slab_rect(s, w, g, step, r, ze)) continue;
    for (int cz = r.z0; cz <= r.z1; ++cz)
      for (int cy = r.y0; cy <= r.y1; ++cy)
        for (int cx = r.x0; cx <= r.x1; ++cx) {
          const int64_t cell = (int64_t)cz * w.sz + (int64_t)cx * w.sx + (int64_t)cy * w.sy;
          const int32_t j1 = g.start[cell + 1];
          for (int32_t j = g.start[cell]; j < j1; ++j) {
            const int32_t t = g.refs[j];
            const double* t9 = tri9 + 9 * (int64_t)t;
            RayHit h;
            if (!ray_tri(s, t9, t9 + 3, t9 + 6, tnear, tfar, h)) continue;
            if (kCount) {
              if (first_meeting(s, w, g, t9, step, r, cz, cx, cy)) ++cnt;
            } else {
              take_min(bd, bt, h.t, t);
            }
          }
        }
    if (!kCount && !w.whole && bt >= 0) {  // the header's (2)
      const double zbest = s.oz + bd * s.dz;
      if (w.fwd ? zbest + w.md < ze : zbest - w.md > ze) break;
    }
  }
  if (!valid) return;
  if (kCount)
    out.count[i] = cnt;
  else
    write_first(out, i, tri9, s, tnear, tfar, bt);
}

}  // namespace

hipError_t mesh_rays_brute(const m3d_mesh* m, const double* rays, int64_t n, double tnear, double tfar, double* t_out,
                           int32_t* tri_out, double* uv_out, int32_t* count_out, hipStream_t st) {
  if (n == 0) return hipSuccess;
  const unsigned blocks = (unsigned)((n + kRayBlock - 1) / kRayBlock);
  const RayOut out{t_out, tri_out, uv_out, count_out};
  if (count_out != nullptr)
    ray_brute_kernel<true><<<blocks, kRayBlock, 0, st>>>(rays, n, tnear, tfar, m->tri9, m->ok, m->nf, out);
  else
    ray_brute_kernel<false><<<blocks, kRayBlock, 0, st>>>(rays, n, tnear, tfar, m->tri9, m->ok, m->nf, out);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  return e;
}

hipError_t mesh_rays_grid(m3d_ctx* ctx, m3d_mesh* m, const double* rays, int64_t n, double tnear, double tfar,
                          double* t_out, int32_t* tri_out, double* uv_out, int32_t* count_out, void* scratch,
                          int64_t* fallback_out, hipStream_t st, std::string* why) {
  *fallback_out = 0;
  if (n == 0) return hipSuccess;
  hipError_t e = mesh_grid_build(ctx, m, st, why);
  if (e != hipSuccess) return e;
  const TriGridDev& g = m->grid;
  RayGridArgs a;
  const double md = (double)g.margin;
  for (int k = 0; k < 3; ++k) {
    a.blo[k] = m->lo[k] - 2.0 * md;
    a.bhi[k] = m->hi[k] + 2.0 * md;
  }
  a.far = 0x1p42 * md;  // 2^18·S with S = 2^24·m
  uint32_t* dfb = static_cast<uint32_t*>(scratch);
  if ((e = hipMemsetAsync(dfb, 0, sizeof(uint32_t), st)) != hipSuccess) return e;
  const unsigned blocks = (unsigned)((n + kRayGridBlock - 1) / kRayGridBlock);
  const RayOut out{t_out, tri_out, uv_out, count_out};
  if (count_out != nullptr)
    ray_grid_kernel<true><<<blocks, kRayGridBlock, 0, st>>>(rays, n, tnear, tfar, m->tri9, g, a, dfb, out);
  else
    ray_grid_kernel<false><<<blocks, kRayGridBlock, 0, st>>>(rays, n, tnear, tfar, m->tri9, g, a, dfb, out);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  uint32_t fb = 0;
  if ((e = hipMemcpyAsync(&fb, dfb, sizeof fb, hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
  if ((e = hipStreamSynchronize(st)) != hipSuccess) return e;
  *fallback_out = (int64_t)fb;
  return hipSuccess;
}

}  // namespace m3d
