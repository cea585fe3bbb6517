// mesh.hip — point-to-mesh distance on the device: for every query the closest triangle of a mesh,
// the closest point on it, its barycentric (v, w) and the Voronoi region it fell in (Open3D
// t.geometry.RaycastingScene.compute_closest_points / compute_distance).
//
// CONTRACT (restated in numpy by tests/mesh_restatement.py).  All arithmetic is fp64, one
// operation at a time (-ffp-contract=off), every dot product x·y = (x0*y0 + x1*y1) + x2*y2.
// The query is p, or q64_of(T, p) (nnkey.h) when a transform is given.  A triangle is (a, b, c),
// the fp64 vertices its three indices name.  closest(p, tri) is Ericson's closest point on a
// triangle (Real-Time Collision Detection §5.1.5), the seven Voronoi regions tested in this order —
// tri_closest (mesh_tri.h) is the ONE function every kernel calls:
//   ab = b−a, ac = c−a, ap = p−a; d1 = ab·ap, d2 = ac·ap.
//     region 0 (A)  if d1 ≤ 0 && d2 ≤ 0:                       point a,            (v, w) = (0, 0)
//   bp = p−b; d3 = ab·bp, d4 = ac·bp.
//     region 1 (B)  if d3 ≥ 0 && d4 ≤ d3:                      point b,            (1, 0)
//   vc = d1*d4 − d3*d2.
//     region 3 (AB) if vc ≤ 0 && d1 ≥ 0 && d3 ≤ 0:  v = d1/(d1−d3), point a + ab*v,      (v, 0)
//   cp = p−c; d5 = ab·cp, d6 = ac·cp.
//     region 2 (C)  if d6 ≥ 0 && d5 ≤ d6:                      point c,            (0, 1)
//   vb = d5*d2 − d1*d6.
//     region 4 (AC) if vb ≤ 0 && d2 ≥ 0 && d6 ≤ 0:  w = d2/(d2−d6), point a + ac*w,      (0, w)
//   va = d3*d6 − d5*d4.
//     region 5 (BC) if va ≤ 0 && (d4−d3) ≥ 0 && (d5−d6) ≥ 0:
//                       w = (d4−d3)/((d4−d3)+(d5−d6)), point b + (c−b)*w,                (1−w, w)
//     region 6 (face) otherwise: s = (va+vb)+vc, v = vb/s, w = vc/s, point (a + ab*v) + ac*w.
//   d² = d2_exact(point, p) (knn_wave.h).
// A triangle is USABLE when its nine coordinates are finite and ab × ac = (ab1*ac2 − ab2*ac1,
// ab2*ac0 − ab0*ac2, ab0*ac1 − ab1*ac0) is not three exact zeros; the others are skipped.  The
// winner of a query is the smallest (d², triangle index) under key_less (knn_wave.h) over ALL
// usable triangles whose d² is not NaN: bit-equal distances go to the lower index.  Outputs: d²,
// the triangle, the point, (v, w) — point ≈ (1−v−w)·a + v·b + w·c — and the region.  A query no
// triangle answers (every d² NaN: a NaN query) gets d² = +inf, triangle −1, NaN point and uv,
// region 255.  A mesh without a usable triangle is an error of the call, not a fault.
//
// The winner is defined over all triangles, so the two paths below cannot differ: they evaluate
// the same function on the same operands and take the same minimum.
//
// BRUTE PATH (mesh_brute_kernel): one thread per query, the triangles staged through LDS in tiles
// of kMeshBruteTile × 9 doubles.  The reference path, and the path for small meshes.
//
// GRID PATH.  A uniform grid over the mesh's bounding box; every usable triangle is referenced
// from every cell its axis-aligned box overlaps (count pass, prefix sum, fill pass: integer
// atomics only; the order of a cell's references changes nothing under a minimum, nor does a
// triangle met more than once).  The cell size starts at cbrt(box volume / F) and doubles while
// the count pass finds more than 16·F references (or the grid more cells than its budget), so one
// huge triangle over a fine grid cannot blow the allocation up.  One wave per query walks the
// cell rows of the query's box, lanes over the references, each lane evaluating tri_closest in
// fp64; a butterfly takes the wave's minimum (d², index).
//
// Covering argument.  Let m = 2^-24 · (largest |coordinate| of the mesh's box) be the margin.
//  (1) Cell ranges.  below(x, w) is an fp32 at or below the real x − w, above(x, w) one at or above
//      x + w (the fp64 sum converted with directed rounding, then one fp32 step further out, which
//      pays for the fp64 sum's half ulp).  A triangle's range on an axis is [cell(lo_f), cell(hi_f)]
//      with lo_f = below(min, m), hi_f = above(max, m): its box rounded OUTWARD and widened by m.  A
//      query's range for the half-width Rf (fp32) is [cell(below(q, Rf)), cell(above(q, Rf))]: in
//      real numbers it contains [q − Rf, q + Rf].  cell is
//      grid_coord (nnkey.h), the same expression for both, and it is monotone (a subtraction, a
//      product by a positive number, a clamp, a truncation), clamping included: coordinates outside
//      the grid share its edge cells.
//  (2) Every triangle whose COMPUTED closest point c lies inside the query's real box [q ± Rf] is
//      referenced from a cell of the scanned box, provided c lies inside the triangle's widened box:
//      lo_f ≤ c ≤ hi_f and q − Rf ≤ c ≤ q + Rf give, by monotonicity, cell(lo_f) ≤ cell(c) ≤
//      cell(hi_f) and cell(query lo) ≤ cell(c) ≤ cell(query hi) on every axis, so the ranges meet.
//      Conversely a triangle NOT referenced from the scanned box has, on some axis, |c − q| > Rf in
//      real numbers; the rounded difference is then ≥ Rf in magnitude (rounding is monotone, Rf is
//      a double), its square ≥ Rf² (exact in fp64: 48 bits), and d² — a sum of it and two
//      non-negative squares — is ≥ Rf².  So a query whose best d² is STRICTLY below (double)Rf² has
//      its global winner: every unscanned triangle is strictly farther.
//      The proviso: a vertex region returns a vertex exactly; an edge region a + e*t with t ∈ [0, 1]
//      (d1 ≥ 0 ≥ d3 makes d1/(d1−d3) ≤ 1 under monotone rounding), off the segment by a few ulps of
//      the coordinates; the face region's v, w carry the cancellation of va, vb, vc, an error of
//      about 2^-52·D²/L in c for a query at distance D from a triangle of edge L.  m leaves 2^28
//      ulps for it; a sliver so thin that its computed point leaves its own box by more than m may
//      be missed by the grid path (the brute path is the definition).
//
// Radius ladder (modelled on clean.hip's k-NN ladder): a host loop of launches over a compacted
// queue of unfinished queries.  Round 0 scans every query with the first radius (one cell, or the
// caller's r0).  A query is FINISHED when its best d² < Rf² for the half-width its box was cut
// with, or when its box covered the whole grid (a non-finite or huge query is given the whole
// grid).  Otherwise it is appended to the next round's queue (an integer atomic on a counter; the
// queue's order changes nothing, a query writes only its own outputs) with Rf = its best distance
// rounded up — an upper bound of the winner's, so that round finishes it — or, if it found
// nothing, twice the radius and at least its distance to the grid's box plus two cells.  Rounds
// are bounded by the grid's size (a box doubles until it covers the grid) and by kMaxRounds on the
// host, which fails with a message.  No device-side spinning, no dependence between queries, no
// floating-point atomics: two calls give the same bits.
#include <float.h>

#include <algorithm>
#include <cmath>
#include <string>

#include <hipcub/hipcub.hpp>

#include "m3d_internal.h"
#include "knn_wave.h"
#include "mesh_tri.h"

namespace m3d {
namespace {

constexpr int kMeshBlock = 256;
constexpr int kMaxRounds = 64;               // host bound of the ladder
constexpr int64_t kMaxCellsAxis = 1024;      // cells per axis
constexpr int64_t kMaxCells = (int64_t)1 << 24;
constexpr int kRefsPerTri = 16;              // the count pass's condition: references ≤ 16·F

// the optional query transform, by value (12 doubles: the rows of [R | t])
struct MeshXf {
  double m[12];
  int on;
};
struct MeshOut {
  double* d2;
  int32_t* tri;
  double* point;
  double* uv;
  uint8_t* region;
};

__device__ __forceinline__ void load_query(const double* __restrict__ xyz, int64_t i, const MeshXf& T, double q[3]) {
  const double p[3] = {xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]};
  if (T.on) {
    q64_of(T.m, p, q);
  } else {
    q[0] = p[0], q[1] = p[1], q[2] = p[2];
  }
}

// the outputs of query i from its winner bt (−1: none), the winner's closest point evaluated again
// (the same function on the same operands: the same bits as in the scan)
__device__ __forceinline__ void write_result(const MeshOut& o, int64_t i, const double* __restrict__ tri9,
                                             const double q[3], int32_t bt) {
  TriHit h;
  if (bt >= 0) {
    const double* t9 = tri9 + 9 * (int64_t)bt;
    tri_closest(t9, t9 + 3, t9 + 6, q, h);
  } else {
    const double nan = __longlong_as_double(0x7FF8000000000000ll);
    h.d2 = INFINITY;
    h.pt[0] = h.pt[1] = h.pt[2] = h.v = h.w = nan;
    h.region = 255;
  }
  if (o.d2 != nullptr) o.d2[i] = h.d2;
  if (o.tri != nullptr) o.tri[i] = bt;
  if (o.point != nullptr) {
    o.point[3 * i] = h.pt[0];
    o.point[3 * i + 1] = h.pt[1];
    o.point[3 * i + 2] = h.pt[2];
  }
  if (o.uv != nullptr) {
    o.uv[2 * i] = h.v;
    o.uv[2 * i + 1] = h.w;
  }
  if (o.region != nullptr) o.region[i] = (uint8_t)h.region;
}

// ------------------------------------------------------------------------------- upload
// (ord_of / ord_inv, the order-preserving integer image of a double: mesh_tri.h)
// what m3d_mesh_create reads back: an index out of range, the usable triangles, their box
struct MeshInfo {
  int32_t bad, usable;
  unsigned long long lo[3], hi[3];
};

// One thread per triangle: its indices are checked BEFORE any vertex is read (an index outside
// [0, nv) flags the mesh and reads nothing), its nine coordinates packed into tri9, its usable flag
// into ok; the usable triangles' box by a wave butterfly and one integer atomic per wave and bound.
__global__ __launch_bounds__(kMeshBlock) void mesh_pack_kernel(const double* __restrict__ v64, int64_t nv,
                                                               const int32_t* __restrict__ tri, int64_t nf,
                                                               double* __restrict__ tri9, uint8_t* __restrict__ ok,
                                                               MeshInfo* __restrict__ info) {
  const int64_t f = (int64_t)blockIdx.x * kMeshBlock + threadIdx.x;
  bool usable = false, bad = false;
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  if (f < nf) {
    const int32_t i0 = tri[3 * f], i1 = tri[3 * f + 1], i2 = tri[3 * f + 2];
    bad = i0 < 0 || i1 < 0 || i2 < 0 || i0 >= nv || i1 >= nv || i2 >= nv;
    double t9[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (!bad) {
      bool fin = true;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        t9[k] = v64[3 * (int64_t)i0 + k];
        t9[3 + k] = v64[3 * (int64_t)i1 + k];
        t9[6 + k] = v64[3 * (int64_t)i2 + k];
        fin = fin && isfinite(t9[k]) && isfinite(t9[3 + k]) && isfinite(t9[6 + k]);
      }
      const double ab[3] = {t9[3] - t9[0], t9[4] - t9[1], t9[5] - t9[2]};
      const double ac[3] = {t9[6] - t9[0], t9[7] - t9[1], t9[8] - t9[2]};
      const double cx = ab[1] * ac[2] - ab[2] * ac[1];
      const double cy = ab[2] * ac[0] - ab[0] * ac[2];
      const double cz = ab[0] * ac[1] - ab[1] * ac[0];
      usable = fin && !(cx == 0.0 && cy == 0.0 && cz == 0.0);
      if (usable) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          lo[k] = fmin(fmin(t9[k], t9[3 + k]), t9[6 + k]);
          hi[k] = fmax(fmax(t9[k], t9[3 + k]), t9[6 + k]);
        }
      }
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) tri9[9 * f + k] = t9[k];
    ok[f] = usable ? 1 : 0;
  }
  const uint64_t mu = __ballot(usable), mb = __ballot(bad);
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) {
      lo[k] = fmin(lo[k], __shfl_xor(lo[k], o));
      hi[k] = fmax(hi[k], __shfl_xor(hi[k], o));
    }
  if ((threadIdx.x & 63) == 0) {
    if (mb != 0) atomicOr(&info->bad, 1);
    if (mu != 0) {
      atomicAdd(&info->usable, (int32_t)__popcll(mu));
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        atomicMin(&info->lo[k], (unsigned long long)ord_of(lo[k]));
        atomicMax(&info->hi[k], (unsigned long long)ord_of(hi[k]));
      }
    }
  }
}

// ------------------------------------------------------------------------------- the grid
// the references a grid would hold (no per-cell work): Σ over usable triangles of their cell count
__global__ __launch_bounds__(kMeshBlock) void tri_refs_total_kernel(const double* __restrict__ tri9,
                                                                    const uint8_t* __restrict__ ok, int64_t nf,
                                                                    TriGridDev g, unsigned long long* __restrict__ total) {
  const int64_t f = (int64_t)blockIdx.x * kMeshBlock + threadIdx.x;
  long long c = 0;
  if (f < nf && ok[f]) {
    int lo[3], hi[3];
    tri_cells(tri9 + 9 * f, g, lo, hi);
    c = (long long)(hi[0] - lo[0] + 1) * (hi[1] - lo[1] + 1) * (hi[2] - lo[2] + 1);
  }
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) c += __shfl_xor(c, o);
  if ((threadIdx.x & 63) == 0 && c != 0) atomicAdd(total, (unsigned long long)c);
}

// kFill false: cnt[cell] += 1 for every cell of every usable triangle's range.  kFill true (after
// the prefix sum start of those counts): the triangle takes the last free slot of each cell, counting
// cnt[cell] back down.
template <bool kFill>
__global__ __launch_bounds__(kMeshBlock) void tri_cells_kernel(const double* __restrict__ tri9,
                                                               const uint8_t* __restrict__ ok, int64_t nf, TriGridDev g,
                                                               int32_t* __restrict__ cnt, const int32_t* __restrict__ start,
                                                               int32_t* __restrict__ refs) {
  const int64_t f = (int64_t)blockIdx.x * kMeshBlock + threadIdx.x;
  if (f >= nf || !ok[f]) return;
  int lo[3], hi[3];
  tri_cells(tri9 + 9 * f, g, lo, hi);
  for (int cz = lo[2]; cz <= hi[2]; ++cz)
    for (int cy = lo[1]; cy <= hi[1]; ++cy) {
      const int64_t row = ((int64_t)cz * g.n[1] + cy) * g.n[0];
      for (int cx = lo[0]; cx <= hi[0]; ++cx) {
        if (kFill)
          refs[start[row + cx] + (atomicSub(&cnt[row + cx], 1) - 1)] = (int32_t)f;
        else
          atomicAdd(&cnt[row + cx], 1);
      }
    }
}

// ------------------------------------------------------------------------------- the two paths
__global__ __launch_bounds__(kMeshBlock) void mesh_brute_kernel(const double* __restrict__ xyz, int64_t n, MeshXf T,
                                                                const double* __restrict__ tri9,
                                                                const uint8_t* __restrict__ ok, int64_t nf, MeshOut out) {
  __shared__ double s9[kMeshBruteTile * 9];
  __shared__ uint8_t sok[kMeshBruteTile];
  const int64_t i = (int64_t)blockIdx.x * kMeshBlock + threadIdx.x;
  const bool valid = i < n;
  double q[3] = {0.0, 0.0, 0.0};
  if (valid) load_query(xyz, i, T, q);
  double bd;
  int32_t bt;
  tri_min_brute<kMeshBlock>(tri9, ok, nf, q, valid, s9, sok, bd, bt);
  if (valid) write_result(out, i, tri9, q, bt);
}

// One round of the ladder, ONE WAVE per pending query.  pend_in null: round 0, wave w takes query
// w with the half-width r0; otherwise query pend_in[w] with rq[that query].
__global__ __launch_bounds__(kMeshBlock) void mesh_grid_kernel(const double* __restrict__ xyz, MeshXf T,
                                                               const double* __restrict__ tri9, TriGridDev g,
                                                               const int32_t* __restrict__ pend_in, int64_t npend,
                                                               float r0, float* __restrict__ rq,
                                                               int32_t* __restrict__ pend_out,
                                                               uint32_t* __restrict__ pend_cnt, MeshOut out) {
  const int lane = threadIdx.x & 63;
  const int64_t wq = (int64_t)blockIdx.x * (kMeshBlock / kWave) + (threadIdx.x >> 6);
  if (wq >= npend) return;  // wave-uniform
  const int64_t i = pend_in != nullptr ? (int64_t)pend_in[wq] : wq;
  double q[3];
  load_query(xyz, i, T, q);
  const float Rf = pend_in != nullptr ? rq[i] : r0;
  // a query outside fp32's comfortable range, or a half-width near its top, takes the whole grid
  const bool all = !(fabs(q[0]) <= 0x1p120 && fabs(q[1]) <= 0x1p120 && fabs(q[2]) <= 0x1p120) || !(Rf < 0x1p122f);
  int c0[3], c1[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    c0[k] = all ? 0 : grid_coord(below(q[k], Rf), g.o[k], g.inv_h, g.n[k]);
    c1[k] = all ? g.n[k] - 1 : grid_coord(above(q[k], Rf), g.o[k], g.inv_h, g.n[k]);
  }
  const bool whole = c0[0] == 0 && c0[1] == 0 && c0[2] == 0 && c1[0] == g.n[0] - 1 && c1[1] == g.n[1] - 1 &&
                     c1[2] == g.n[2] - 1;
  double bd = INFINITY;
  int32_t bt = -1;
  tri_min_box(tri9, g, c0, c1, lane, q, bd, bt);  // every lane holds the wave's minimum
  const bool finished = whole || (bt >= 0 && bd < (double)Rf * (double)Rf);
  if (lane != 0) return;
  if (finished) {
    write_result(out, i, tri9, q, bt);
    return;
  }
  float Rn;
  if (bt >= 0 && bd < (double)INFINITY) {
    Rn = __double2float_ru(sqrt(bd) * (1.0 + 0x1p-20));
  } else {  // nothing yet: twice the radius, and at least into the grid's box
    const float h = 1.0f / g.inv_h;
    double gap = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double glo = (double)g.o[k], ghi = glo + (double)g.n[k] * (double)h;
      gap = fmax(gap, fmax(glo - q[k], q[k] - ghi));
    }
    Rn = fmaxf(2.0f * Rf, __double2float_ru(gap + 2.0 * (double)h));
  }
  rq[i] = Rn <= FLT_MAX ? Rn : FLT_MAX;
  pend_out[atomicAdd(pend_cnt, 1u)] = (int32_t)i;
}

// the pieces of a grid call's scratch for n queries (null: the layout's size alone)
struct MeshScratch {
  int32_t *pend_a = nullptr, *pend_b = nullptr;
  float* rq = nullptr;
  uint32_t* cnt = nullptr;
  size_t bytes = 0;
  MeshScratch(int64_t n, void* scratch) {
    Carve cv;
    cv.add(&pend_a, (size_t)n);
    cv.add(&pend_b, (size_t)n);
    cv.add(&rq, (size_t)n);
    cv.add(&cnt, kMaxRounds);
    bytes = cv.bytes();
    if (scratch != nullptr) cv.place(scratch);
  }
};

// the grid of cell h over the mesh's box: origin below every widened triangle end, dimensions
// clamped to ≥ 1; false when it would hold more cells than the budget
bool grid_shape(const m3d_mesh* m, double h, TriGridDev* g) {
  double S = 0.0;
  for (int k = 0; k < 3; ++k) S = std::max({S, std::fabs(m->lo[k]), std::fabs(m->hi[k])});
  g->margin = std::max(float_up(S * 0x1p-24), FLT_MIN);
  g->inv_h = (float)(1.0 / h);
  int64_t cells = 1;
  for (int k = 0; k < 3; ++k) {
    g->o[k] = std::nextafterf(float_down(m->lo[k] - (double)g->margin), -INFINITY);  // = below(lo, margin)
    const double nk = std::floor((m->hi[k] - m->lo[k]) / h) + 1.0;
    if (!(nk <= (double)kMaxCellsAxis)) return false;
    g->n[k] = (int)std::max(nk, 1.0);
    cells *= g->n[k];
  }
  g->ncells = cells;
  return cells <= kMaxCells;
}

}  // namespace

size_t mesh_scratch_bytes(int64_t n) { return n > 0 ? MeshScratch(n, nullptr).bytes : 0; }

hipError_t mesh_upload(m3d_mesh* m, hipStream_t st, int* bad_index) {
  *bad_index = 0;
  m->usable = 0;
  if (m->nf == 0) return hipSuccess;  // nothing to pack, nothing to read back
  MeshInfo h, *d = nullptr;
  hipError_t e = dev_malloc(&d, sizeof(MeshInfo));
  if (e != hipSuccess) return e;
  h.bad = h.usable = 0;
  for (int k = 0; k < 3; ++k) {
    h.lo[k] = ~0ull;
    h.hi[k] = 0ull;
  }
  e = hipMemcpyAsync(d, &h, sizeof h, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) {
    const unsigned blocks = (unsigned)((m->nf + kMeshBlock - 1) / kMeshBlock);
    mesh_pack_kernel<<<blocks, kMeshBlock, 0, st>>>(m->v64, m->nv, m->tri, m->nf, m->tri9, m->ok, d);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(&h, d, sizeof h, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  (void)hipFree(d);
  if (e != hipSuccess) return e;
  *bad_index = h.bad;
  if (h.bad != 0) return hipSuccess;
  m->usable = h.usable;
  for (int k = 0; k < 3; ++k) {
    m->lo[k] = h.usable > 0 ? ord_inv(h.lo[k]) : 0.0;
    m->hi[k] = h.usable > 0 ? ord_inv(h.hi[k]) : 0.0;
  }
  return hipSuccess;
}

// the triangle grid of a mesh with usable triangles, built once (synchronous)
hipError_t mesh_grid_build(m3d_ctx* ctx, m3d_mesh* m, hipStream_t st, std::string* why) {
  if (m->grid_built) return hipSuccess;
  if (m->gblock != nullptr) {  // a build that failed half way
    block_release(m->gblock);
    m->gblock = nullptr;
  }
  const int64_t F = m->usable;
  double ext[3], emax = 0.0;
  for (int k = 0; k < 3; ++k) {
    ext[k] = m->hi[k] - m->lo[k];
    emax = std::max(emax, ext[k]);
  }
  if (!(emax > 0.0) || !std::isfinite(emax)) {
    *why = "mesh grid: the usable triangles' box is empty or not finite";
    return hipErrorUnknown;
  }
  // the first cell: cbrt(box volume / F), a flat axis counted as 1e-4 of the longest (a planar
  // mesh then starts too fine and the count pass below coarsens it)
  double vol = 1.0;
  for (int k = 0; k < 3; ++k) vol *= std::max(ext[k], 1e-4 * emax);
  double h = std::cbrt(vol / (double)F);
  if (!(h > 0.0) || !std::isfinite(h)) h = emax;
  hipError_t e = ctx->tmp.reserve(256);
  if (e != hipSuccess) return e;
  const unsigned blocks = (unsigned)((m->nf + kMeshBlock - 1) / kMeshBlock);
  TriGridDev g{};
  unsigned long long total = 0;
  int doublings = 0;
  for (;; h *= 2.0, ++doublings) {
    if (doublings > 2200) {  // fp64 has no more doublings to give
      *why = "mesh grid: no cell size satisfies the reference budget";
      return hipErrorUnknown;
    }
    if (!grid_shape(m, h, &g)) continue;
    unsigned long long* dtot = reinterpret_cast<unsigned long long*>(ctx->tmp.base);
    if ((e = hipMemsetAsync(dtot, 0, sizeof(unsigned long long), st)) != hipSuccess) return e;
    tri_refs_total_kernel<<<blocks, kMeshBlock, 0, st>>>(m->tri9, m->ok, m->nf, g, dtot);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = hipMemcpyAsync(&total, dtot, sizeof total, hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
    if ((e = hipStreamSynchronize(st)) != hipSuccess) return e;
    if (total <= (unsigned long long)kRefsPerTri * (unsigned long long)F) break;  // one cell: total = F
  }
  // counts → offsets → references
  int32_t *start = nullptr, *refs = nullptr;
  Carve own;
  own.add(&start, (size_t)g.ncells + 1);
  own.add(&refs, (size_t)total);
  if ((e = own.alloc(&m->gblock, &m->gblock_bytes, st)) != hipSuccess) return e;
  size_t scan_bytes = 0;
  int32_t* cnt = nullptr;
  char* scan_tmp = nullptr;
  e = hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, cnt, start, (int)(g.ncells + 1), st);
  if (e != hipSuccess) return e;
  Carve tmp;
  tmp.add(&cnt, (size_t)g.ncells + 1);
  tmp.add(&scan_tmp, std::max<size_t>(scan_bytes, 1));
  if ((e = ctx->tmp.reserve(tmp.bytes())) != hipSuccess) return e;
  tmp.place(ctx->tmp.base);
  if ((e = hipMemsetAsync(cnt, 0, sizeof(int32_t) * ((size_t)g.ncells + 1), st)) != hipSuccess) return e;
  tri_cells_kernel<false><<<blocks, kMeshBlock, 0, st>>>(m->tri9, m->ok, m->nf, g, cnt, nullptr, nullptr);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if ((e = hipcub::DeviceScan::ExclusiveSum(scan_tmp, scan_bytes, cnt, start, (int)(g.ncells + 1), st)) != hipSuccess)
    return e;
  tri_cells_kernel<true><<<blocks, kMeshBlock, 0, st>>>(m->tri9, m->ok, m->nf, g, cnt, start, refs);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if ((e = hipStreamSynchronize(st)) != hipSuccess) return e;
  g.start = start;
  g.refs = refs;
  m->grid = g;
  m->nrefs = (int64_t)total;
  m->doublings = doublings;
  m->grid_built = true;
  return hipSuccess;
}

namespace {
MeshXf xf_of(const double* T) {
  MeshXf x{};
  x.on = T != nullptr ? 1 : 0;
  for (int k = 0; k < 12; ++k) x.m[k] = T != nullptr ? T[k] : 0.0;
  return x;
}
}  // namespace

hipError_t mesh_closest_brute(const m3d_mesh* m, const double* xyz, int64_t n, const double* T, double* d2,
                              int32_t* tri, double* point, double* uv, uint8_t* region, hipStream_t st) {
  if (n == 0 || m->nf == 0) return hipSuccess;  // no query, or no triangle to stage: no launch
  const unsigned blocks = (unsigned)((n + kMeshBlock - 1) / kMeshBlock);
  mesh_brute_kernel<<<blocks, kMeshBlock, 0, st>>>(xyz, n, xf_of(T), m->tri9, m->ok, m->nf,
                                                   MeshOut{d2, tri, point, uv, region});
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  return e;
}

hipError_t mesh_closest_grid(m3d_ctx* ctx, m3d_mesh* m, const double* xyz, int64_t n, const double* T, double r0,
                             double* d2, int32_t* tri, double* point, double* uv, uint8_t* region, void* scratch,
                             hipStream_t st, std::string* why) {
  m->last_rounds = 0;
  if (n == 0 || m->usable == 0) return hipSuccess;
  hipError_t e = mesh_grid_build(ctx, m, st, why);
  if (e != hipSuccess) return e;
  const MeshScratch L(n, scratch);
  int32_t* pend[2] = {L.pend_a, L.pend_b};
  if ((e = hipMemsetAsync(L.cnt, 0, sizeof(uint32_t) * kMaxRounds, st)) != hipSuccess) return e;
  const TriGridDev& g = m->grid;
  float rf = r0 > 0.0 ? float_up(r0) : 1.0f / g.inv_h;  // automatic: one cell
  if (!(rf > 0.0f)) rf = FLT_MIN;
  if (!(rf <= FLT_MAX)) rf = FLT_MAX;
  const MeshXf xf = xf_of(T);
  const MeshOut out{d2, tri, point, uv, region};
  int64_t npend = n;
  int round = 0;
  for (; round < kMaxRounds && npend > 0; ++round) {
    const int32_t* in = round == 0 ? nullptr : pend[(round - 1) & 1];
    const unsigned blocks = (unsigned)((npend + 3) / 4);
    mesh_grid_kernel<<<blocks, kMeshBlock, 0, st>>>(xyz, xf, m->tri9, g, in, npend, rf, L.rq, pend[round & 1],
                                                    L.cnt + round, out);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    uint32_t left = 0;
    if ((e = hipMemcpyAsync(&left, L.cnt + round, sizeof left, hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
    if ((e = hipStreamSynchronize(st)) != hipSuccess) return e;
    npend = (int64_t)left;
  }
  m->last_rounds = round;
  if (npend > 0) {
    *why = "mesh ladder: round bound reached with queries pending";
    return hipErrorUnknown;
  }
  return hipSuccess;
}

}  // namespace m3d
