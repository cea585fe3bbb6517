// knn_wave.h — the wave-per-point neighbourhood scans: ONE WAVE walks the cell box of a query, lanes
// over the candidates of a cell row.  The walk (wave_box_chunks) and the two scans on top of it:
//   wave_scan_box      the fixed-radius scan: every point with d² < r² (cluster.hip link / label,
//                      iss.hip moments / non-max; clean.hip radius_count_kernel keeps the same
//                      scan written out, for its speed);
//   wave_knn_scan_box  the kk nearest of those in a wave-held sorted list (prep.hip
//                      hybrid_search_wave_kernel, clean.hip knn_level_kernel).
// This is the one place where the walk, the list and their exactness argument live.
//
// Contract of both scans: membership is d² < r² (strict, the query itself included), d² =
// (dx·dx + dy·dy) + dz·dz with d = p_t − q in fp64 on the cloud's original coordinates
// (-ffp-contract=off) — the oracles' test bit for bit.  The centred fp32 grid points only screen
// candidates (prefilter_bound) and size the cell box (box_half_width): a candidate the screen
// passes is decided by its exact d², one it drops is provably outside the current threshold (r²,
// or the list's kk-th entry).  The box is cut out of the grid with grid_coord (nnkey.h), the
// expression that placed the points, so the covering argument holds by construction.
// The list adds: the kk smallest (d², index) keys in ascending order, ties by index.
#pragma once

#include <float.h>

#include <cmath>

#include "linalg.h"
#include "m3d_internal.h"
#include "nnkey.h"

namespace m3d {

// ------------------------------------------------------------------------------- host side
// bound on |fp32 distance − fp64 distance| of two centred points (both coordinate roundings,
// √3·2·u·rmax, u = 2^-24)
inline double pair_eabs(const m3d_cloud* c) { return 3.4641016151377544 * c->rmax * 0x1p-24 * 1.01; }

// the fp32 box half-width that covers every point within `radius` (fp64) of a query: the radius
// plus the centring / rounding error of both fp32 coordinates.  Clamped to FLT_MAX: grid_coord
// clamps the cell range to the grid, so an infinite and a FLT_MAX half-width select the same cells.
inline float box_half_width(const m3d_cloud* c, double radius) {
  const double Rd = (radius + 2.0 * c->rmax * 0x1p-24 * 1.01) * (1.0 + 1e-6);
  const float f = (float)Rd * (1.0f + 1e-6f);
  return std::isfinite(f) ? f : FLT_MAX;
}

// ------------------------------------------------------------------------------- device helpers
__device__ __forceinline__ double d2_exact(const double* a, const double* b) {
  const double dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
  return (dx * dx + dy * dy) + dz * dz;
}

// the list's total order: (d², index)
__device__ __forceinline__ bool key_less(double d, int32_t t, double D, int32_t T) {
  return d < D || (d == D && t < T);
}

// fp32 prefilter of a candidate against an exact fp64 threshold thr (inclusive): with e the
// bound on |fp32 distance − fp64 distance| of two centred points (pair_eabs), any point whose
// fp64 d² ≤ thr has a directly computed fp32 d² (three roundings of relative u each, covered by
// the 4e-6 factors) ≤ this bound — so a candidate above it can be skipped without its fp64 gather.
// Host and device give the same float (the conversion rounds up on both): the fixed-radius scans
// take their one bound from the host (radius_screen), the list kernels follow their threshold on
// the device.
__host__ __device__ __forceinline__ float prefilter_bound(double thr, double e) {
  const double b = (sqrt(thr) + e) * (1.0 + 4e-6);
  const double b2 = b * b * (1.0 + 4e-6);
#if defined(__HIP_DEVICE_COMPILE__)
  const float f = __double2float_ru(b2);
#else
  float f = (float)b2;  // to nearest, then up if that fell below
  if ((double)f < b2) f = std::nextafter(f, INFINITY);
#endif
  return std::isfinite(f) ? f : FLT_MAX;
}

// what a fixed-radius scan (wave_scan_box) of cloud c takes: the box half-width, the exact r² and
// the fp32 screen bound of r², formed once on the host (the threshold never moves)
struct RadiusScreen {
  float Rf;
  double r2;
  float bf;
};
inline RadiusScreen radius_screen(const m3d_cloud* c, double radius) {
  const double r2 = radius * radius;
  return {box_half_width(c, radius), r2, prefilter_bound(r2, pair_eabs(c))};
}

// lane l ← lane l − 1 across the whole wave (gfx9 DPP wave_shr:1; lane 0 keeps `old`): a VALU
// move, no LDS round trip like ds_bpermute
__device__ __forceinline__ int32_t wave_shr1(int32_t old, int32_t v) {
  return __builtin_amdgcn_update_dpp(old, v, 0x138, 0xF, 0xF, false);
}
__device__ __forceinline__ double wave_shr1(double old, double v) {
  const uint64_t o = (uint64_t)__double_as_longlong(old), x = (uint64_t)__double_as_longlong(v);
  const uint32_t lo = (uint32_t)wave_shr1((int32_t)(uint32_t)o, (int32_t)(uint32_t)x);
  const uint32_t hi = (uint32_t)wave_shr1((int32_t)(uint32_t)(o >> 32), (int32_t)(uint32_t)(x >> 32));
  return __longlong_as_double((long long)(((uint64_t)hi << 32) | lo));
}
// (readlane_f64: linalg.h)

// LDS written by some lanes of a wave is read by others of the same wave
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ------------------------------------------------------------------------------- the list
// Up to kk ≤ 64·kS entries sorted by (d², index) across the lanes of ONE wave: entry e in lane
// e % 64, slot e / 64.  D and T are only ever indexed by compile-time constants (unrolled loops,
// the `v == u` select), so they stay in registers.  cnt, thr and thr_t are wave-uniform.
template <int kS>
struct WaveKnnList {
  double D[kS];
  int32_t T[kS];
  int cnt;        // entries held
  double thr;     // exact threshold: r² until kk are held, then the kk-th entry (inclusive)
  int32_t thr_t;
  float bf;       // prefilter_bound of thr as of the last chunk: the fp32 screen of the next one

  __device__ __forceinline__ void reset(double r2, double eabs) {
#pragma unroll
    for (int u = 0; u < kS; ++u) {
      D[u] = 0.0;
      T[u] = -1;
    }
    cnt = 0;
    thr = r2;
    thr_t = INT32_MAX;
    bf = prefilter_bound(r2, eabs);
  }

  // whether a point strictly inside the radius would enter the list (cnt never exceeds kk)
  __device__ __forceinline__ bool accepts(double d, int32_t t, int kk) const {
    return cnt != kk || key_less(d, t, thr, thr_t);
  }

  // One (wave-uniform) entry into the list: its place = the held entries below it (a ballot), the
  // entries from there on move up one lane, the kk-th entry sets the next threshold.
  __device__ __forceinline__ void insert(double x, int32_t xt, int kk) {
    const int lane = threadIdx.x & 63;
    int pos = 0;
#pragma unroll
    for (int u = 0; u < kS; ++u) {
      const int e = u * 64 + lane;
      pos += __popcll(__ballot(e < cnt && key_less(D[u], T[u], x, xt)));
    }
#pragma unroll
    for (int u = kS - 1; u >= 0; --u) {
      // lane 0 of slot u takes lane 63 of slot u − 1 (a uniform read), the others their left
      // neighbour
      const double d63 = u > 0 ? readlane_f64(D[u > 0 ? u - 1 : 0], 63) : 0.0;
      const int32_t t63 = u > 0 ? __builtin_amdgcn_readlane(T[u > 0 ? u - 1 : 0], 63) : -1;
      const double dc = wave_shr1(d63, D[u]);
      const int32_t tc = wave_shr1(t63, T[u]);
      const int e = u * 64 + lane;
      if (e > pos) {
        D[u] = dc;
        T[u] = tc;
      } else if (e == pos) {
        D[u] = x;
        T[u] = xt;
      }
    }
    cnt = cnt < kk ? cnt + 1 : kk;
    if (cnt == kk) {
      const int u = (kk - 1) / 64, l = (kk - 1) % 64;
      double dk = D[0];
      int32_t tk = T[0];
#pragma unroll
      for (int v = 0; v < kS; ++v)
        if (v == u) {
          dk = D[v];
          tk = T[v];
        }
      thr = readlane_f64(dk, l);
      thr_t = __builtin_amdgcn_readlane(tk, l);
    }
  }

  // kS == 1: the candidates of a chunk (mask = the ballot of cand; lane l holds candidate (d, t))
  // merged in one step instead of one insertion each.  Every element's place in the union of the
  // held list and the candidates is its rank (the keys (d², index) are distinct): a list entry is
  // preceded by its own index and the candidates below it, a candidate by the list entries below
  // it (binary search over the sorted list) and the candidates below it.  Elements ranked below
  // kk are written to the wave's LDS row at their rank and read back.
  __device__ __forceinline__ void merge_chunk(uint64_t mask, bool cand, double d, int32_t t, int kk,
                                              double* lds_d_row, int32_t* lds_t_row) {
    static_assert(kS == 1, "merge_chunk: one slot per lane");
    const int lane = threadIdx.x & 63;
    int rl = lane, rc = 0;
    for (uint64_t mm = mask; mm != 0; mm &= mm - 1) {
      const int s = __builtin_ctzll(mm);
      const double x = readlane_f64(d, s);
      const int32_t xt = __builtin_amdgcn_readlane(t, s);
      rl += key_less(x, xt, D[0], T[0]) ? 1 : 0;
      rc += key_less(x, xt, d, t) ? 1 : 0;
    }
    int lo = 0, hi = cnt;  // list entries below this lane's candidate: the first index whose
    for (int it = 0; it < 7; ++it) {  // key is not below it
      const int mid = (lo + hi) >> 1;
      const int src = mid < 64 ? mid : 63;
      const double dm = __shfl(D[0], src);
      const int32_t tm = __shfl(T[0], src);
      if (lo < hi) {
        if (key_less(dm, tm, d, t))
          lo = mid + 1;
        else
          hi = mid;
      }
    }
    rc += lo;
    const int c = __popcll(mask);
    const int ncnt = cnt + c < kk ? cnt + c : kk;
    if (lane < cnt && rl < kk) {
      lds_d_row[rl] = D[0];
      lds_t_row[rl] = T[0];
    }
    if (cand && rc < kk) {
      lds_d_row[rc] = d;
      lds_t_row[rc] = t;
    }
    wave_lds_sync();
    if (lane < ncnt) {
      D[0] = lds_d_row[lane];
      T[0] = lds_t_row[lane];
    }
    wave_lds_sync();
    cnt = ncnt;
    if (cnt == kk) {
      thr = readlane_f64(D[0], kk - 1);
      thr_t = __builtin_amdgcn_readlane(T[0], kk - 1);
    }
  }
};

// ------------------------------------------------------------------------------- the walk
// The cell box of half-width Rf around the fp32 query qf, walked by one wave: of every cell row
// [j0, j1) of the sorted grid (the rows are contiguous, so a chunk is read coalesced) the
// 64-candidate chunks starting at jb = j0 + chunk0, + stride, … (point offsets; 0 and 64: all of
// them): body(jb, j1).  body returns true (wave-uniform) to leave the box.  Every loop is bounded
// by the grid's dimensions or a cell row's length.
template <class Body>
__device__ __forceinline__ void wave_box_chunks(const float4 qf, const GridDev& g, float Rf, int chunk0,
                                                int stride, Body&& body) {
  const int x0 = grid_coord(qf.x - Rf, g.o[0], g.inv_h, g.n[0]);
  const int x1 = grid_coord(qf.x + Rf, g.o[0], g.inv_h, g.n[0]);
  const int y0 = grid_coord(qf.y - Rf, g.o[1], g.inv_h, g.n[1]);
  const int y1 = grid_coord(qf.y + Rf, g.o[1], g.inv_h, g.n[1]);
  const int z0 = grid_coord(qf.z - Rf, g.o[2], g.inv_h, g.n[2]);
  const int z1 = grid_coord(qf.z + Rf, g.o[2], g.inv_h, g.n[2]);
  bool stop = false;  // wave-uniform
  for (int cz = z0; cz <= z1 && !stop; ++cz)
    for (int cy = y0; cy <= y1 && !stop; ++cy) {
      const int64_t row = ((int64_t)cz * g.n[1] + cy) * g.n[0];
      const int32_t j0 = g.start[row + x0], j1 = g.start[row + x1 + 1];
      for (int32_t jb = j0 + chunk0; jb < j1 && !stop; jb += stride) stop = body(jb, j1);
    }
}

// The fixed-radius scan: for every chunk of the box, pre(t) in the lanes whose candidate t passes
// the fp32 screen bf — BEFORE the exact test reads the candidate's coordinates, so what pre loads is
// in flight beside them — then, in every lane, f(in, t, dx, dy, dz) with d = p_t − q and `in` the
// exact test d² < r² (false in a lane without a candidate or behind the screen).  f returns true
// (wave-uniform) to leave the box.
template <class Pre, class F>
__device__ __forceinline__ void wave_scan_box(const double* __restrict__ xyz64, const double* q, const float4 qf,
                                              const GridDev& g, float Rf, double r2, float bf, int lane,
                                              Pre&& pre, F&& f) {
  wave_box_chunks(qf, g, Rf, 0, 64, [&](int32_t jb, int32_t j1) {
    const int32_t j = jb + lane;
    bool in = false;
    int32_t t = 0;
    double dx = 0.0, dy = 0.0, dz = 0.0;
    if (j < j1) {
      const float4 tp = g.pts[j];
      t = __float_as_int(tp.w);
      const float fx = qf.x - tp.x, fy = qf.y - tp.y, fz = qf.z - tp.z;
      if ((fx * fx + fy * fy) + fz * fz <= bf) {
        pre(t);
        const double* p = xyz64 + 3 * (int64_t)t;
        dx = p[0] - q[0], dy = p[1] - q[1], dz = p[2] - q[2];
        in = (dx * dx + dy * dy) + dz * dz < r2;  // d2_exact's expression
      }
    }
    return f(in, t, dx, dy, dz);
  });
}

// The box scanned into the list: the candidates of a chunk are screened in fp32 against
// prefilter_bound of the current threshold, the survivors' exact fp64 d² evaluated and the
// qualifying ones merged (kS == 1, three or more) or inserted one by one.  The fp32 screen bound
// follows the kk-th entry once per chunk: the entries of a chunk are tested against the exact
// thr, bf only screens the next chunk.  lds_*_row: 64 entries owned by this wave (kS == 1 only).
// The inner loops are bounded by the 64 bits of a ballot.
template <int kS>
__device__ __forceinline__ void wave_knn_scan_box(WaveKnnList<kS>& L, const double* __restrict__ xyz64,
                                                  const double* q, const float4 qf, const GridDev& g, float Rf,
                                                  double r2, double eabs, int kk, int chunk0, int stride,
                                                  double* lds_d_row, int32_t* lds_t_row) {
  const int lane = threadIdx.x & 63;
  wave_box_chunks(qf, g, Rf, chunk0, stride, [&](int32_t jb, int32_t j1) {
    const int32_t j = jb + lane;
    bool cand = false;
    double d = 0.0;
    int32_t t = -1;
    if (j < j1) {
      const float4 tp = g.pts[j];
      const float fx = qf.x - tp.x, fy = qf.y - tp.y, fz = qf.z - tp.z;
      if ((fx * fx + fy * fy) + fz * fz <= L.bf) {
        t = __float_as_int(tp.w);
        d = d2_exact(xyz64 + 3 * (int64_t)t, q);
        cand = d < r2 && L.accepts(d, t, kk);
      }
    }
    uint64_t m = __ballot(cand);
    if constexpr (kS == 1) {
      if (__popcll(m) >= 3) {
        L.merge_chunk(m, cand, d, t, kk, lds_d_row, lds_t_row);
        m = 0;
      }
    }
    while (m != 0) {
      const int src = __builtin_ctzll(m);
      m &= m - 1;
      const double x = readlane_f64(d, src);
      const int32_t xt = __builtin_amdgcn_readlane(t, src);
      if (!L.accepts(x, xt, kk)) continue;  // the threshold moved
      L.insert(x, xt, kk);
    }
    if (L.cnt == kk) L.bf = prefilter_bound(L.thr, eabs);
    return false;  // the whole box, always
  });
}

}  // namespace m3d
