// cluster.hip — DBSCAN on the device: Open3D 0.19 PointCloud::ClusterDBSCAN's labels in closed form.
//
// nbs[i] = {j : d²(i, j) < eps²} (strict, the point itself included): the fixed-radius scan of
// knn_wave.h (wave_scan_box; its contract and exactness argument are stated there).
// core[i] = |nbs[i]| ≥ min_points.  Open3D's sequential loop gives, whatever order its
// unordered_set pops in:
//   core point      → the rank of its connected component in the graph on core points with an edge
//                     for every core pair with d² < eps², components ranked by smallest member index;
//   border point    → (not core, at least one core neighbour) the smallest label among its core
//                     neighbours;
//   any other point → −1.
//
// Three box scans on the cloud's grid of cell eps, each ONE WAVE per point in the grid's cell order,
// lanes over the candidates of a cell row:
//   1. core flags   clean.hip radius_flags (radius_count_kernel, nb_points = min_points − 1)
//   2. link         every core point i unites itself with every core neighbour j < i (each edge
//                   once) in a lock-free union–find over parent[n]; then flatten, its own launch.
//                   A wave remembers a root its point's tree has had, so a neighbour already in
//                   that tree costs one load of parent[] (link_kernel)
//   3. label        roots flagged, an inclusive scan in index order numbers them; a core point takes
//                   its root's number, a non-core point scans its box for the smallest root among its
//                   core neighbours (the numbering is monotone in the root index, so the smallest
//                   root is the smallest label)
// then the cluster sizes (integer atomics, one per distinct label of a wave), the core / noise
// counts and the largest cluster (a 64-bit integer max over (size, ~label)).  Integer atomics only:
// the partition and the labels are unique, so two calls return the same bits.
//
// The union–find (link_kernel) is the only place where workgroups communicate inside a launch.
//   * parent[i] = i at the start.  A root r is hooked only by compare-and-swap(parent[r]: r → s)
//     with s < r; a non-root x is only ever lowered (atomicMin, path halving) to a value read from
//     parent[] of one of its ancestors.  So parent[x] ≤ x always, parent[x] < x for every non-root,
//     a non-root never becomes a root again and every stored value only decreases.
//   * Hence every walk x → parent[x] → … strictly decreases and ends at a root within n steps,
//     whatever stale or fresh values it reads: every value ever stored in parent[x] is a node of
//     x's tree at the time of the store, and trees only merge.
//   * unite(a, b) finds both roots, and hooks the LARGER under the smaller.  The CAS succeeds only
//     if the larger is still a root; if not, somebody hooked it meanwhile and the retry starts from
//     it — its new root is smaller, so the larger root of consecutive tries strictly decreases: at
//     most n tries.  A root is its tree's smallest index (induction over hooks: the hooked tree's
//     smallest is its root r, the other tree holds s < r), so a component's final root is its
//     smallest core index — Open3D's ranking key.
//   * Every access to parent[] in link_kernel is an agent-scope relaxed atomic: the XCDs' L2s are
//     private and a plain load may return a stale line.  Correctness does not need a fresh value —
//     a stale parent is an older ancestor, it costs another step or another trip round the CAS
//     loop — and no wave ever waits for another's progress: there is nothing to hang on.
//   * The loops are capped all the same (n + 64 steps).  A cap that is hit sets a fault word and
//     the call fails: a bug ends the call instead of occupying the device.
// Flatten and label run in later launches and read parent[] with plain loads.
#include <float.h>

#include <algorithm>
#include <cmath>
#include <string>

#include <hipcub/hipcub.hpp>

#include "m3d_internal.h"
#include "knn_wave.h"

namespace m3d {
namespace {

constexpr int kClBlock = 256;
constexpr int kClWaves = kClBlock / kWave;

// stats words (device, int32 unless noted)
constexpr int kStCore = 0, kStNoise = 1, kStFault = 2, kStBest = 4;  // [4..5]: uint64 (size, ~label)
constexpr int kStWords = 8;

#define M3D_RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

__device__ __forceinline__ int32_t uf_load(int32_t* parent, int32_t x) {
  return __hip_atomic_load(parent + x, M3D_RLX_AGENT);
}

// the root of x's tree as far as this lane can see it, halving the path on the way; −1: cap hit
__device__ __forceinline__ int32_t uf_find(int32_t* parent, int32_t x, int32_t cap) {
  for (int32_t step = 0; step < cap; ++step) {
    const int32_t p = uf_load(parent, x);
    if (p == x) return x;
    const int32_t gp = uf_load(parent, p);
    if (gp == p) return p;
    atomicMin(parent + x, gp);  // x is no root: lowering it to an ancestor's parent (gp < p < x)
    x = gp;
  }
  return -1;
}

// false: cap hit
__device__ __forceinline__ bool uf_unite(int32_t* parent, int32_t a, int32_t b, int32_t cap) {
  for (int32_t tries = 0; tries < cap; ++tries) {
    const int32_t ra = uf_find(parent, a, cap), rb = uf_find(parent, b, cap);
    if (ra < 0 || rb < 0) return false;
    if (ra == rb) return true;
    const int32_t hi = ra > rb ? ra : rb, lo = ra > rb ? rb : ra;
    int32_t expect = hi;
    if (__hip_atomic_compare_exchange_strong(parent + hi, &expect, lo, __ATOMIC_RELAXED, M3D_RLX_AGENT)) return true;
    a = hi;  // hooked meanwhile: its new root is smaller
    b = lo;
  }
  return false;
}

// parent[i] = i, sizes[i] = 0, the stats words zero
__global__ __launch_bounds__(kClBlock) void init_kernel(int64_t n, int32_t* __restrict__ parent,
                                                        int32_t* __restrict__ sizes, int32_t* __restrict__ stats) {
  const int64_t i = (int64_t)blockIdx.x * kClBlock + threadIdx.x;
  if (i < kStWords) stats[i] = 0;
  if (i >= n) return;
  parent[i] = (int32_t)i;
  sizes[i] = 0;
}

// pass 2: every core point unites itself with its core neighbours of smaller index.  parent is
// deliberately not __restrict__ / const: it is read and written through atomics only.
__global__ __launch_bounds__(kClBlock) void link_kernel(const double* __restrict__ xyz64,
                                                        const float4* __restrict__ xyz32, int64_t n, GridDev g,
                                                        float Rf, double r2, float bf,
                                                        const uint8_t* __restrict__ core, int32_t* parent,
                                                        int32_t* stats) {
  const int lane = threadIdx.x & 63;
  const int64_t wq = (int64_t)blockIdx.x * kClWaves + (threadIdx.x >> 6);
  if (wq >= n) return;  // wave-uniform
  const int32_t i = __float_as_int(g.pts[wq].w);
  if (!core[i]) return;  // wave-uniform
  const double q[3] = {xyz64[3 * (int64_t)i], xyz64[3 * (int64_t)i + 1], xyz64[3 * (int64_t)i + 2]};
  const int32_t cap = n + 64 < INT32_MAX ? (int32_t)(n + 64) : INT32_MAX;
  bool ok = true;
  // ri (wave-uniform): a root i's tree has had.  A neighbour whose parent or root is ri is in i's
  // tree for good (trees only merge), whenever either was read: once the paths are short nearly
  // every lane leaves here on the one load that travelled beside its coordinates.  The others
  // unite; then i's root is read again.
  int32_t ri = i, p = 0;
  bool c = false;
  wave_scan_box(
      xyz64, q, xyz32[i], g, Rf, r2, bf, lane,
      [&](int32_t t) {
        c = t < i && core[t] != 0;
        p = uf_load(parent, t);
      },
      [&](bool in, int32_t t, double, double, double) {
        const bool edge = in && c;  // in: this chunk's pre ran in this lane
        int32_t rt = ri;
        if (edge && p != ri) rt = p == t ? t : uf_find(parent, t, cap);
        if (rt < 0) ok = false, rt = ri;
        if (__ballot(rt != ri) == 0) return false;  // wave-uniform
        if (rt != ri) ok = uf_unite(parent, ri, rt, cap) && ok;
        ri = __builtin_amdgcn_readfirstlane(uf_find(parent, i, cap));
        if (ri < 0) ok = false, ri = i;
        return false;  // the whole box
      });
  if (!ok) atomicOr(stats + kStFault, 1);
}

// parent[i] = its root (plain loads: a later launch than every hook); root[i] = 1 for a core root.
// A thread may read a parent another thread of this launch has already flattened: an ancestor either way.
__global__ __launch_bounds__(kClBlock) void flatten_kernel(int64_t n, const uint8_t* __restrict__ core,
                                                           int32_t* parent, int32_t* __restrict__ root,
                                                           int32_t* stats) {
  const int64_t i = (int64_t)blockIdx.x * kClBlock + threadIdx.x;
  if (i >= n) return;
  int32_t x = (int32_t)i;
  const int64_t cap = n + 64;
  int64_t step = 0;
  for (; step < cap; ++step) {
    const int32_t p = parent[x];
    if (p == x) break;
    x = p;
  }
  if (step == cap) atomicOr(stats + kStFault, 2);
  if (x != (int32_t)i) parent[i] = x;
  root[i] = (core[i] && x == (int32_t)i) ? 1 : 0;
}

// pass 3: the labels.  rank: the inclusive scan of root[] (rank[r] − 1 = the number of root r).
__global__ __launch_bounds__(kClBlock) void label_kernel(const double* __restrict__ xyz64,
                                                         const float4* __restrict__ xyz32, int64_t n, GridDev g,
                                                         float Rf, double r2, float bf,
                                                         const uint8_t* __restrict__ core,
                                                         const int32_t* __restrict__ parent,
                                                         const int32_t* __restrict__ rank,
                                                         int32_t* __restrict__ labels) {
  const int lane = threadIdx.x & 63;
  const int64_t wq = (int64_t)blockIdx.x * kClWaves + (threadIdx.x >> 6);
  if (wq >= n) return;  // wave-uniform
  const int32_t i = __float_as_int(g.pts[wq].w);
  if (core[i]) {
    if (lane == 0) labels[i] = rank[parent[i]] - 1;
    return;
  }
  const double q[3] = {xyz64[3 * (int64_t)i], xyz64[3 * (int64_t)i + 1], xyz64[3 * (int64_t)i + 2]};
  int32_t best = INT32_MAX, p = 0;
  bool c = false;
  wave_scan_box(
      xyz64, q, xyz32[i], g, Rf, r2, bf, lane,
      [&](int32_t t) {
        c = core[t] != 0;
        p = parent[t];
      },
      [&](bool in, int32_t, double, double, double) {
        if (in && c) best = min(best, p);
        return false;  // the whole box
      });
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) best = min(best, __shfl_xor(best, o));
  if (lane == 0) labels[i] = best == INT32_MAX ? -1 : rank[best] - 1;
}

// sizes[label] (one atomic per distinct label of a wave's 64 consecutive points), the core and
// noise counts (one atomic per wave)
__global__ __launch_bounds__(kClBlock) void tally_kernel(int64_t n, const uint8_t* __restrict__ core,
                                                         const int32_t* __restrict__ labels,
                                                         int32_t* __restrict__ sizes, int32_t* __restrict__ stats) {
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * kClBlock + threadIdx.x;
  const bool live = i < n;
  const int32_t lab = live ? labels[i] : -1;
  const int32_t ncore = (int32_t)__popcll(__ballot(live && core[i]));
  const int32_t nnoise = (int32_t)__popcll(__ballot(live && lab < 0));
  if (lane == 0) {
    if (ncore) atomicAdd(stats + kStCore, ncore);
    if (nnoise) atomicAdd(stats + kStNoise, nnoise);
  }
  bool todo = lab >= 0;
  while (__ballot(todo) != 0) {  // at most 64 rounds: each retires a label's lanes
    const unsigned long long act = __ballot(todo);
    const int lead = __ffsll((long long)act) - 1;
    const int32_t L = __shfl(lab, lead);
    const bool mine = todo && lab == L;
    const int32_t c = (int32_t)__popcll(__ballot(mine));
    if (lane == lead) atomicAdd(sizes + L, c);
    if (mine) todo = false;
  }
}

// the biggest cluster, the lowest label on ties: max over (size << 32 | ~label)
__global__ __launch_bounds__(kClBlock) void largest_kernel(int64_t n, const int32_t* __restrict__ rank,
                                                           const int32_t* __restrict__ sizes,
                                                           unsigned long long* __restrict__ best) {
  const int32_t nc = rank[n - 1];
  unsigned long long b = 0;
  for (int64_t l = (int64_t)blockIdx.x * kClBlock + threadIdx.x; l < nc; l += (int64_t)gridDim.x * kClBlock)
    b = max(b, ((unsigned long long)(uint32_t)sizes[l] << 32) | (uint32_t)~(uint32_t)l);
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) {
    const unsigned long long v = ((unsigned long long)(uint32_t)__shfl_xor((int)(b >> 32), o) << 32) |
                                 (uint32_t)__shfl_xor((int)(uint32_t)b, o);
    b = max(b, v);
  }
  if ((threadIdx.x & 63) == 0 && b != 0) atomicMax(best, b);
}

// the pieces of a call's scratch for n points, placed onto `scratch` (null: the layout's size alone)
struct ClusterScratch {
  uint8_t* core = nullptr;
  int32_t *parent = nullptr, *root = nullptr, *rank = nullptr, *sizes = nullptr, *stats = nullptr;
  char* tmp = nullptr;
  size_t tmp_bytes = 0, bytes = 0;
  ClusterScratch(int64_t n, void* scratch) {
    size_t tb = 0;
    hipcub::DeviceScan::InclusiveSum(nullptr, tb, (int32_t*)nullptr, (int32_t*)nullptr, (int)n, (hipStream_t)0);
    tmp_bytes = std::max<size_t>(tb, 1);
    Carve cv;
    cv.add(&core, (size_t)n);
    cv.add(&parent, (size_t)n);
    cv.add(&root, (size_t)n);
    cv.add(&rank, (size_t)n);
    cv.add(&sizes, (size_t)n);
    cv.add(&stats, kStWords);
    cv.add(&tmp, tmp_bytes);
    bytes = cv.bytes();
    if (scratch != nullptr) cv.place(scratch);
  }
};

}  // namespace

size_t cluster_scratch_bytes(int64_t n) { return n > 0 ? ClusterScratch(n, nullptr).bytes : 0; }

// Profiling (m3d_profile_*): core flags under M3D_KERNEL_SCORE, link under M3D_KERNEL_NN, flatten
// and the root scan under M3D_KERNEL_LOOP, label under M3D_KERNEL_TERMS, sizes / counts / largest
// under M3D_KERNEL_KABSCH.
hipError_t cluster_dbscan(m3d_ctx* ctx, const m3d_cloud* c, const Grid* g, double eps, int32_t min_points,
                          int32_t* labels_out, m3d_dbscan_result* out, int32_t* sizes_out, int32_t* count_out,
                          void* scratch, hipStream_t st, std::string* why) {
  const int64_t n = c->n;
  const ClusterScratch L(n, scratch);
  uint8_t* core = L.core;
  int32_t *parent = L.parent, *root = L.root, *rank = L.rank, *stats = L.stats;
  int32_t* sizes = sizes_out != nullptr ? sizes_out : L.sizes;
  const RadiusScreen s = radius_screen(c, eps);
  const unsigned per_thread = (unsigned)((n + kClBlock - 1) / kClBlock);
  const unsigned per_wave = (unsigned)((n + kClWaves - 1) / kClWaves);
  hipError_t e = hipSuccess;
  {
    KTimer t(ctx, M3D_KERNEL_SCORE, st);
    init_kernel<<<per_thread, kClBlock, 0, st>>>(n, parent, sizes, stats);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = radius_flags(c, g, min_points - 1, eps, count_out, core, st)) != hipSuccess) return e;
  }
  {
    KTimer t(ctx, M3D_KERNEL_NN, st);
    link_kernel<<<per_wave, kClBlock, 0, st>>>(c->xyz64, c->xyz32, n, g->dev, s.Rf, s.r2, s.bf, core, parent, stats);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  {
    KTimer t(ctx, M3D_KERNEL_LOOP, st);
    flatten_kernel<<<per_thread, kClBlock, 0, st>>>(n, core, parent, root, stats);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    size_t tb = L.tmp_bytes;
    if ((e = hipcub::DeviceScan::InclusiveSum(L.tmp, tb, root, rank, (int)n, st)) != hipSuccess) return e;
  }
  {
    KTimer t(ctx, M3D_KERNEL_TERMS, st);
    label_kernel<<<per_wave, kClBlock, 0, st>>>(c->xyz64, c->xyz32, n, g->dev, s.Rf, s.r2, s.bf, core, parent,
                                                rank, labels_out);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  {
    KTimer t(ctx, M3D_KERNEL_KABSCH, st);
    tally_kernel<<<per_thread, kClBlock, 0, st>>>(n, core, labels_out, sizes, stats);
    largest_kernel<<<std::min(per_thread, 256u), kClBlock, 0, st>>>(
        n, rank, sizes, reinterpret_cast<unsigned long long*>(stats + kStBest));
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  int32_t h[kStWords] = {0};
  int32_t nc = 0;
  if ((e = hipMemcpyAsync(h, stats, sizeof h, hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
  if ((e = hipMemcpyAsync(&nc, rank + (n - 1), sizeof nc, hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
  if ((e = hipStreamSynchronize(st)) != hipSuccess) return e;
  if (h[kStFault] != 0) {
    *why = "union-find step bound reached (fault word " + std::to_string(h[kStFault]) + ")";
    return hipErrorUnknown;
  }
  out->num_clusters = nc;
  out->num_core = h[kStCore];
  out->num_noise = h[kStNoise];
  const uint32_t best_size = (uint32_t)h[kStBest + 1], best_inv = (uint32_t)h[kStBest];
  out->largest_label = nc > 0 ? (int64_t)(uint32_t)~best_inv : -1;
  out->largest_size = nc > 0 ? (int64_t)best_size : 0;
  return hipSuccess;
}

}  // namespace m3d
