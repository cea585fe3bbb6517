// thin.hip — thinning a cloud to a minimum point distance on the device: the points KEPT are
// original points of the cloud (a voxel mean moves points off the surface they were measured on),
// no two of them closer than `radius`, and every dropped point has a kept one strictly inside it.
//
// CONTRACT (restated in numpy by tests/mesh_sample_restatement.py).  Given a cloud, a finite
// radius > 0 and a seed: key_i = sample_base(seed, i) (sampler.h); the points are ranked by
// (key_i, i).  kept_i holds iff there is no j with (key_j, j) < (key_i, i), kept_j and
// d²(i, j) < radius², where d² is d2_exact on the original fp64 coordinates and the test is strict —
// wave_scan_box's membership test (knn_wave.h).  This is dart throwing in the hashed order: going
// through the points by rank, a point is kept unless a kept point lies strictly inside its radius.
// The definition is a recursion over a total order, so the result is unique.  A point with a
// coordinate that is not finite is never kept and blocks nobody (its d² to anything is not below
// radius²).
//
// Why a hashed rank: the rounds below decide a point once every lower-ranked neighbour is decided,
// so the round count is the longest chain of neighbours with ascending rank.  With the index as
// rank, a cloud stored in scan order (20,000 points of a unit square sorted by x, radius 0.02) needs
// 180 rounds; with the hashed key it needs 9, and 3,000 to 20,000 uniform points in a cube need 7
// or 8 either way (CPU simulation of the round structure).
//
// DEVICE FORM.  decided[n] int32: 0 undecided, +k kept in round k, −k dropped in round k.  A host
// loop of launches over a compacted queue of undecided points (modelled on mesh.hip's ladder: an
// integer atomic append, one count read per round).  Round R, ONE WAVE per queued point i: it scans
// the point's box on the cloud's cached grid of cell `radius` (radius_screen + wave_scan_box, as
// cluster.hip does), and for every neighbour j inside the radius with (key_j, j) < (key_i, i) reads
// decided[j].  An entry that is 0 OR HAS MAGNITUDE R counts as undecided: an entry written in this
// launch reads the same as the 0 it replaced, so a store racing with a load cannot change what is
// read, and the decisions of round R are a function of the state after round R − 1 alone — the round
// count is deterministic as well.
//   a lower-ranked KEPT neighbour                → decided[i] = −R (the wave leaves the box at once);
//   else a lower-ranked UNDECIDED neighbour      → i stays queued;
//   else                                         → decided[i] = +R.
// Termination: the lowest-ranked undecided point has no undecided lower-ranked neighbour, so every
// round decides at least one point; the host caps the loop at kThinMaxRounds and fails with a
// message.  No device-side waiting, no floating-point atomics; a wave writes only its own point's
// entry (and its queue slot, whose position changes nothing).
#include <float.h>

#include <algorithm>
#include <cmath>
#include <string>

#include "m3d_internal.h"
#include "knn_wave.h"
#include "sampler.h"

namespace m3d {
namespace {

constexpr int kThinBlock = 256;
constexpr int kThinWaves = kThinBlock / kWave;
constexpr int kThinMaxRounds = 256;

// per round two words: [2R] points left queued, [2R + 1] points kept
struct ThinScratch {
  int32_t *q_a = nullptr, *q_b = nullptr;
  uint32_t* cnt = nullptr;
  size_t bytes = 0;
  ThinScratch(int64_t n, void* scratch) {
    Carve cv;
    cv.add(&q_a, (size_t)n);
    cv.add(&q_b, (size_t)n);
    cv.add(&cnt, 2 * (kThinMaxRounds + 1));
    bytes = cv.bytes();
    if (scratch != nullptr) cv.place(scratch);
  }
};

// (key_a, a) < (key_b, b)
__device__ __forceinline__ bool rank_less(uint64_t ka, int32_t a, uint64_t kb, int32_t b) {
  return ka < kb || (ka == kb && a < b);
}

// One round.  q_in null: round 1, wave w takes the w-th point in the grid's cell order; otherwise
// point q_in[w].  decided is deliberately not __restrict__ / const: other waves of this launch
// store to it (see the header for why that cannot change what is read).
__global__ __launch_bounds__(kThinBlock) void thin_round_kernel(const double* __restrict__ xyz64,
                                                                const float4* __restrict__ xyz32, GridDev g,
                                                                float Rf, double r2, float bf, uint64_t seed,
                                                                int32_t R, const int32_t* __restrict__ q_in,
                                                                int64_t nq, int32_t* decided,
                                                                int32_t* __restrict__ q_out,
                                                                uint32_t* __restrict__ cnt) {
  const int lane = threadIdx.x & 63;
  const int64_t wq = (int64_t)blockIdx.x * kThinWaves + (threadIdx.x >> 6);
  if (wq >= nq) return;  // wave-uniform
  const int32_t i = q_in != nullptr ? q_in[wq] : __float_as_int(g.pts[wq].w);
  const double q[3] = {xyz64[3 * (int64_t)i], xyz64[3 * (int64_t)i + 1], xyz64[3 * (int64_t)i + 2]};
  if (!(isfinite(q[0]) && isfinite(q[1]) && isfinite(q[2]))) {  // wave-uniform
    if (lane == 0) decided[i] = -R;
    return;
  }
  const uint64_t ki = sample_base(seed, (int64_t)i);
  bool blocked = false, drop = false;
  int32_t st = 0;
  wave_scan_box(
      xyz64, q, xyz32[i], g, Rf, r2, bf, lane,
      [&](int32_t t) { st = __hip_atomic_load(decided + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); },
      [&](bool in, int32_t t, double, double, double) {
        // in: this chunk's pre ran in this lane, st is decided[t]
        const bool lower = in && rank_less(sample_base(seed, (int64_t)t), t, ki, i);
        const bool und = st == 0 || st == R || st == -R;
        if (__ballot(lower && !und && st > 0) != 0) {
          drop = true;
          return true;  // wave-uniform: leave the box
        }
        blocked = blocked || (lower && und);
        return false;
      });
  const bool wait = __ballot(blocked) != 0;
  if (lane != 0) return;
  if (drop) {
    decided[i] = -R;
  } else if (wait) {
    q_out[atomicAdd(cnt + 2 * R, 1u)] = i;
  } else {
    decided[i] = R;
    atomicAdd(cnt + 2 * R + 1, 1u);
  }
}

}  // namespace

size_t thin_scratch_bytes(int64_t n) { return n > 0 ? ThinScratch(n, nullptr).bytes : 0; }

hipError_t thin_min_distance(const m3d_cloud* c, const Grid* g, double radius, uint64_t seed, int32_t* decided,
                             int64_t* kept_out, int32_t* rounds_out, void* scratch, hipStream_t st,
                             std::string* why) {
  const int64_t n = c->n;
  const ThinScratch L(n, scratch);
  int32_t* queue[2] = {L.q_a, L.q_b};
  const RadiusScreen s = radius_screen(c, radius);
  hipError_t e;
  if ((e = hipMemsetAsync(decided, 0, sizeof(int32_t) * (size_t)n, st)) != hipSuccess) return e;
  if ((e = hipMemsetAsync(L.cnt, 0, sizeof(uint32_t) * 2 * (kThinMaxRounds + 1), st)) != hipSuccess) return e;
  int64_t nq = n, kept = 0;
  int32_t R = 0;
  while (nq > 0 && R < kThinMaxRounds) {
    ++R;
    const int32_t* in = R == 1 ? nullptr : queue[(R - 1) & 1];
    const unsigned blocks = (unsigned)((nq + kThinWaves - 1) / kThinWaves);
    thin_round_kernel<<<blocks, kThinBlock, 0, st>>>(c->xyz64, c->xyz32, g->dev, s.Rf, s.r2, s.bf, seed, R, in, nq,
                                                     decided, queue[R & 1], L.cnt);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    uint32_t h[2] = {0, 0};
    if ((e = hipMemcpyAsync(h, L.cnt + 2 * R, sizeof h, hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
    if ((e = hipStreamSynchronize(st)) != hipSuccess) return e;
    nq = (int64_t)h[0];
    kept += (int64_t)h[1];
  }
  *kept_out = kept;
  *rounds_out = R;
  if (nq > 0) {
    *why = "thin_min_distance: round bound reached with points undecided";
    return hipErrorUnknown;
  }
  return hipSuccess;
}

}  // namespace m3d
