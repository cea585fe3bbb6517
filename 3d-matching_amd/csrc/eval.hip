// eval.hip — registration evaluation (m3d_evaluate_registration): after the NN scan of a loop
// object, one pass takes every source's exact fp64 winner (the same expressions, hence the same
// bits, as icp.hip nn_finalize_kernel), writes idx / d² in the caller's source order and reduces,
// over the matched sources, the sums Open3D's EvaluateRegistration and
// GetInformationMatrixFromPointClouds need.
//
// Sums (kEvalUsed of kEvalSlots, fp64): count, Σd², and the nine moments of the matched TARGET
// points q = (x, y, z) in the target's original fp64 coordinates (m3d_cloud::xyz64 — GᵀG is not
// translation invariant, so not the centred fp32 frame): Σx Σy Σz, Σx² Σy² Σz², Σxy Σxz Σyz.
// The host assembles the 6×6 GᵀG of the rows G₁ = (0, z, −y, 1, 0, 0), G₂ = (−z, 0, x, 0, 1, 0),
// G₃ = (y, −x, 0, 0, 0, 1) from them (api.cpp eval_information).
//
// Order of summation (fixed, so two runs — and the brute-force and grid scans, which leave the
// same winners on the same Morton slots — give the same bits): a block holds 256 consecutive
// slots; each wave adds its 64 lanes in an xor butterfly (32, 16, …, 1: every lane ends with the
// same sum), the block adds its four wave sums in wave order into partials[block]; then one
// block adds the partials as icp.hip reduce_kernel does — group g takes blocks g, g + 32, … in
// increasing order, the 32 group sums are added in group order.  No floating-point atomics.
#include "m3d_internal.h"
#include "nnkey.h"

namespace m3d {

constexpr int kEvalSlots = 16;
constexpr int kEvalUsed = 11;
constexpr int kEvalBlock = 256;
constexpr int kEvalGroups = 32;
// eval_reduce_kernel's output words past the sums: the grid scan's deferral count and fault word
constexpr int kEvalDeferCount = 14;
constexpr int kEvalDeferFault = 15;

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) v += xor_lane_f64(v, o);
  return v;
}

// ns > 0 and nt > 0 (launch_eval keeps the empty cases away: no slot 0 to load)
__global__ __launch_bounds__(kEvalBlock) void eval_kernel(const double* __restrict__ pcd64,
                                                          const float4* __restrict__ src32, int64_t ns,
                                                          const double* __restrict__ tgt64, int64_t nt,
                                                          GridDev g, const IcpState* __restrict__ s,
                                                          const int64_t* __restrict__ keys,
                                                          const uint32_t* __restrict__ near2,
                                                          const int32_t* __restrict__ slot, int with_info,
                                                          int32_t* __restrict__ idx, double* __restrict__ d2out,
                                                          double* __restrict__ partials) {
  __shared__ double red[kEvalBlock / kWave][kEvalSlots];
  const int64_t i0 = (int64_t)blockIdx.x * kEvalBlock + threadIdx.x;
  const bool valid = i0 < ns;
  const int64_t i = valid ? i0 : 0;
  double Q[3];
  q64_of(s->dT, pcd64 + 3 * i, Q);
  int64_t gj;
  double d;
  winner_fp64(valid, valid ? (uint64_t)keys[i] : (uint64_t)kKeyNone,
              valid ? __uint_as_float(near2[i]) : kInf, s, g, tgt64, 0, nt, src32[i], Q, gj, d);
  const bool hit = valid && gj >= 0 && gj < nt;
  if (valid) {
    const int64_t o = slot != nullptr ? (int64_t)slot[i] : i;  // slot → the caller's source order
    if (idx != nullptr) idx[o] = hit ? (int32_t)gj : -1;
    if (d2out != nullptr) d2out[o] = hit ? d : INFINITY;
  }
  double v[kEvalUsed];
#pragma unroll
  for (int k = 0; k < kEvalUsed; ++k) v[k] = 0.0;
  if (hit) {
    v[0] = 1.0;
    v[1] = d;
    if (with_info) {
      const double* q = tgt64 + 3 * gj;
      const double x = q[0], y = q[1], z = q[2];
      v[2] = x;
      v[3] = y;
      v[4] = z;
      v[5] = x * x;
      v[6] = y * y;
      v[7] = z * z;
      v[8] = x * y;
      v[9] = x * z;
      v[10] = y * z;
    }
  }
  const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave;
#pragma unroll
  for (int k = 0; k < kEvalUsed; ++k) {
    const double t = wave_sum(v[k]);
    if (lane == 0) red[w][k] = t;
  }
  __syncthreads();
  if (threadIdx.x < kEvalSlots) {
    double t = 0.0;
    if (threadIdx.x < kEvalUsed)
      for (int k = 0; k < kEvalBlock / kWave; ++k) t += red[k][threadIdx.x];
    partials[(int64_t)blockIdx.x * kEvalSlots + threadIdx.x] = t;
  }
}

// out[0 .. kEvalUsed) = the sums over the nblocks partials (nblocks = 0: zeros), and the deferral
// header of the grid scan (hcnt null: zeros): result and fault word reach the host together
__global__ __launch_bounds__(kEvalGroups * kEvalSlots) void eval_reduce_kernel(
    const double* __restrict__ partials, int64_t nblocks, const uint32_t* __restrict__ hcnt,
    double* __restrict__ out) {
  __shared__ double red[kEvalGroups][kEvalSlots];
  const int sl = threadIdx.x & (kEvalSlots - 1);
  const int g = threadIdx.x / kEvalSlots;
  double v = 0.0;
  for (int64_t b = g; b < nblocks; b += kEvalGroups) v += partials[b * kEvalSlots + sl];
  red[g][sl] = v;
  __syncthreads();
  if (threadIdx.x < kEvalSlots) {
    double t = 0.0;
    for (int k = 0; k < kEvalGroups; ++k) t += red[k][threadIdx.x];
    if (threadIdx.x == kEvalDeferCount) t = hcnt != nullptr ? (double)hcnt[0] : 0.0;
    if (threadIdx.x == kEvalDeferFault) t = hcnt != nullptr ? (double)hcnt[kDeferFault] : 0.0;
    out[threadIdx.x] = t;
  }
}

// no target: every source is unmatched
__global__ __launch_bounds__(kEvalBlock) void eval_fill_kernel(int64_t ns, int32_t* __restrict__ idx,
                                                               double* __restrict__ d2out) {
  const int64_t i = (int64_t)blockIdx.x * kEvalBlock + threadIdx.x;
  if (i >= ns) return;
  if (idx != nullptr) idx[i] = -1;
  if (d2out != nullptr) d2out[i] = INFINITY;
}

int64_t eval_blocks(int64_t ns) { return ns > 0 ? (ns + kEvalBlock - 1) / kEvalBlock : 0; }
size_t eval_scratch_bytes(int64_t ns) {
  return sizeof(double) * (size_t)kEvalSlots * (size_t)std::max<int64_t>(eval_blocks(ns), 1);
}

// partials: eval_scratch_bytes(ns) bytes of device scratch; out: kEvalSlots doubles the host can
// read after a stream sync (the context's mapped pinned memory).  The loop's NN scan for the
// current transform must have been enqueued on st before.
hipError_t launch_eval(const m3d_icp* s, int with_info, int32_t* idx, double* d2, double* partials,
                       double* out, hipStream_t st) {
  const int64_t ns = s->src->n, nt = s->tgt->n;
  const int64_t nb = (ns == 0 || nt == 0) ? 0 : eval_blocks(ns);
  if (nb > 0)
    eval_kernel<<<(unsigned)nb, kEvalBlock, 0, st>>>(s->pcd64, s->src->xyz32, ns, s->tgt->xyz64, nt,
                                                    s->tgrid->dev, s->state, s->keys, s->near2,
                                                    s->src->slot, with_info, idx, d2, partials);
  eval_reduce_kernel<<<1, kEvalGroups * kEvalSlots, 0, st>>>(partials, nb, s->hcnt, out);
  return hipGetLastError();
}

hipError_t launch_eval_fill(int64_t ns, int32_t* idx, double* d2, hipStream_t st) {
  if (ns == 0 || (idx == nullptr && d2 == nullptr)) return hipSuccess;
  eval_fill_kernel<<<(unsigned)eval_blocks(ns), kEvalBlock, 0, st>>>(ns, idx, d2);
  return hipGetLastError();
}

}  // namespace m3d
