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
// G₃ = (y, −x, 0, 0, 0, 1) from them (api_icp.cpp eval_information).
//
// Order of summation: the loop's fixed order (icp.hip, "reduce"; nnkey.h block_partial per block
// of 256 consecutive slots, launch_reduce over the block partials) — two runs, and the brute-force
// and grid scans, which leave the same winners on the same Morton slots, give the same bits.
#include "m3d_internal.h"
#include "nnkey.h"

namespace m3d {

constexpr int kEvalSlots = 16;
constexpr int kEvalUsed = 11;
constexpr int kEvalBlock = 256;

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
  const SlotWinner w = slot_winner((int64_t)blockIdx.x * kEvalBlock + threadIdx.x, pcd64, src32, ns, tgt64, nt, g, s,
                                   keys, near2);
  if (w.valid) {
    const int64_t o = slot != nullptr ? (int64_t)slot[w.i] : w.i;  // slot → the caller's source order
    if (idx != nullptr) idx[o] = w.hit ? (int32_t)w.gj : -1;
    if (d2out != nullptr) d2out[o] = w.hit ? w.d : INFINITY;
  }
  double v[kEvalUsed];
#pragma unroll
  for (int k = 0; k < kEvalUsed; ++k) v[k] = 0.0;
  if (w.hit) {
    v[0] = 1.0;
    v[1] = w.d;
    if (with_info) {
      const double* q = tgt64 + 3 * w.gj;
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
  block_partial<kEvalSlots, kEvalUsed, kEvalBlock>(v, partials);
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
// read after a stream sync (the context's mapped pinned memory): the sums over the partials (no
// blocks: zeros) and, in its last two words, the grid scan's deferral count and fault word (brute
// force: zeros) — result and fault word reach the host together.  The loop's NN scan for the
// current transform must have been enqueued on st before.
hipError_t launch_eval(const m3d_icp* s, int with_info, int32_t* idx, double* d2, double* partials,
                       double* out, hipStream_t st) {
  const int64_t ns = s->src->n, nt = s->tgt->n;
  const int64_t nb = (ns == 0 || nt == 0) ? 0 : eval_blocks(ns);
  if (nb > 0)
    eval_kernel<<<(unsigned)nb, kEvalBlock, 0, st>>>(s->pcd64, s->src->xyz32, ns, s->tgt->xyz64, nt,
                                                    s->tgrid->dev, s->state, s->keys, s->near2,
                                                    s->src->slot, with_info, idx, d2, partials);
  return launch_reduce(partials, nb, kEvalSlots, out, nullptr, s->hcnt, st);
}

hipError_t launch_eval_fill(int64_t ns, int32_t* idx, double* d2, hipStream_t st) {
  if (ns == 0 || (idx == nullptr && d2 == nullptr)) return hipSuccess;
  eval_fill_kernel<<<(unsigned)eval_blocks(ns), kEvalBlock, 0, st>>>(ns, idx, d2);
  return hipGetLastError();
}

}  // namespace m3d
