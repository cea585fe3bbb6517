// icp.hip — ICP refinement for gfx950.
//
// Reference: src/matcher/icp.py:42-48 → Open3D 0.19 RegistrationICP with
// TransformationEstimationPointToPlane and ICPConvergenceCriteria(1e-6, 1e-6, 30).
// One iteration = Eval(T) [1-NN within r, fitness, rmse] + ComputeTransformation + T ← ΔT·T.
//
// Kernels per iteration (all device resident, no host round trip):
//   keyinit  O(Ns)      seeds each query's bound with its previous neighbour (fp32 d²)
//   nn       O(Ns·Nt)   brute-force scan (nn_brute.hip, nn_mfma_kernel): the key of nnkey.h, packed
//                       (bits(d²) << 32 | idx) with lexicographic (d², index) argmin — the same
//                       result as a full direct fp32 scan; the screen's error bounds come from
//                       refresh_rt32 here.  (grid.hip: the radius-bounded grid search, same key.)
//   terms_solve O(Ns)   fp64: radius test d² < r² (strict, nanoflann), point-to-plane
//                       J = [p×n ; n], r = (p−q)·n → JTJ(21) JTr(6) Σr²; count; Σd² → block
//                       partials; the last block reduces them in a fixed order and one wave runs
//                       the solve (fitness/rmse, convergence test, LDLT(JTJ, −JTr),
//                       x → Rz·Ry·Rx|t, T ← ΔT·T).
// The multi-GPU paths use the same pieces as separate launches (terms_kernel, reduce_kernel,
// solve_kernel) with the RCCL MIN on keys / SUM on the 32 term slots between them.
#include <float.h>

#include <algorithm>
#include <string>
#include <type_traits>
#include <vector>
#include <stdlib.h>

#include "lds_dma.h"
#include "linalg.h"
#include "m3d_internal.h"
#include "nnkey.h"

namespace m3d {

// terms pass geometry: 512-thread blocks, one source per thread (196 block partials at cfg1, as
// 256 × 2 gave): two waves per SIMD share the fp64 work and hide each other's round trips — the
// last terms wave of a cfg1 evaluation ends ≈ 1 µs sooner (docs/EXPERIMENTS.md §R6)
constexpr int kTermsBlock = 512;
constexpr double kU = 5.9604644775390625e-08;
constexpr double kU64 = 1.1102230246251565e-16;

// nn_brute_terms.hip compiles this file again with M3D_ICP_TERMS_ONLY=1 and keeps only the terms
// pass (terms_block and what it calls) for the NN kernel that runs it in place
#ifndef M3D_ICP_TERMS_ONLY
#define M3D_ICP_TERMS_ONLY 0
#endif
#if !M3D_ICP_TERMS_ONLY

// ------------------------------------------------------------------------------- state
// FrameParams: m3d_internal.h
// Refresh the fp32 search transform and radius bound for transform T (device side; T and
// r2 = s->r2 passed in registers by the solve, which has them already).
// fp64 → fp32 rounded toward +inf on the vector unit (the library's __double2float_ru bounces the
// bits through the scalar unit, ≈ 20 dependent instructions each, five of them per refresh):
// the round-to-nearest value, moved one ulp up when it lies below d (−0 / +0 → the least denormal)
__device__ __forceinline__ float f32_ru(double d) {
  const float f = (float)d;
  const uint32_t u = __float_as_uint(f);
  const uint32_t up = f == 0.0f ? 1u : ((int32_t)u >= 0 ? u + 1u : u - 1u);
  return (double)f < d ? __uint_as_float(up) : f;
}

// r = √r2, taken by the caller (the solve computes it while its factorisation runs)
__device__ void refresh_rt32_from(IcpState* s, const double* T, double r2, double r, const FrameParams& f,
                                  int iters) {
  const double* cs = f.cs;
  const double* ct = f.ct;
  const double pinf = f.pinf, qinf = f.qinf;
  double rowl1 = 0.0, tinf = 0.0;
  for (int i = 0; i < 3; ++i) {
    const double* r = T + 4 * i;
    const double tp = fma(r[2], cs[2], fma(r[1], cs[1], r[0] * cs[0])) + r[3] - ct[i];
    for (int j = 0; j < 3; ++j) s->Rt32[3 * i + j] = (float)r[j];
    s->Rt32[9 + i] = (float)tp;
    rowl1 = fmax(rowl1, fabs(r[0]) + fabs(r[1]) + fabs(r[2]));
    tinf = fmax(tinf, fabs(tp));
  }
  // E: per-coordinate bound on |fp32 query − fp64 query| + |fp32 target − fp64 target| in the
  // centred frame: the fp32 roundings of p_c, R, t' and the three fmas (≤ 5u·Σ|r||p| + 4u|t'|),
  // the target's u|t_c|, and the fp64 query Q of the contract against T·p: Q is the source
  // transformed update by update (Open3D's pcd.Transform(update), IcpState::dT), so each of the
  // iters + 1 applications adds ≤ 4 roundings of 2⁻⁵³ of the magnitudes involved; the updates
  // are rotations to fp64 accuracy, which carry the earlier errors over without growth in the
  // 2-norm (√3 per coordinate).  The last term covers an init within 1e-12 of the identity,
  // which Open3D does not apply to the points (Eigen isIdentity) while T = init.
  double tabs = 0.0, csinf = 0.0, ctinf = 0.0;
  for (int i = 0; i < 3; ++i) {
    tabs = fmax(tabs, fabs(T[4 * i + 3]));
    csinf = fmax(csinf, fabs(cs[i]));
    ctinf = fmax(ctinf, fabs(ct[i]));
  }
  const double mag = rowl1 * (csinf + pinf) + tabs + ctinf + qinf;
  // the fp32 part, term by term (xform32: q = fma(r0, px, fma(r1, py, fma(r2, pz, t′)))):
  // p rounding u·Σ|r||p| + R rounding u·Σ|r||p| + three fma roundings ≤ 3u(Σ|r||p| + |t′|) +
  // t′ rounding u|t′| + the target's u|t_c|, Σ|r||p| ≤ ‖r‖₁·|p|∞; ×1.01 for the O(u²) products.
  // (Term by term because the fp32 → fp64 ambiguity band, hence the terms pass's fp64 walks, scale
  // with E.)
  const double E32 = 1.01 * kU * (5.0 * rowl1 * pinf + 4.0 * tinf + qinf);
  const double E = E32 + 8.0 * kU64 * 1.7320508075688772 * (double)(iters + 2) * mag + 1e-11 * (mag + 1.0);
  // nnkey.h: |√d2f − |Q − t|| ≤ e_q + 3u√d2f with e_q = √3·E; band_of's absolute term 2·e_q
  const double eq = 1.7320508075688772 * E * 1.01;
  const float eqf = f32_ru(eq), bef = f32_ru(2.0 * eq * 1.01);
  s->eq = isfinite(eqf) ? eqf : FLT_MAX;
  s->band_e = isfinite(bef) ? bef : FLT_MAX;
  const double e = 2.0 * (3.0 * kU * (r + 1.7320508075688772 * E) * (r + 1.7320508075688772 * E) +
                          2.0 * 1.7320508075688772 * E * r + 3.0 * E * E);
  float hi = f32_ru(r2 + e);
  if (!isfinite(hi)) hi = FLT_MAX;
  s->r2_hi = hi;
  // Screen bound: |fl(|t|² − 2q·t) − (d² − |q|²)| + rounding of thr ≤ eps,
  // with |t|∞ ≤ qinf (target), |q|∞ ≤ Q = rowl1·pinf + |t'|∞ (query after the transform).
  const double Q = rowl1 * pinf + tinf;
  const double E1 = 5.0 * kU * (3.0 * qinf * qinf + 6.0 * Q * qinf);
  const double es = 2.0 * (E1 + 6.0 * kU * (double)hi + 12.0 * kU * Q * Q) + 1e-30;
  const float esf = f32_ru(es);
  s->screen_eps = isfinite(esf) ? esf : FLT_MAX;
  // MFMA screen (nn_mfma_kernel): the same key from fp16 hi/lo operands scaled
  // by S = s16, in S² units.  Per coordinate a = −2Sq, t = St split as x = xh + xl + r with
  // |r| ≤ u16²|x| + 2σ (u16 = 2⁻¹¹, σ = 2⁻²⁵ fp16 subnormal half-spacing); the dropped al·tl and
  // the split remainders cost ≤ 3u16²|a||t| + 4σ(|a| + |t|) per coordinate, the w = S²|t|² split
  // u16²|w| + 2σ; the 11 exact fp16 products are accumulated in fp32 by the MFMA in an
  // unspecified order: ≤ 32·u·Σ|products| (a bound for ≤ 16 additions even if each rounds by a
  // full ulp).  Back in unscaled units (÷ S²) plus the stored-|t|² rounding u·|t|².
  const double S = f.s16;
  const double As = 2.0 * Q * S, Ts = qinf * S;
  const double Ws = 3.0 * Ts * Ts * (1.0 + 1e-6);
  const double u16 = 4.8828125e-04, sig = 2.98023223876953125e-08;
  const double P = 3.0 * As * Ts;
  const double Esplit = 3.0 * u16 * u16 * P + 4.0 * sig * 3.0 * (As + Ts) + u16 * u16 * Ws + 2.0 * sig;
  const double Eacc = 32.0 * kU * 1.01 * (P + Ws);
  const double E1m = 1.05 * (Esplit + Eacc) / (S * S) + kU * 3.0 * qinf * qinf;
  const double esm = 2.0 * (E1m + 6.0 * kU * (double)hi + 12.0 * kU * Q * Q) + 1e-30;
  const float esmf = f32_ru(esm);
  s->screen_eps_m = isfinite(esmf) ? esmf : FLT_MAX;
  s->mfma_scale = (float)S;
  // operands must stay well inside the fp16 range (max 65504) and the bound finite
  s->mfma_ok = (As < 16384.0 && Ts < 16384.0 && Ws < 16384.0 && isfinite(esmf) &&
                hi < FLT_MAX && esmf < 0.25f * FLT_MAX) ? 1 : 0;
}

__device__ void refresh_rt32(IcpState* s, const FrameParams& f) {
  double T[16];
  for (int k = 0; k < 16; ++k) T[k] = s->T[k];
  refresh_rt32_from(s, T, s->r2, sqrt(s->r2), f, s->iters);
}

__device__ __forceinline__ void set_identity(double* M) {
  for (int k = 0; k < 16; ++k) M[k] = (k % 5 == 0) ? 1.0 : 0.0;
}

// The common end of the state-setup kernels below, after T and dT are written: nothing evaluated
// yet, radius r2, the search transform of T.  bound_ok = 0: keys / corr belong to another
// transform, so no bound seeds until the next update.
__device__ __forceinline__ void reset_eval(IcpState* s, double r2, const FrameParams& f) {
  s->fitness = s->rmse = s->prev_fitness = s->prev_rmse = 0.0;
  s->count = 0;
  s->evals = s->iters = s->done = s->converged = 0;
  s->ticket = 0;
  s->plan_ok = 0;  // the next NN launch runs the uniform slices: a run's launch shapes are its own
  s->r2 = r2;
  s->bound_ok = 0;
  refresh_rt32(s, f);
  s->eq_prev = s->eq;
}

// apply_init: the points start as init·p (the loop's pcd64 holds p, dT = init); 0: as p (dT = I),
// Open3D's RegistrationICP for an init that isIdentity() — T still starts at init
__global__ void icp_init_kernel(IcpState* s, double T0, double T1, double T2, double T3, double T4,
                                double T5, double T6, double T7, double T8, double T9, double T10,
                                double T11, double r2, FrameParams f, int apply_init) {
  if (threadIdx.x != 0) return;
  const double T[12] = {T0, T1, T2, T3, T4, T5, T6, T7, T8, T9, T10, T11};
  for (int k = 0; k < 12; ++k) s->T[k] = T[k];
  s->T[12] = s->T[13] = s->T[14] = 0.0;
  s->T[15] = 1.0;
  for (int k = 0; k < 16; ++k) s->dT[k] = apply_init ? s->T[k] : ((k % 5 == 0) ? 1.0 : 0.0);
  set_identity(s->last_upd);
  reset_eval(s, r2, f);
}

// state for evaluating transform T (device, row-major 4×4): feature-RANSAC validation (a6)
__global__ void icp_set_T_kernel(IcpState* s, const double* __restrict__ T, double r2, FrameParams f) {
  if (threadIdx.x != 0) return;
  for (int k = 0; k < 16; ++k) s->T[k] = s->dT[k] = T[k];  // the loop's pcd64 holds p
  set_identity(s->last_upd);
  reset_eval(s, r2, f);
}

// a6 batched validation (grid.hip validate_kernel): one evaluation state per hypothesis, with
// icp_set_T's semantics, for the hypotheses list[0..n) of the transform array T
__global__ __launch_bounds__(64) void val_states_kernel(IcpState* __restrict__ states,
                                                        const double* __restrict__ T,
                                                        const int32_t* __restrict__ list, int64_t n,
                                                        double r2, FrameParams f) {
  const int64_t k = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (k >= n) return;
  IcpState* s = states + k;
  const double* Th = T + 16 * (int64_t)list[k];
  for (int j = 0; j < 16; ++j) s->T[j] = s->dT[j] = Th[j];  // validation reads the source itself
  reset_eval(s, r2, f);
}

// ------------------------------------------------------------------------------- keyinit
__global__ __launch_bounds__(256) void keyinit_kernel(const float4* __restrict__ src32, int64_t ns,
                                                      const float4* __restrict__ tgt32,
                                                      int64_t nt_shard, int64_t off,
                                                      const IcpState* __restrict__ s,
                                                      const int32_t* __restrict__ prev,
                                                      const int64_t* __restrict__ dprev,
                                                      int64_t* __restrict__ keys,
                                                      uint32_t* __restrict__ near2, int64_t q0) {
  // keys ← seed_key (nnkey.h), near2 ← none; sources [q0, ns)
  if (s->done) return;
  const int64_t i = q0 + (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= ns) return;
  const float* Rt = s->Rt32;  // uniform → scalar loads (a local copy went to scratch)
  const float4 p = src32[i];
  float x, y, z;
  xform32(Rt, p, x, y, z);
  keys[i] = seed_key(s, i, p, x, y, z, tgt32, nt_shard, off, prev, dprev);
  near2[i] = kNearNone;
}

#endif  // !M3D_ICP_TERMS_ONLY
// ------------------------------------------------------------------------------- terms
// Transposing wave reduction of 32 per-lane slots: each butterfly step halves the slots a lane
// keeps (the partner gets the other half), so 32 slots cost 31 pair exchanges instead of
// 32 × 6 full butterflies.  Steps 32 and 16 use the gfx950 permlane swaps (no selects);
// 8, 4, 2 exchange by DPP moves; the last step adds the two lanes of a pair.  Afterwards lanes
// 2k and 2k+1 both hold the wave's sum of slot k.  A fixed tree: deterministic.
template <bool k32>
__device__ __forceinline__ double swap_add(double a, double b) {
  const uint64_t ua = (uint64_t)__double_as_longlong(a), ub = (uint64_t)__double_as_longlong(b);
  const uint32_t alo = (uint32_t)ua, ahi = (uint32_t)(ua >> 32);
  const uint32_t blo = (uint32_t)ub, bhi = (uint32_t)(ub >> 32);
  const auto rl = k32 ? __builtin_amdgcn_permlane32_swap(alo, blo, false, false)
                      : __builtin_amdgcn_permlane16_swap(alo, blo, false, false);
  const auto rh = k32 ? __builtin_amdgcn_permlane32_swap(ahi, bhi, false, false)
                      : __builtin_amdgcn_permlane16_swap(ahi, bhi, false, false);
  const double na = __longlong_as_double((long long)(((uint64_t)rh[0] << 32) | rl[0]));
  const double nb = __longlong_as_double((long long)(((uint64_t)rh[1] << 32) | rl[1]));
  return na + nb;  // lanes of bit 0: a-slot over both halves; bit 1: b-slot
}

// the partner's half arrives by DPP (nnkey.h xor_lane_f64: all lanes active), without the LDS
// unit's round trip
template <int kOff>
__device__ __forceinline__ double xchg_add(double a, double b, int lane) {
  const bool hi = (lane & kOff) != 0;
  const double keep = hi ? b : a, send = hi ? a : b;
  return keep + xor_lane_f64(send, kOff);
}

__device__ __forceinline__ double wave_transpose_sum32(const double (&v)[32], int lane) {
  double w16[16], w8[8], w4[4], w2[2];
#pragma unroll
  for (int j = 0; j < 16; ++j) w16[j] = swap_add<true>(v[j], v[j + 16]);
#pragma unroll
  for (int j = 0; j < 8; ++j) w8[j] = swap_add<false>(w16[j], w16[j + 8]);
#pragma unroll
  for (int j = 0; j < 4; ++j) w4[j] = xchg_add<8>(w8[j], w8[j + 4], lane);
#pragma unroll
  for (int j = 0; j < 2; ++j) w2[j] = xchg_add<4>(w4[j], w4[j + 2], lane);
  const double w1 = xchg_add<2>(w2[0], w2[1], lane);
  return w1 + xor_lane_f64(w1, 1);  // slot lane >> 1
}

// One source's contribution to the 30 term slots (layout below), in a fixed operation order:
// every terms pass (terms_block, single device or shard) adds a source through this function,
// so equal winners give equal bits.  Q = the fp64 transformed source, q / n its winner's point and
// normal, d2 = the winner's fp64 d², c = the source centre (point-to-point).
template <int kEst>
__device__ __forceinline__ void terms_add(double (&acc)[30], const double (&Q)[3], const double (&q)[3],
                                          const double (&n)[3], double d2, const double (&c)[3]) {
  const double d[3] = {Q[0] - q[0], Q[1] - q[1], Q[2] - q[2]};
  acc[28] += 1.0;
  acc[29] += d2;
  if (kEst == M3D_EST_POINT_TO_PLANE) {
    const double r = d[0] * n[0] + d[1] * n[1] + d[2] * n[2];
    double J[6];
    cross3(Q, n, J);
    J[3] = n[0];
    J[4] = n[1];
    J[5] = n[2];
    int k = 0;
#pragma unroll
    for (int x = 0; x < 6; ++x)
#pragma unroll
      for (int y = x; y < 6; ++y) acc[k++] += J[x] * J[y];
#pragma unroll
    for (int x = 0; x < 6; ++x) acc[21 + x] += J[x] * r;
    acc[27] += r * r;
  } else {
    const double pc[3] = {Q[0] - c[0], Q[1] - c[1], Q[2] - c[2]};
    const double qc[3] = {q[0] - c[0], q[1] - c[1], q[2] - c[2]};
#pragma unroll
    for (int x = 0; x < 3; ++x) {
      acc[x] += pc[x];
      acc[3 + x] += qc[x];
#pragma unroll
      for (int y = 0; y < 3; ++y) acc[6 + 3 * x + y] += pc[x] * qc[y];
    }
  }
}

// Inputs of the terms pass.  Winner of source i:
//  * claim == nullptr (one device, or a source shard against the whole target): the fp64 winner
//    decided from the scan keys (nnkey.h winner_fp64; ambiguous queries resolved over the
//    target grid g);
//  * claim != nullptr (target shard, after the two MIN exchanges of m3d_icp_shard_*): claim[i],
//    the global winner (INT32_MAX none), whose fp64 d² every rank knows from dmin; the rank
//    owning the target adds its terms.  dmin is kept in dprev for the next bound seeds.
struct TermsArgs {
  double* pcd64;          // the loop's fp64 points: the query is dT·pcd64[i], written back (Open3D's
                          // pcd.Transform(update): the next update applies to these)
  const float4* src32;
  int64_t ns;
  const double* tgt64;
  const double* nrm64;
  const double* rec64;    // the target's 64-B records (point, normal), or null: tgt64 / nrm64
  int64_t nt_shard, off;
  const int64_t* keys;
  uint32_t* near2;
  GridDev g;
  const int32_t* claim;
  const int64_t* dmin;
  int64_t* dprev;
  int32_t* corr;
  int est;
  double c[3];
  int64_t* reset_keys;   // fused single-device loop: hand the keys back as kKeyNone
  float4* seed;          // with reset_keys and rec64: the next scan's seed records (below), else null
};
// What the NN kernel that runs the terms pass in place (nn_brute.hip nn_mfma_terms_kernel) reads
// through ONE kernel argument: a device-resident copy, written when the loop is created — every
// member points into the loop's state or is a constant of the loop
struct NnTermsDev {
  TermsArgs a;       // terms_args(s, 0, no claim, reset_keys)
  double* partials;
  uint32_t* tix;     // per query block: the slices that have published (m3d_icp::nn_tix)
};

// est: M3D_EST_POINT_TO_PLANE → slots 0..20 JTJ (upper, row-major), 21..26 JTr, 27 Σr²
//      M3D_EST_POINT_TO_POINT → slots 0..2 Σp_c, 3..5 Σq_c, 6..14 Σ p_c q_cᵀ (row-major)
// both: 28 count, 29 Σd²  (c = source centre: identical on every shard)
// kWT: write the block partial through to memory (sc1 store) for the fused last-block reduce.
// One source per thread, in two load rounds: (1) its key / runner-up / fp64 point (or claim /
// dmin), (2) after the fp64 decision, the winner's fp64 target (and normal); the rare ambiguous
// queries are resolved by the whole wave in between (nnkey.h resolve_wave, one ballot when there
// are none).
#if M3D_TAIL_CLOCK  // diagnostic builds only (tools/tail_clock.py): per-wave start / end of the
                    // terms pass, the last block's ticket, reduce and solve steps (100 MHz), and
                    // per wave the number of ambiguous queries it resolved
__device__ unsigned long long g_tail_clock[3 * 4096 + 24];  // + 16 finer stamps at 3·4096 + 8
#endif
// kEst: the estimator as a template parameter (one path compiled per kernel: a runtime branch
// between the two accumulation forms kept two accumulators in scratch memory)
#if M3D_TERMS_CLOCK  // diagnostic builds only (tools/terms_phases.py): per wave, stamps at the terms
                     // pass's phase ends, each after s_waitcnt 0 (the phases serialise), kept in
                     // registers and stored at the end
__device__ unsigned long long g_terms_clock[4096 * 8];
#define M3D_TPH(k)                               \
  do {                                           \
    __builtin_amdgcn_s_waitcnt(0);               \
    tph_[k] = __builtin_amdgcn_s_memrealtime();  \
  } while (0)
#else
#define M3D_TPH(k) \
  do {             \
  } while (0)
#endif
// bx: the block's index (its 512 sources and its partial).  kSc1: the keys and runner-ups are read
// with sc1 loads — the caller is the NN kernel whose blocks published them a moment ago
// (nn_brute.hip nn_terms_handoff).
template <bool kWT, int kEst, bool kSc1 = false>
__device__ __forceinline__ void terms_block(const TermsArgs& a, const IcpState* __restrict__ s,
                                            double* __restrict__ partials, const unsigned bx) {
  __shared__ double red[kTermSlots][kTermsBlock / kWave];
#if M3D_TERMS_CLOCK
  unsigned long long tph_[8];
#endif
  M3D_TPH(0);
  double acc[30];
#pragma unroll
  for (int k = 0; k < 30; ++k) acc[k] = 0.0;
  // One source per thread, still written as kP = 1 rounds of one-element arrays (the form of the
  // rounds-5/6 "sources per thread" experiments): with scalars and no `u` loops the compiler emits a
  // different instruction stream for the four terms kernels (docs/EXPERIMENTS.md §R9), so that
  // rewrite waits for a change that re-times them anyway.
  constexpr int kP = 1;
  int64_t ii[kP];
  bool valid[kP];
  double vs[kP][3];
  int64_t gj[kP];
  double d2[kP];
  bool fixed[kP];  // winner and d² already final (resolved in fp64, or given by the claim)
  uint64_t k1[kP];
  float n2[kP];
#pragma unroll
  for (int u = 0; u < kP; ++u) {
    const int64_t i = ((int64_t)bx * kP + u) * kTermsBlock + threadIdx.x;
    valid[u] = i < a.ns;
    ii[u] = valid[u] ? i : 0;
    gj[u] = -1;
    d2[u] = 0.0;
    fixed[u] = true;
    if (kSc1) {
      k1[u] = valid[u] ? (uint64_t)__hip_atomic_load(&a.keys[ii[u]], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                       : (uint64_t)kKeyNone;
      n2[u] = valid[u] ? __uint_as_float(__hip_atomic_load(&a.near2[ii[u]], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
                       : kInf;
    } else if (a.claim == nullptr) {
      k1[u] = valid[u] ? (uint64_t)a.keys[ii[u]] : (uint64_t)kKeyNone;
      n2[u] = valid[u] ? __uint_as_float(a.near2[ii[u]]) : kInf;
    } else if (valid[u]) {
      const int32_t cj = a.claim[ii[u]];
      const int64_t dm = a.dmin[ii[u]];
      if (cj != 0x7FFFFFFF) {
        gj[u] = cj;
        d2[u] = __longlong_as_double(dm);
      }
      if (a.dprev != nullptr) a.dprev[ii[u]] = dm;
    }
    q64_of(s->dT, a.pcd64 + 3 * ii[u], vs[u]);
    if (valid[u])
      for (int k = 0; k < 3; ++k) a.pcd64[3 * ii[u] + k] = vs[u][k];
  }
  M3D_TPH(1);
  if (a.claim == nullptr) {
    bool amb[kP];
    float X[kP], qx[kP], qy[kP], qz[kP];
    int64_t bj[kP];
    double bd[kP];
#pragma unroll
    for (int u = 0; u < kP; ++u) {
      if (valid[u] && a.reset_keys != nullptr) {
        a.reset_keys[ii[u]] = kKeyNone;
        a.near2[ii[u]] = kNearNone;
      }
      // nnkey.h winner_fp64, split: ambiguous queries resolved here by the wave, the others'
      // candidate (k1's target) re-evaluated in fp64 after the batched target loads below
      X[u] = valid[u] && k1[u] != (uint64_t)kKeyNone ? search_bound(key_d2(k1[u]), s->band_e, s->r2_hi) : -1.0f;
      amb[u] = X[u] >= 0.0f && n2[u] <= X[u];
#if M3D_TAIL_CLOCK
      {
        const int64_t gw = (int64_t)bx * (kTermsBlock / kWave) + threadIdx.x / kWave;
        const int na = __popcll(__ballot(amb[u]));
        if ((threadIdx.x & (kWave - 1)) == 0 && gw < 4096) g_tail_clock[2 * 4096 + 8 + gw] = na;
      }
#endif
      qx[u] = qy[u] = qz[u] = 0.0f;
      if (amb[u]) xform32(s->Rt32, a.src32[ii[u]], qx[u], qy[u], qz[u]);
      bj[u] = -1;
      bd[u] = 0.0;
    }
    // the wave's ambiguous queries in one walk, two at a time (nnkey.h)
    resolve_wave(amb[0], a.g, a.tgt64, a.off, qx[0], qy[0], qz[0], X[0], vs[0], s->r2, bj[0], bd[0]);
#pragma unroll
    for (int u = 0; u < kP; ++u) {
      if (amb[u]) {
        gj[u] = bj[u];
        d2[u] = bd[u];
      } else if (valid[u] && key_real(k1[u])) {
        const int64_t c = (int64_t)(uint32_t)k1[u];
        if (c >= a.off && c < a.off + a.nt_shard) {
          gj[u] = c;
          fixed[u] = false;
        }
      }
    }
  }
  M3D_TPH(2);
  double tq[kP][3], tn[kP][3];
  double pad[kP][2];  // the record's last 16 bytes: the target's centred fp32 point (pack_rec_kernel)
#pragma unroll
  for (int u = 0; u < kP; ++u) {
    pad[u][0] = pad[u][1] = 0.0;
    const bool own = valid[u] && gj[u] >= a.off && gj[u] < a.off + a.nt_shard;
    // branch-free: a source whose winner is not on this shard loads target 0 and drops it — but
    // an EMPTY target shard has no target 0 (no arrays at all): nothing is loaded there
    const int64_t l = own ? gj[u] - a.off : 0;
    if (a.nt_shard == 0) {
      for (int k = 0; k < 3; ++k) tq[u][k] = tn[u][k] = 0.0;
    } else if (a.rec64 != nullptr) {
      const double4 r0 = reinterpret_cast<const double4*>(a.rec64)[2 * l];
      const double4 r1 = reinterpret_cast<const double4*>(a.rec64)[2 * l + 1];
      tq[u][0] = r0.x;
      tq[u][1] = r0.y;
      tq[u][2] = r0.z;
      tn[u][0] = r0.w;
      tn[u][1] = r1.x;
      tn[u][2] = r1.y;
      pad[u][0] = r1.z;
      pad[u][1] = r1.w;
    } else {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        tq[u][k] = a.tgt64[3 * l + k];
        tn[u][k] = kEst == M3D_EST_POINT_TO_PLANE ? a.nrm64[3 * l + k] : 0.0;
      }
    }
  }
  M3D_TPH(3);
#pragma unroll
  for (int u = 0; u < kP; ++u) {
    if (!valid[u]) continue;
    if (!fixed[u]) {  // k1's target: the fp64 winner iff its d64 < r²
      const double d = d2_64(vs[u], tq[u]);
      if (d < s->r2) {
        d2[u] = d;
      } else {
        gj[u] = -1;
      }
    }
    const int64_t i = ii[u];
    if (a.corr != nullptr) a.corr[i] = (int32_t)gj[u];
    // Seed record of the next self-seeded scan (nnkey.h seed_key_rec): the final winner's fp32
    // point — the record gathered above is gj's, resolved winners included — and its index, −1
    // none (then the point is never read).  Only the fused tail that hands the keys back has the
    // pointer: keys_clean ⇒ seed[i] describes corr[i].
    if (kWT && a.seed != nullptr) {
      a.seed[i] = make_float4(__int_as_float(__double2loint(pad[u][0])), __int_as_float(__double2hiint(pad[u][0])),
                              __int_as_float(__double2loint(pad[u][1])), __int_as_float((int32_t)gj[u]));
    }
    if (gj[u] < a.off || gj[u] >= a.off + a.nt_shard) continue;  // none, or another shard's target
    terms_add<kEst>(acc, vs[u], tq[u], tn[u], d2[u], a.c);
  }
  M3D_TPH(4);
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  {
    double v[32];
#pragma unroll
    for (int k = 0; k < 32; ++k) v[k] = k < 30 ? acc[k] : 0.0;
    const double w = wave_transpose_sum32(v, lane);
    if ((lane & 1) == 0) red[lane >> 1][wave] = w;
  }
  M3D_TPH(5);
  __syncthreads();
  M3D_TPH(6);
  if (threadIdx.x < kTermSlots) {
    double v = 0.0;
    if (threadIdx.x < 30)
      for (int w = 0; w < kTermsBlock / kWave; ++w) v += red[threadIdx.x][w];
    double* dst = partials + (int64_t)bx * kTermSlots + threadIdx.x;
    if (kWT)
      __hip_atomic_store(reinterpret_cast<unsigned long long*>(dst), __double_as_longlong(v),
                         __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else
      *dst = v;
  }
  M3D_TPH(7);
#if M3D_TERMS_CLOCK
  {
    const int64_t gw = (int64_t)bx * (kTermsBlock / kWave) + threadIdx.x / kWave;
    if ((threadIdx.x & (kWave - 1)) == 0 && gw < 4096)
      for (int k = 0; k < 8; ++k) g_terms_clock[8 * gw + k] = tph_[k];
  }
#endif
}

#if !M3D_ICP_TERMS_ONLY
template <int kEst>
__global__ __launch_bounds__(kTermsBlock) void terms_kernel(TermsArgs a, const IcpState* __restrict__ s,
                                                            double* __restrict__ partials) {
  if (s->done) return;
  terms_block<false, kEst>(a, s, partials, blockIdx.x);
}

// Target-sharded evaluation, step 1 (m3d_icp_shard_nn): this shard's fp64 winner of every query
// (winner_fp64 over the shard's targets) → lidx / ld64 and the exchange key dkey = bits(d64)
// (INT64_MAX none; d64 ≥ +0, so the integer MIN over ranks is the fp64 minimum).
__global__ __launch_bounds__(256) void shard_winner_kernel(
    const double* __restrict__ pcd64, const float4* __restrict__ src32, int64_t ns,
    const double* __restrict__ tgt64, int64_t nt_shard, int64_t off, GridDev g,
    const IcpState* __restrict__ s, const int64_t* __restrict__ keys,
    const uint32_t* __restrict__ near2, int32_t* __restrict__ lidx, int64_t* __restrict__ ld64,
    int64_t* __restrict__ dkey, int64_t q0) {
  if (s->done) return;
  const int64_t i0 = q0 + (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool valid = i0 < ns;
  const int64_t i = valid ? i0 : 0;
  // a query with no candidate on this shard (kKeyNone: e.g. every query whose box missed a spatial
  // shard's grid) has no winner here and is never ambiguous: its fp64 point and fp32 source are
  // not read (at 1M sources on one of 8 slabs, ~7/8 of the queries)
  const uint64_t k1 = valid ? (uint64_t)keys[i] : (uint64_t)kKeyNone;
  const bool need = k1 != (uint64_t)kKeyNone;
  double Q[3] = {0.0, 0.0, 0.0};
  if (need) q64_of(s->dT, pcd64 + 3 * i, Q);
  const float4 p32 = need ? src32[i] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  int64_t gj;
  double d;
  winner_fp64(valid, k1, need ? __uint_as_float(near2[i]) : kInf, s, g, tgt64, off, nt_shard, p32, Q, gj, d);
  if (!valid) return;
  const int64_t k = gj >= 0 ? __double_as_longlong(d) : kKeyNone;
  lidx[i] = (int32_t)gj;
  ld64[i] = k;
  dkey[i] = k;
}

// Step 2 (m3d_icp_shard_claim): after MIN(dkey) over ranks, the ranks whose own winner has the
// global minimum d64 claim it with their target index; MIN(claim) over ranks then breaks exact
// fp64 ties between shards by the lowest index (the lexicographic (d64, index) minimum).
__global__ __launch_bounds__(256) void shard_claim_kernel(int64_t ns, const IcpState* __restrict__ s,
                                                          const int32_t* __restrict__ lidx,
                                                          const int64_t* __restrict__ ld64,
                                                          const int64_t* __restrict__ dmin,
                                                          int32_t* __restrict__ claim) {
  if (s->done) return;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= ns) return;
  claim[i] = (lidx[i] >= 0 && ld64[i] == dmin[i]) ? lidx[i] : 0x7FFFFFFF;
}

// ------------------------------------------------------------------------------- reduce
// Order of summation of every pass over a loop's source slots (the ICP terms, eval.hip, gicp.hip).
// It is fixed, so two runs — and the brute-force and grid scans, which leave the same winners on
// the same Morton slots — give the same bits (tests/test_gpu_sum_order.py restates it in numpy):
// a block holds consecutive slots and writes one row of partials (eval.hip, gicp.hip: 256 slots,
// nnkey.h block_partial — each wave adds its 64 lanes in an xor butterfly 32, 16, …, 1, the block
// adds its four wave sums in wave order; the ICP terms: terms_block); then reduce_kernel, one
// block of 32 groups × kSlots columns: group g adds rows g, g + 32, … in increasing order
// (independent loads in flight), and the 32 group sums are added in group order.  No
// floating-point atomics.
// s: a loop state whose `done` skips the kernel, or null.  hcnt: the grid scan's deferral header
// (m3d_icp::hcnt), or null; given, the LAST TWO words of sums are overwritten with its count and
// its fault word, so that a one-evaluation call reads its result and the fault word together
// (those columns of the partials are padding: zeros).
constexpr int kReduceGroups = 32;
template <int kSlots>
__device__ __forceinline__ double group_sum(const double* __restrict__ partials, int64_t nblocks,
                                            int g, int slot) {
  double v = 0.0;
#pragma unroll 4
  for (int64_t b = g; b < nblocks; b += kReduceGroups) v += partials[b * kSlots + slot];
  return v;
}

template <int kSlots>
__global__ __launch_bounds__(kReduceGroups * kSlots) void reduce_kernel(
    const double* __restrict__ partials, int64_t nblocks, double* __restrict__ sums,
    const IcpState* __restrict__ s, const uint32_t* __restrict__ hcnt) {
  if (s != nullptr && s->done) return;
  __shared__ double red[kReduceGroups][kSlots];
  const int slot = threadIdx.x & (kSlots - 1);
  const int g = threadIdx.x / kSlots;
  red[g][slot] = group_sum<kSlots>(partials, nblocks, g, slot);
  __syncthreads();
  if (threadIdx.x < kSlots) {
    double t = 0.0;
    for (int k = 0; k < kReduceGroups; ++k) t += red[k][threadIdx.x];
    if (hcnt != nullptr && threadIdx.x == kSlots - 2) t = (double)hcnt[0];
    if (hcnt != nullptr && threadIdx.x == kSlots - 1) t = (double)hcnt[kDeferFault];
    sums[threadIdx.x] = t;
  }
}

// ------------------------------------------------------------------------------- solve
struct SolveParams {
  double rel_fit, rel_rmse;
  int max_iter, est;
  int64_t ns;
  double c[3];  // centre used by point-to-point sums
  FrameParams f;
};

// The state fields the solve reads, loaded by solve_in — in the fused tail before the partial
// sums, so that their global round trip overlaps the reduction's.
struct SolveIn {
  int32_t evals, iters;
  double prev_fit, prev_rmse, r2;
  float eq;
  double T[16];
  float rt[12];
};

__device__ __forceinline__ void solve_in(const IcpState* s, SolveIn& in) {
  in.evals = s->evals;
  in.iters = s->iters;
  in.prev_fit = s->prev_fitness;
  in.prev_rmse = s->prev_rmse;
  in.r2 = s->r2;
  in.eq = s->eq;
#pragma unroll
  for (int k = 0; k < 16; ++k) in.T[k] = s->T[k];
#pragma unroll
  for (int k = 0; k < 12; ++k) in.rt[k] = s->Rt32[k];
}

#if M3D_TAIL_CLOCK
#define M3D_TCLK(k)                                                                   \
  do {                                                                                \
    if (threadIdx.x == 0)                                                             \
      g_tail_clock[(k) < 8 ? 2 * 4096 + (k) : 3 * 4096 + (k)] = __builtin_amdgcn_s_memrealtime(); \
  } while (0)
#else
#define M3D_TCLK(k) \
  do {              \
  } while (0)
#endif
template <int kEst>
__device__ void solve_state(const double* sums, IcpState* s, const SolveParams& sp, const SolveIn& in) {
  double sm[30];
#pragma unroll
  for (int k = 0; k < 30; ++k) sm[k] = sums[k];
  const int32_t evals = in.evals, iters = in.iters;
  const double prev_fit = in.prev_fit, prev_rmse = in.prev_rmse, r2 = in.r2;
  const float eq = in.eq;
  double T[16];
  float rt[12];
#pragma unroll
  for (int k = 0; k < 16; ++k) T[k] = in.T[k];
#pragma unroll
  for (int k = 0; k < 12; ++k) rt[k] = in.rt[k];
  const double count = sm[28];
  const double r = sqrt(in.r2);  // for refresh_rt32_from; independent of everything below
  // point-to-plane: the unpivoted LDLT of JᵀJ does not depend on the convergence test, so it is
  // written first, in the same basic block as fitness / rmse, for the scheduler to interleave the
  // chains (measured neutral against filling A / b after the test, docs/EXPERIMENTS.md §R6; the
  // same bits);
  // its result is used only if the loop goes on
  double A[36], b[6], x[6];
  bool spd_ok = false;
  if (kEst == M3D_EST_POINT_TO_PLANE) {
    int k = 0;
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
      for (int c = a; c < 6; ++c) {
        A[a * 6 + c] = sm[k];
        A[c * 6 + a] = sm[k];
        ++k;
      }
#pragma unroll
    for (int a = 0; a < 6; ++a) b[a] = -sm[21 + a];
    spd_ok = ldlt6_solve_spd(A, b, x);  // straight-line; x garbage (unused) when it fails
  }
  const double fit = count > 0.0 ? count / (double)sp.ns : 0.0;
  const double rmse = count > 0.0 ? sqrt(sm[29] / count) : 0.0;
  M3D_TCLK(10);
  bool stop = false;
  if (evals > 0 && fabs(prev_fit - fit) < sp.rel_fit && fabs(prev_rmse - rmse) < sp.rel_rmse) {
    s->converged = 1;
    stop = true;
  } else if (iters >= sp.max_iter) {
    stop = true;
  }
  s->fitness = fit;
  s->rmse = rmse;
  s->count = (int64_t)count;
  s->prev_fitness = fit;
  s->prev_rmse = rmse;
  s->evals = evals + 1;
  if (stop) {
    s->done = 1;
    return;
  }
  double upd[16];
  for (int k = 0; k < 16; ++k) upd[k] = (k % 5 == 0) ? 1.0 : 0.0;
  // the search transform of the evaluation just reduced: seed_key's bound for the next one
#pragma unroll
  for (int k = 0; k < 12; ++k) s->Rt32_prev[k] = rt[k];
  s->eq_prev = eq;
  s->bound_ok = sp.f.shared;  // bounds compare keys across ranks: only in a shared frame
  M3D_TCLK(11);
  if (count > 0.0) {
    if (kEst == M3D_EST_POINT_TO_PLANE) {
      M3D_TCLK(3);
      // a full-rank JᵀJ unpivoted (no scalar-unit row swaps: 1.6 µs of the tail); a
      // (near-)singular one through Eigen's pivot order, which decides its zero components
      if (!spd_ok) ldlt6_solve(A, b, x);
      M3D_TCLK(4);
      vec6_to_matrix_wave(x, upd);
      M3D_TCLK(5);
    } else {
      const double n = count;
      double mp[3], mq[3], Hm[9], R[9];
      for (int a = 0; a < 3; ++a) {
        mp[a] = sm[a] / n;
        mq[a] = sm[3 + a] / n;
      }
      for (int a = 0; a < 3; ++a)
        for (int c = 0; c < 3; ++c) Hm[3 * a + c] = sm[6 + 3 * a + c] / n - mp[a] * mq[c];
      rotation_from_cov(Hm, R);
      for (int a = 0; a < 3; ++a) {
        const double mpw[3] = {mp[0] + sp.c[0], mp[1] + sp.c[1], mp[2] + sp.c[2]};
        for (int c = 0; c < 3; ++c) upd[4 * a + c] = R[3 * a + c];
        upd[4 * a + 3] = (mq[a] + sp.c[a]) - (R[3 * a] * mpw[0] + R[3 * a + 1] * mpw[1] + R[3 * a + 2] * mpw[2]);
      }
    }
  }
  bool finite = true;
  for (int k = 0; k < 16; ++k) finite = finite && isfinite(upd[k]);
  if (!finite)
    for (int k = 0; k < 16; ++k) upd[k] = (k % 5 == 0) ? 1.0 : 0.0;
  // T ← ΔT·T and the points ← ΔT·points (applied by the next evaluation's query, IcpState::dT)
#pragma unroll
  for (int k = 0; k < 16; ++k) s->dT[k] = s->last_upd[k] = upd[k];
  // both are affine (bottom row 0 0 0 1): the 12 products that are not 0 or 1 (the same sums as
  // matmul4 without its exact-zero terms)
  matmul4_affine(upd, T, T);
#pragma unroll
  for (int k = 0; k < 16; ++k) s->T[k] = T[k];
  s->iters = iters + 1;
  M3D_TCLK(6);
  refresh_rt32_from(s, T, r2, r, sp.f, iters + 1);
  M3D_TCLK(7);
}

template <int kEst>
__global__ void solve_kernel(const double* __restrict__ sums, IcpState* __restrict__ s,
                             SolveParams sp) {
  if (threadIdx.x >= kWave || s->done) return;
  SolveIn in;
  solve_in(s, in);
  solve_state<kEst>(sums, s, sp, in);
}

// Past 256 partials (the separate tail of a large source, 1M: 1,954 rows) the same order on 32
// blocks instead of one: block g adds group g (blocks g, g + 32, …; 32 loads in flight per batch),
// stores the group sum write-through into partials row g (a row only this block reads), drains it
// and takes the ticket; the last block adds rows 0..31 in group order with sc1 loads — the same
// sums, bit for bit, as reduce_kernel — and, for a single-device step (do_solve), runs the solve
// on them (solve_kernel's work without its launch).
template <int kEst>
__global__ __launch_bounds__(kTermSlots) void reduce_groups_kernel(double* __restrict__ partials,
                                                                   int64_t nblocks, double* __restrict__ sums,
                                                                   IcpState* __restrict__ s, SolveParams sp,
                                                                   int do_solve) {
  if (s->done) return;
  const int g = blockIdx.x, slot = threadIdx.x;
  double v = 0.0;
  for (int64_t b0 = g; b0 < nblocks; b0 += (int64_t)kReduceGroups * 32) {
    double t[32];
#pragma unroll
    for (int k = 0; k < 32; ++k) {
      const int64_t b = b0 + (int64_t)k * kReduceGroups;
      t[k] = b < nblocks ? partials[b * kTermSlots + slot] : 0.0;
    }
#pragma unroll
    for (int k = 0; k < 32; ++k)
      if (b0 + (int64_t)k * kReduceGroups < nblocks) v += t[k];
  }
  __hip_atomic_store(reinterpret_cast<unsigned long long*>(partials + (int64_t)g * kTermSlots + slot),
                     __double_as_longlong(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __shared__ int last;
  __syncthreads();
  if (slot == 0)
    last = __hip_atomic_fetch_add(&s->ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ==
           (uint32_t)(kReduceGroups - 1);
  __syncthreads();
  if (!last) return;
  SolveIn in;
  if (do_solve) solve_in(s, in);  // its loads overlap the group rows'
  double tot = 0.0;
  for (int k = 0; k < kReduceGroups; ++k)
    tot += __longlong_as_double(__hip_atomic_load(
        reinterpret_cast<unsigned long long*>(partials + (int64_t)k * kTermSlots + slot), __ATOMIC_RELAXED,
        __HIP_MEMORY_SCOPE_AGENT));
  sums[slot] = tot;
  __shared__ double out[kTermSlots];
  out[slot] = tot;
  __syncthreads();
  if (slot == 0) s->ticket = 0;
  if (do_solve) solve_state<kEst>(out, s, sp, in);
}

// The brute-force NN's slice plan for the next evaluation (nn_plan.h), by ONE wave: wave 1 of the
// fused tail's last block, which otherwise idles while wave 0 runs solve_state.  A lane holds the
// counts of query blocks lane, lane + 64, … (kPlanMaxQ / 64 of them), loaded by plan_in before the
// partial sums as SolveIn is; plan_wave zeroes the counters (the reader does), keeps the counts it
// read in `seen`, bisects τ with a wave sum per probe and writes the table in the uniform launch's
// order — slice y of every query block that has one, by ballot ranks — then the empty entries and
// the flag.  A forced plan (plan_ok = 2) keeps its table.  No block waits for it: the next NN
// launch reads table and flag after this kernel ends.
constexpr int kPlanPer = kPlanMaxQ / kWave;
struct PlanIn {
  uint32_t t[kPlanPer];
  int32_t flag;
};
__device__ __forceinline__ void plan_in(const PlanArgs& pa, const IcpState* s, int lane, PlanIn& in) {
  in.flag = __hip_atomic_load(&s->plan_ok, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
  for (int k = 0; k < kPlanPer; ++k) {
    // branch-free (a clamped index, selected after): under a per-lane branch every load would be
    // waited for inside its own branch, eight round trips one after the other
    const int x = k * kWave + lane;
    in.t[k] = __hip_atomic_load(&pa.cnt[min(x, pa.n - 1)], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
#pragma unroll
  for (int k = 0; k < kPlanPer; ++k) in.t[k] = k * kWave + lane < pa.n ? min(in.t[k], kPlanTmax) : 0u;
}
// sum / max of v over the wave's 64 lanes (all active), wave-uniform: DPP inside each row of 16
// lanes, then the four rows by v_readlane — no LDS round trips (a probe of the bisection is
// one of these)
template <bool kMax>
__device__ __forceinline__ uint32_t plan_wave_red(uint32_t v) {
  const auto op = [](uint32_t a, uint32_t b) { return kMax ? max(a, b) : a + b; };
#pragma unroll
  for (int o = 1; o < 16; o <<= 1) v = op(v, (uint32_t)xor_lane((int)v, o, kWave));
  const auto rl = [&](int l) { return (uint32_t)__builtin_amdgcn_readlane((int)v, l); };
  return op(op(rl(0), rl(16)), op(rl(32), rl(48)));
}
__device__ void plan_wave(const PlanArgs& pa, IcpState* s, int lane, const PlanIn& in) {
  uint32_t tmax = 0, tsum = 0;
#pragma unroll
  for (int k = 0; k < kPlanPer; ++k) {
    const int x = k * kWave + lane;
    if (x < pa.n) {
      pa.cnt[x] = 0u;
      pa.seen[x] = in.t[k];
    }
    tmax = max(tmax, in.t[k]);
    tsum += in.t[k];
  }
  if (in.flag == 2) return;
  tmax = plan_wave_red<true>(tmax);
  tsum = plan_wave_red<false>(tsum);
  const uint32_t cap = (uint32_t)pa.cap;
  const uint32_t tau = plan_tau(tmax, tsum, (uint32_t)pa.n, (uint32_t)pa.budget, [&](uint32_t m) {
    uint32_t a = 0;
#pragma unroll
    for (int k = 0; k < kPlanPer; ++k)
      if (k * kWave < pa.n)  // (wave-uniform: the chunks past n cost nothing)
        a += k * kWave + lane < pa.n ? plan_slices(in.t[k], m, cap) : 0u;
    return plan_wave_red<false>(a);
  });
  uint32_t S[kPlanPer];
#pragma unroll
  for (int k = 0; k < kPlanPer; ++k) S[k] = k * kWave + lane < pa.n ? plan_slices(in.t[k], tau, cap) : 0u;
  int pos = 0;
  for (uint32_t y = 0; y < cap; ++y) {
    const int pos0 = pos;
#pragma unroll
    for (int k = 0; k < kPlanPer; ++k) {
      if (k * kWave >= pa.n) break;
      const bool has = S[k] > y;
      const uint64_t m = __ballot(has);
      const int at = pos + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
      if (has && at < pa.budget) pa.table[at] = plan_entry((uint32_t)(k * kWave + lane), y, S[k]);
      pos += __builtin_popcountll(m);
    }
    if (pos == pos0) break;  // no query block has a slice y
  }
  for (int i = pos + lane; i < pa.budget; i += kWave) pa.table[i] = kPlanEmpty;
  if (lane == 0) s->plan_ok = 1;
}

// Fused single-device iteration tail: terms → block partial → the last block to finish (ticket)
// reduces all partials in reduce_kernel's exact order and runs solve_state.  Cross-XCD hand-off
// (MI355X_MICROARCH.md, visibility table, "last adder" row): each block stores its partial
// write-through (sc1), drains it (vmcnt(0)) and one lane adds to the agent-scope ticket; the
// block whose add returned nblocks − 1 reads every partial with sc1 loads.  No L2 write-back or
// invalidate fences are needed.
// kPlanner: with the NN slice planner in wave 1 of the last block (loops whose NN launch takes a plan);
// false: without it, the kernel of every other loop — grid NN, the 1M source — as it was (PlanNone
// is empty).
struct PlanNone {
  static constexpr int32_t n = 0;
};
// What one block does once every partial is in memory: the fixed-order reduce into `sums`, then
// wave 0 solves (do_solve) while wave 1 plans (kPlanner) — what terms_solve_kernel's last block
// runs behind its ticket (the same text there), as a function for reduce_solve_kernel, whose
// partials come from the NN kernel before it (nn_brute.hip nn_mfma_terms_kernel).
template <int kEst, bool kPlanner, class Plan>
__device__ __forceinline__ void reduce_solve_block(IcpState* s, double* partials, int64_t nblocks,
                                                   double* __restrict__ sums, const SolveParams& sp, int do_solve,
                                                   const Plan& pa) {
  __shared__ double red[kReduceGroups][kTermSlots];
  M3D_TCLK(0);
  SolveIn in;
  if (do_solve && threadIdx.x < kWave) solve_in(s, in);
  // wave 1: the NN slice planner's counts (plan_wave below), in flight with the partials as well
  const bool planner = kPlanner && pa.n > 0 && threadIdx.x >= kWave && threadIdx.x < 2 * kWave;
  PlanIn pin;
  if constexpr (kPlanner)
    if (planner) plan_in(pa, s, threadIdx.x - kWave, pin);
  // every load of the other blocks' partials is an sc1 load (L2-coherent, bypasses L1)
  const int slot = threadIdx.x & (kTermSlots - 1);
  constexpr int kG = kReduceGroups / (kTermsBlock / kTermSlots);  // groups per thread
  double gv[kG];
#pragma unroll
  for (int u = 0; u < kG; ++u) gv[u] = 0.0;
  const int g0 = threadIdx.x / kTermSlots;
  constexpr int kR = 8;  // rounds of kReduceGroups blocks in flight per batch (kR·kG loads):
                         // 256 blocks (cfg1: 196) in ONE batch of dependent loads
  for (int64_t b0 = 0; b0 < nblocks; b0 += kR * kReduceGroups) {
    double t[kR][kG];
#pragma unroll
    for (int r = 0; r < kR; ++r)
#pragma unroll
      for (int u = 0; u < kG; ++u) {
        const int64_t b = b0 + r * kReduceGroups + g0 + u * (kTermsBlock / kTermSlots);
        t[r][u] = b < nblocks
                      ? __longlong_as_double(__hip_atomic_load(
                            reinterpret_cast<unsigned long long*>(partials + b * kTermSlots + slot),
                            __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
                      : 0.0;
      }
#pragma unroll
    for (int r = 0; r < kR; ++r)
#pragma unroll
      for (int u = 0; u < kG; ++u) gv[u] += t[r][u];
  }
  M3D_TCLK(8);  // thread 0's loads landed and added
#pragma unroll
  for (int u = 0; u < kG; ++u) red[g0 + u * (kTermsBlock / kTermSlots)][slot] = gv[u];
  __syncthreads();
  if (threadIdx.x < kTermSlots) {
    double t = 0.0;
    for (int k = 0; k < kReduceGroups; ++k) t += red[k][threadIdx.x];
    red[0][threadIdx.x] = t;  // row 0 is consumed by this thread only before the overwrite
    sums[threadIdx.x] = t;
  }
  M3D_TCLK(9);
  __syncthreads();
  M3D_TCLK(1);
  if (threadIdx.x < kWave) {
    if (threadIdx.x == 0) s->ticket = 0;
    if (do_solve) solve_state<kEst>(red[0], s, sp, in);
  } else if (planner) {
    if constexpr (kPlanner) plan_wave(pa, s, threadIdx.x - kWave, pin);
  }
  M3D_TCLK(2);
}

template <int kEst, bool kPlanner>
__global__ __launch_bounds__(kTermsBlock) void terms_solve_kernel(
    TermsArgs a, IcpState* s, double* partials, int64_t nblocks, double* __restrict__ sums,
    SolveParams sp, int do_solve, std::conditional_t<kPlanner, PlanArgs, PlanNone> pa) {
  // do_solve = 0: the sharded tail (m3d_icp_shard_terms) — terms + the fixed-order reduce into
  // `sums` in one launch; the caller all-reduces them and runs m3d_icp_solve
  if (s->done) return;
#if M3D_TAIL_CLOCK
  const unsigned long long clk0 = __builtin_amdgcn_s_memrealtime();
#endif
  terms_block<true, kEst>(a, s, partials, blockIdx.x);
#if M3D_TAIL_CLOCK
  {
    const unsigned long long clk1 = __builtin_amdgcn_s_memrealtime();
    const int64_t gw = (int64_t)blockIdx.x * (kTermsBlock / kWave) + threadIdx.x / kWave;
    if ((threadIdx.x & (kWave - 1)) == 0 && gw < 4096) {
      g_tail_clock[2 * gw] = clk0;
      g_tail_clock[2 * gw + 1] = clk1;
    }
  }
#endif
  __shared__ double red[kReduceGroups][kTermSlots];
  __shared__ int last;
  // the partial went out write-through (sc1): drain it, then one lane takes the ticket
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t t =
        __hip_atomic_fetch_add(&s->ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    last = (t == (uint32_t)(nblocks - 1));
  }
  __syncthreads();
  if (!last) return;
  // (reduce_solve_block's text, kept in place: calling it from here re-times this kernel —
  // docs/EXPERIMENTS.md §R29)
  M3D_TCLK(0);
  SolveIn in;
  if (do_solve && threadIdx.x < kWave) solve_in(s, in);
  // wave 1: the NN slice planner's counts (plan_wave below), in flight with the partials as well
  const bool planner = kPlanner && pa.n > 0 && threadIdx.x >= kWave && threadIdx.x < 2 * kWave;
  PlanIn pin;
  if constexpr (kPlanner)
    if (planner) plan_in(pa, s, threadIdx.x - kWave, pin);
  // every load of the other blocks' partials is an sc1 load (L2-coherent, bypasses L1)
  const int slot = threadIdx.x & (kTermSlots - 1);
  constexpr int kG = kReduceGroups / (kTermsBlock / kTermSlots);  // groups per thread
  double gv[kG];
#pragma unroll
  for (int u = 0; u < kG; ++u) gv[u] = 0.0;
  const int g0 = threadIdx.x / kTermSlots;
  constexpr int kR = 8;  // rounds of kReduceGroups blocks in flight per batch (kR·kG loads):
                         // 256 blocks (cfg1: 196) in ONE batch of dependent loads
  for (int64_t b0 = 0; b0 < nblocks; b0 += kR * kReduceGroups) {
    double t[kR][kG];
#pragma unroll
    for (int r = 0; r < kR; ++r)
#pragma unroll
      for (int u = 0; u < kG; ++u) {
        const int64_t b = b0 + r * kReduceGroups + g0 + u * (kTermsBlock / kTermSlots);
        t[r][u] = b < nblocks
                      ? __longlong_as_double(__hip_atomic_load(
                            reinterpret_cast<unsigned long long*>(partials + b * kTermSlots + slot),
                            __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
                      : 0.0;
      }
#pragma unroll
    for (int r = 0; r < kR; ++r)
#pragma unroll
      for (int u = 0; u < kG; ++u) gv[u] += t[r][u];
  }
  M3D_TCLK(8);  // thread 0's loads landed and added
#pragma unroll
  for (int u = 0; u < kG; ++u) red[g0 + u * (kTermsBlock / kTermSlots)][slot] = gv[u];
  __syncthreads();
  if (threadIdx.x < kTermSlots) {
    double t = 0.0;
    for (int k = 0; k < kReduceGroups; ++k) t += red[k][threadIdx.x];
    red[0][threadIdx.x] = t;  // row 0 is consumed by this thread only before the overwrite
    sums[threadIdx.x] = t;
  }
  M3D_TCLK(9);
  __syncthreads();
  M3D_TCLK(1);
  if (threadIdx.x < kWave) {
    if (threadIdx.x == 0) s->ticket = 0;
    if (do_solve) solve_state<kEst>(red[0], s, sp, in);
  } else if (planner) {
    if constexpr (kPlanner) plan_wave(pa, s, threadIdx.x - kWave, pin);
  }
  M3D_TCLK(2);
}

// The tail of an iteration whose terms ran inside the NN kernel (nn_mfma_terms_kernel): one block,
// launched behind it — the kernel boundary is the hand-off, every partial is in memory.
__global__ __launch_bounds__(kTermsBlock) void reduce_solve_kernel(IcpState* s, double* partials, int64_t nblocks,
                                                                   double* __restrict__ sums, SolveParams sp,
                                                                   PlanArgs pa) {
  if (s->done) return;
  reduce_solve_block<M3D_EST_POINT_TO_PLANE, true>(s, partials, nblocks, sums, sp, 1, pa);
}

// finalize standalone NN (m3d_nn1): the fp64 winner (nnkey.h winner_fp64) and its d64
__global__ __launch_bounds__(256) void nn_finalize_kernel(const double* __restrict__ pcd64,
                                                          const float4* __restrict__ src32,
                                                          int64_t ns,
                                                          const double* __restrict__ tgt64,
                                                          int64_t nt, GridDev g,
                                                          const IcpState* __restrict__ s,
                                                          const int64_t* __restrict__ keys,
                                                          const uint32_t* __restrict__ near2,
                                                          const int32_t* __restrict__ slot,
                                                          int32_t* __restrict__ idx,
                                                          double* __restrict__ d2out) {
  const SlotWinner w = slot_winner((int64_t)blockIdx.x * 256 + threadIdx.x, pcd64, src32, ns, tgt64, nt, g, s, keys,
                                   near2);
  if (!w.valid) return;
  const int64_t o = slot != nullptr ? (int64_t)slot[w.i] : w.i;  // slot → the caller's source order
  idx[o] = (int32_t)w.gj;
  if (d2out != nullptr) d2out[o] = w.gj >= 0 ? w.d : INFINITY;
}

// An order change by a slot table: dst[slot[k]] = v[k] (slot order → the caller's order), or with
// kGather dst[k] = v[slot[k]] (the caller's order → slot order)
template <typename V, bool kGather>
__global__ void permute_kernel(const V* __restrict__ v, const int32_t* __restrict__ slot, int64_t n,
                               V* __restrict__ dst) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= n) return;
  if (kGather)
    dst[k] = v[slot[k]];
  else
    dst[slot[k]] = v[k];
}

// ------------------------------------------------------------------------------- pairs
// The correspondence set (Open3D RegistrationResult.correspondence_set): (i, v[i]) for every i
// with v[i] ≥ 0, in increasing i.  An order-preserving compaction in three launches over chunks
// of 1024 entries (256 threads × 4, entry base + u·256 + t): per-chunk counts, one block's
// exclusive scan of the counts, placement (per-wave ballots, LDS prefix over the chunk's 16
// (u, wave) groups in index order).
constexpr int kPairChunk = 1024;

__global__ __launch_bounds__(256) void pair_count_kernel(const int32_t* __restrict__ v, int64_t n,
                                                         int32_t* __restrict__ cnt) {
  __shared__ int part[4];
  const int64_t base = (int64_t)blockIdx.x * kPairChunk;
  int c = 0;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int64_t i = base + u * 256 + threadIdx.x;
    c += __popcll(__ballot(i < n && v[i] >= 0));
  }
  if ((threadIdx.x & (kWave - 1)) == 0) part[threadIdx.x / kWave] = c;
  __syncthreads();
  if (threadIdx.x == 0) cnt[blockIdx.x] = part[0] + part[1] + part[2] + part[3];
}

// one block: cnt[0..nb) → exclusive offsets in place, the total in cnt[nb]
__global__ __launch_bounds__(1024) void pair_scan_kernel(int32_t* __restrict__ cnt, int64_t nb) {
  __shared__ int32_t wsum[16];
  __shared__ int32_t carry_s;
  const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave;
  if (threadIdx.x == 0) carry_s = 0;
  __syncthreads();
  for (int64_t b0 = 0; b0 < nb; b0 += 1024) {
    const int64_t b = b0 + threadIdx.x;
    const int32_t x = b < nb ? cnt[b] : 0;
    int32_t incl = x;  // inclusive wave scan
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
      const int32_t y = __shfl_up(incl, o, kWave);
      if (lane >= o) incl += y;
    }
    if (lane == kWave - 1) wsum[w] = incl;
    __syncthreads();
    int32_t before = carry_s;
    for (int k = 0; k < w; ++k) before += wsum[k];
    if (b < nb) cnt[b] = before + incl - x;
    __syncthreads();
    if (threadIdx.x == 1023) carry_s = before + incl;
    __syncthreads();
  }
  if (threadIdx.x == 0) cnt[nb] = carry_s;
}

__global__ __launch_bounds__(256) void pair_place_kernel(const int32_t* __restrict__ v, int64_t n,
                                                         const int32_t* __restrict__ off,
                                                         int32_t* __restrict__ pairs) {
  __shared__ int grp[16];  // popcount of group (u, wave), index order u·4 + wave
  const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave;
  const int64_t base = (int64_t)blockIdx.x * kPairChunk;
  bool hit[4];
  int32_t val[4];
  uint64_t m[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int64_t i = base + u * 256 + threadIdx.x;
    val[u] = i < n ? v[i] : -1;
    hit[u] = val[u] >= 0;
    m[u] = __ballot(hit[u]);
    if (lane == 0) grp[u * 4 + w] = __popcll(m[u]);
  }
  __syncthreads();
  const uint64_t below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
  int32_t o = off[blockIdx.x];  // entries of the chunk's rows before row u
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    int32_t before = o;
    for (int k = 0; k < w; ++k) before += grp[u * 4 + k];
    if (hit[u]) {
      const int32_t k = before + __popcll(m[u] & below);
      pairs[2 * (int64_t)k] = (int32_t)(base + u * 256 + threadIdx.x);
      pairs[2 * (int64_t)k + 1] = val[u];
    }
    for (int k = 0; k < 4; ++k) o += grp[u * 4 + k];
  }
}

__global__ void keys_to_idx_kernel(const int64_t* __restrict__ keys, int64_t n,
                                   int32_t* __restrict__ idx) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) idx[i] = keys[i] == kKeyNone ? -1 : (int32_t)(uint32_t)keys[i];
}

// ------------------------------------------------------------------------------- launchers
static FrameParams frame_of(const m3d_icp* s) {
  FrameParams f;
  for (int k = 0; k < 3; ++k) {
    f.cs[k] = s->src->center[k];
    f.ct[k] = s->tgt->center[k];
  }
  f.pinf = s->src->rmax;
  f.qinf = s->tgt->rmax;
  f.s16 = s->tgt->s16;
  f.shared = s->tgt->center_given;
  return f;
}

static SolveParams solve_params(const m3d_icp* s) {
  SolveParams sp;
  sp.rel_fit = s->params.relative_fitness;
  sp.rel_rmse = s->params.relative_rmse;
  sp.max_iter = s->params.max_iteration;
  sp.est = s->params.estimation;
  sp.ns = s->ns_total > 0 ? s->ns_total : s->src->n;
  for (int k = 0; k < 3; ++k) sp.c[k] = s->src->center[k];
  sp.f = frame_of(s);
  return sp;
}

// f(std::integral_constant<int, E>) for the estimator E = est: a launcher writes the launch of a
// kEst kernel once
template <typename F>
static void with_est(int est, F f) {
  if (est == M3D_EST_POINT_TO_PLANE)
    f(std::integral_constant<int, M3D_EST_POINT_TO_PLANE>{});
  else
    f(std::integral_constant<int, M3D_EST_POINT_TO_POINT>{});
}

// the loop's fp64 points start as the source itself (the init, if applied, is dT)
static hipError_t reset_points(const m3d_icp* s, hipStream_t st) {
  if (s->src->n == 0) return hipSuccess;
  return hipMemcpyAsync(s->pcd64, s->src->xyz64, sizeof(double) * 3 * s->src->n, hipMemcpyDeviceToDevice, st);
}

// The NN plan's tile counters start a run at zero, like the flag (reset_eval): the run's first plan
// counts the run's own evaluations only.  (Where no planner reads them — GICP, M3D_ICP_FUSED=0 — they
// add up until the next reset; a planner that runs later in the same run reads them clamped at
// kPlanTmax, and sums over evaluations size the slices like one evaluation's counts.)
static hipError_t reset_plan_counts(const m3d_icp* s, hipStream_t st) {
  if (s->nn_cnt == nullptr) return hipSuccess;
  // (and the query blocks' tickets of nn_mfma_terms_kernel, which follow the counts in the arena)
  return hipMemsetAsync(s->nn_cnt, 0, (size_t)s->nn_qblocks * sizeof(uint32_t) * (s->nn_tix != nullptr ? 2 : 1), st);
}

hipError_t launch_icp_state_init(IcpState* state, const double* T, bool apply_init, double r2, const FrameParams& f,
                                 hipStream_t st) {
  icp_init_kernel<<<1, 64, 0, st>>>(state, T[0], T[1], T[2], T[3], T[4], T[5], T[6], T[7], T[8], T[9], T[10], T[11],
                                    r2, f, apply_init ? 1 : 0);
  return hipGetLastError();
}

hipError_t launch_icp_reset(const m3d_icp* s, const double* T, bool apply_init, hipStream_t st) {
  hipError_t e = reset_points(s, st);
  if (e == hipSuccess) e = reset_plan_counts(s, st);
  if (e != hipSuccess) return e;
  return launch_icp_state_init(s->state, T, apply_init, s->max_dist * s->max_dist, frame_of(s), st);
}

hipError_t launch_icp_set_T(const m3d_icp* s, const double* T_dev, hipStream_t st) {
  hipError_t e = reset_points(s, st);
  if (e == hipSuccess) e = reset_plan_counts(s, st);
  if (e != hipSuccess) return e;
  icp_set_T_kernel<<<1, 64, 0, st>>>(s->state, T_dev, s->max_dist * s->max_dist, frame_of(s));
  return hipGetLastError();
}

// m3d_icp_copy_points: the loop's points in the caller's order.  Before the first evaluation the
// init is still in dT (pcd64 = the source): apply it as the evaluation will (q64_of, Eigen's
// order) — RegistrationICP's pcd at that point is init·source — unless dT is exactly I
// (init isIdentity(): Open3D leaves pcd untouched, and I·p could turn a −0 into +0).
// moved: the host enqueued a terms pass since the reset (m3d_icp::points_moved) — that pass wrote
// dT·pcd64 back, and until its solve runs evals is still 0 (the shard protocol's terms → all-reduce
// → solve): the points are pcd64 as it stands.
__global__ void copy_points_kernel(const IcpState* __restrict__ s, const double* __restrict__ v,
                                   const int32_t* __restrict__ slot, int64_t n, double* __restrict__ dst,
                                   int moved) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= n) return;
  const int64_t o = (int64_t)slot[k];
  bool apply = s->evals == 0 && !moved;
  if (apply) {
    bool eye = true;
    for (int e = 0; e < 16; ++e) eye = eye && s->dT[e] == ((e % 5) == 0 ? 1.0 : 0.0);
    apply = !eye;
  }
  if (apply) {
    double q[3];
    q64_of(s->dT, v + 3 * k, q);
    for (int c = 0; c < 3; ++c) dst[3 * o + c] = q[c];
  } else {
    for (int c = 0; c < 3; ++c) dst[3 * o + c] = v[3 * k + c];
  }
}

hipError_t launch_copy_points(const m3d_icp* s, double* dst, hipStream_t st) {
  const int64_t n = s->src->n;
  if (n == 0) return hipSuccess;
  copy_points_kernel<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(s->state, s->pcd64, s->src->slot, n, dst,
                                                                  s->points_moved ? 1 : 0);
  return hipGetLastError();
}

hipError_t launch_val_states(const m3d_icp* s, const double* T_dev, const int32_t* list, int64_t n,
                             IcpState* states, hipStream_t st) {
  if (n == 0) return hipSuccess;
  val_states_kernel<<<(unsigned)((n + 63) / 64), 64, 0, st>>>(states, T_dev, list, n,
                                                              s->max_dist * s->max_dist, frame_of(s));
  return hipGetLastError();
}

hipError_t launch_icp_keyinit(const m3d_icp* s, int64_t off, hipStream_t st, int64_t q0, int64_t q1) {
  const int64_t ns = q1 < 0 ? s->src->n : q1;
  if (ns <= q0) return hipSuccess;
  keyinit_kernel<<<(unsigned)((ns - q0 + 255) / 256), 256, 0, st>>>(
      s->src->xyz32, ns, s->tgt->xyz32, s->tgt->n, off, s->state, s->corr, s->dprev, s->keys,
      s->near2, q0);
  return hipGetLastError();
}


// 64-B target record: fp64 point, fp64 normal, and in the last 16 bytes the centred fp32 point
// (xyz32's bits: what the scan's seed gather read), which the fused tail copies into the seed
// records; every other reader takes the first 48 bytes only
__global__ __launch_bounds__(256) void pack_rec_kernel(const double* __restrict__ xyz,
                                                       const double* __restrict__ nrm,
                                                       const float4* __restrict__ xyz32, int64_t n,
                                                       double* __restrict__ rec) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double r[8];
  for (int k = 0; k < 3; ++k) {
    r[k] = xyz[3 * i + k];
    r[3 + k] = nrm != nullptr ? nrm[3 * i + k] : 0.0;
  }
  const float4 p = xyz32[i];
  r[6] = __hiloint2double(__float_as_int(p.y), __float_as_int(p.x));
  r[7] = __hiloint2double(__float_as_int(p.w), __float_as_int(p.z));
  for (int k = 0; k < 8; ++k) rec[8 * i + k] = r[k];
}

hipError_t ensure_target_rec(const m3d_cloud* c, hipStream_t st) {
  if (c->rec64 != nullptr || c->n == 0) return hipSuccess;
  double* rec = nullptr;
  hipError_t e = block_alloc(reinterpret_cast<void**>(&rec), sizeof(double) * 8 * c->n, st);
  if (e != hipSuccess) return e;
  pack_rec_kernel<<<(unsigned)((c->n + 255) / 256), 256, 0, st>>>(c->xyz64, c->nrm64, c->xyz32, c->n, rec);
  e = hipGetLastError();  // asynchronous (stream order); m3d_icp_create synchronises once
  if (e != hipSuccess) {
    block_release(rec);
    return e;
  }
  c->rec64 = rec;
  return hipSuccess;
}

// The target grid's points in fp64, in the grid's cell order (w = index bits): resolve_wave then
// reads an ambiguous query's box candidates with their fp64 coordinates in one load instead of the
// fp32 point and then a gather of the fp64 one
__global__ __launch_bounds__(256) void pack_pts64_kernel(const float4* __restrict__ pts,
                                                         const double* __restrict__ xyz, int64_t n,
                                                         double4* __restrict__ out) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= n) return;
  const int32_t j = __float_as_int(pts[k].w);
  out[k] = make_double4(xyz[3 * (int64_t)j], xyz[3 * (int64_t)j + 1], xyz[3 * (int64_t)j + 2],
                        __longlong_as_double((long long)j));
}

hipError_t build_grid_pts64(const m3d_cloud* c, Grid* g, hipStream_t st) {
  if (g->pts64 != nullptr || g->n_pts == 0) return hipSuccess;
  double4* p = nullptr;
  hipError_t e = block_alloc(reinterpret_cast<void**>(&p), sizeof(double4) * g->n_pts, st);
  if (e != hipSuccess) return e;
  pack_pts64_kernel<<<(unsigned)((g->n_pts + 255) / 256), 256, 0, st>>>(g->pts, c->xyz64, g->n_pts, p);
  e = hipGetLastError();  // asynchronous (stream order); m3d_icp_create synchronises once
  if (e != hipSuccess) {
    block_release(p);
    return e;
  }
  g->pts64 = p;
  g->dev.pts64 = p;
  return hipSuccess;
}

static TermsArgs terms_args(const m3d_icp* s, int64_t off, const int32_t* claim,
                            const int64_t* dmin, bool reset_keys) {
  TermsArgs a;
  a.pcd64 = s->pcd64;
  a.src32 = s->src->xyz32;
  a.ns = s->src->n;
  a.tgt64 = s->tgt->xyz64;
  a.nrm64 = s->tgt->nrm64;
  a.rec64 = s->tgt->rec64;
  a.nt_shard = s->tgt->n;
  a.off = off;
  a.keys = s->keys;
  a.near2 = s->near2;
  a.g = s->tgrid->dev;
  a.claim = claim;
  a.dmin = dmin;
  a.dprev = claim != nullptr ? s->dprev : nullptr;
  a.corr = s->corr;
  a.est = s->params.estimation;
  for (int k = 0; k < 3; ++k) a.c[k] = s->src->center[k];
  a.reset_keys = reset_keys ? s->keys : nullptr;
  // (launch_icp_nn takes the records under the same condition)
  a.seed = reset_keys && claim == nullptr && off == 0 && a.rec64 != nullptr ? s->seed : nullptr;
  return a;
}

hipError_t launch_icp_terms_mode(const m3d_icp* s, int64_t off, const int32_t* claim,
                                 const int64_t* dmin, hipStream_t st) {
  const int64_t ns = s->src->n;
  if (ns == 0) return hipMemsetAsync(s->partials, 0, sizeof(double) * kTermSlots, st);
  const TermsArgs ta = terms_args(s, off, claim, dmin, false);
  const unsigned nb = (unsigned)s->nblocks;
  with_est(ta.est, [&](auto e) {
    terms_kernel<decltype(e)::value><<<nb, kTermsBlock, 0, st>>>(ta, s->state, s->partials);
  });
  return hipGetLastError();
}

// reduce_groups_kernel; do_solve = 0: the sums only (the estimator matters to the solve alone: one
// instance serves both)
static void launch_reduce_groups(const m3d_icp* s, double* sums, int do_solve, hipStream_t st) {
  const SolveParams sp = do_solve ? solve_params(s) : SolveParams{};
  with_est(do_solve ? s->params.estimation : M3D_EST_POINT_TO_PLANE, [&](auto e) {
    reduce_groups_kernel<decltype(e)::value><<<kReduceGroups, kTermSlots, 0, st>>>(
        s->partials, s->nblocks, sums, s->state, sp, do_solve);
  });
}

// out[0 .. slots) = the sums of the `rows` rows of `slots` (16 or 32) columns in partials
// (reduce_kernel: rows = 0 gives zeros)
hipError_t launch_reduce(const double* partials, int64_t rows, int slots, double* out, const IcpState* s,
                         const uint32_t* hcnt, hipStream_t st) {
  if (slots == 16)
    reduce_kernel<16><<<1, kReduceGroups * 16, 0, st>>>(partials, rows, out, s, hcnt);
  else if (slots == kTermSlots)
    reduce_kernel<kTermSlots><<<1, kReduceGroups * kTermSlots, 0, st>>>(partials, rows, out, s, hcnt);
  else
    return hipErrorInvalidValue;
  return hipGetLastError();
}

hipError_t launch_icp_reduce(const m3d_icp* s, double* sums, hipStream_t st) {
  if (s->nblocks <= 256) return launch_reduce(s->partials, s->nblocks, kTermSlots, sums, s->state, nullptr, st);
  launch_reduce_groups(s, sums, 0, st);  // group g's first row is block g's: rows 0..31 exist
  return hipGetLastError();
}

// the single-device separate tail after the terms pass: reduce + solve (one launch past 256
// partials, reduce_groups_kernel's last block solving; two below)
hipError_t launch_icp_reduce_solve(const m3d_icp* s, hipStream_t st) {
  if (s->nblocks <= 256) {
    hipError_t e = launch_icp_reduce(s, s->sums, st);
    return e == hipSuccess ? launch_icp_solve(s, s->sums, st) : e;
  }
  launch_reduce_groups(s, s->sums, 1, st);
  return hipGetLastError();
}

// sharded tail: terms (shard offset off; claim/dmin: the target-shard exchange results, or null
// for a source shard) + reduce into sums, one launch
static void launch_terms_solve(const TermsArgs& ta, const m3d_icp* s, double* sums, int do_solve,
                               hipStream_t st) {
  const unsigned nb = (unsigned)s->nblocks;
  const SolveParams sp = solve_params(s);
  const PlanArgs pa = nn_plan_args(s);
  with_est(ta.est, [&](auto e) {
    if (pa.n > 0)
      terms_solve_kernel<decltype(e)::value, true><<<nb, kTermsBlock, 0, st>>>(ta, s->state, s->partials, s->nblocks,
                                                                               sums, sp, do_solve, pa);
    else
      terms_solve_kernel<decltype(e)::value, false><<<nb, kTermsBlock, 0, st>>>(ta, s->state, s->partials, s->nblocks,
                                                                                sums, sp, do_solve, PlanNone{});
  });
}

hipError_t launch_icp_terms_reduce(const m3d_icp* s, int64_t off, const int32_t* claim,
                                   const int64_t* dmin, double* sums, bool reset_keys,
                                   hipStream_t st) {
  const int64_t ns = s->src->n;
  if (ns == 0) {
    hipError_t e = launch_icp_terms_mode(s, off, claim, dmin, st);
    return e == hipSuccess ? launch_icp_reduce(s, sums, st) : e;
  }
  launch_terms_solve(terms_args(s, off, claim, dmin, reset_keys), s, sums, 0, st);
  return hipGetLastError();
}

hipError_t launch_icp_solve_state(IcpState* state, const double* sums, double relative_fitness, double relative_rmse,
                                  int32_t max_iteration, int32_t estimation, int64_t ns, const double* center,
                                  const FrameParams& f, hipStream_t st) {
  SolveParams sp;
  sp.rel_fit = relative_fitness;
  sp.rel_rmse = relative_rmse;
  sp.max_iter = max_iteration;
  sp.est = estimation;
  sp.ns = ns;
  for (int k = 0; k < 3; ++k) sp.c[k] = center[k];
  sp.f = f;
  with_est(sp.est, [&](auto e) { solve_kernel<decltype(e)::value><<<1, 64, 0, st>>>(sums, state, sp); });
  return hipGetLastError();
}

hipError_t launch_icp_solve(const m3d_icp* s, const double* sums, hipStream_t st) {
  const SolveParams sp = solve_params(s);
  return launch_icp_solve_state(s->state, sums, sp.rel_fit, sp.rel_rmse, sp.max_iter, sp.est, sp.ns, sp.c, sp.f, st);
}

hipError_t launch_icp_terms_solve(const m3d_icp* s, bool reset_keys, hipStream_t st) {
  const int64_t ns = s->src->n;
  if (ns == 0) {  // no blocks to take tickets: the unfused tail handles the empty source
    hipError_t e = launch_icp_terms_mode(s, 0, nullptr, nullptr, st);
    if (e == hipSuccess) e = launch_icp_reduce(s, s->sums, st);
    return e == hipSuccess ? launch_icp_solve(s, s->sums, st) : e;
  }
  launch_terms_solve(terms_args(s, 0, nullptr, nullptr, reset_keys), s, s->sums, 1, st);
  return hipGetLastError();
}

// ---- the iteration whose terms pass runs inside the NN kernel (nn_brute.hip nn_mfma_terms_kernel)
__global__ void store_nn_terms_kernel(NnTermsDev v, NnTermsDev* dst) { *dst = v; }

size_t nn_terms_dev_bytes() { return sizeof(NnTermsDev); }

// the loop's NnTermsDev (s->nn_targs), once, at m3d_icp_create
hipError_t launch_nn_terms_setup(const m3d_icp* s, hipStream_t st) {
  NnTermsDev v;
  v.a = terms_args(s, 0, nullptr, nullptr, true);
  v.partials = s->partials;
  v.tix = s->nn_tix;
  store_nn_terms_kernel<<<1, 1, 0, st>>>(v, reinterpret_cast<NnTermsDev*>(s->nn_targs));
  return hipGetLastError();
}

// its tail: one block reduces the partials the NN kernel left, solves and plans
hipError_t launch_icp_reduce_solve_block(const m3d_icp* s, hipStream_t st) {
  reduce_solve_kernel<<<1, kTermsBlock, 0, st>>>(s->state, s->partials, s->nblocks, s->sums, solve_params(s),
                                                 nn_plan_args(s));
  return hipGetLastError();
}

hipError_t launch_nn_finalize(const m3d_icp* s, int32_t* idx, double* d2, hipStream_t st) {
  const int64_t ns = s->src->n;
  if (ns == 0) return hipSuccess;
  nn_finalize_kernel<<<(unsigned)((ns + 255) / 256), 256, 0, st>>>(
      s->pcd64, s->src->xyz32, ns, s->tgt->xyz64, s->tgt->n, s->tgrid->dev, s->state, s->keys,
      s->near2, s->src->slot, idx, d2);
  return hipGetLastError();
}

template <typename V, bool kGather>
static hipError_t launch_permute(const V* v, const int32_t* slot, int64_t n, V* dst, hipStream_t st) {
  if (n == 0) return hipSuccess;
  permute_kernel<V, kGather><<<(unsigned)((n + 255) / 256), 256, 0, st>>>(v, slot, n, dst);
  return hipGetLastError();
}

hipError_t launch_scatter_i32(const int32_t* v, const int32_t* slot, int64_t n, int32_t* dst,
                              hipStream_t st) {
  if (n > 0 && slot == nullptr) return hipMemcpyAsync(dst, v, sizeof(int32_t) * n, hipMemcpyDeviceToDevice, st);
  return launch_permute<int32_t, false>(v, slot, n, dst, st);
}
hipError_t launch_gather_i32(const int32_t* v, const int32_t* slot, int64_t n, int32_t* dst, hipStream_t st) {
  return launch_permute<int32_t, true>(v, slot, n, dst, st);
}
hipError_t launch_scatter_f64(const double* v, const int32_t* slot, int64_t n, double* dst, hipStream_t st) {
  return launch_permute<double, false>(v, slot, n, dst, st);
}

hipError_t launch_corr_pairs(const int32_t* v, int64_t n, int32_t* cnt, int32_t* pairs, hipStream_t st) {
  if (n <= 0) return hipMemsetAsync(cnt, 0, sizeof(int32_t), st);
  const int64_t nb = (n + kPairChunk - 1) / kPairChunk;
  pair_count_kernel<<<(unsigned)nb, 256, 0, st>>>(v, n, cnt);
  pair_scan_kernel<<<1, 1024, 0, st>>>(cnt, nb);
  pair_place_kernel<<<(unsigned)nb, 256, 0, st>>>(v, n, cnt, pairs);
  return hipGetLastError();
}

hipError_t launch_shard_winner(const m3d_icp* s, int64_t off, int64_t* dkey, hipStream_t st,
                               int64_t q0, int64_t q1) {
  const int64_t ns = q1 < 0 ? s->src->n : q1;
  if (ns <= q0) return hipSuccess;
  shard_winner_kernel<<<(unsigned)((ns - q0 + 255) / 256), 256, 0, st>>>(
      s->pcd64, s->src->xyz32, ns, s->tgt->xyz64, s->tgt->n, off, s->tgrid->dev, s->state,
      s->keys, s->near2, s->lidx, s->ld64, dkey, q0);
  return hipGetLastError();
}

hipError_t launch_shard_claim(const m3d_icp* s, const int64_t* dmin, int32_t* claim, hipStream_t st) {
  const int64_t ns = s->src->n;
  if (ns == 0) return hipSuccess;
  shard_claim_kernel<<<(unsigned)((ns + 255) / 256), 256, 0, st>>>(ns, s->state, s->lidx, s->ld64,
                                                                   dmin, claim);
  return hipGetLastError();
}

hipError_t launch_keys_to_idx(const int64_t* keys, int64_t n, int32_t* idx, hipStream_t st) {
  if (n == 0) return hipSuccess;
  keys_to_idx_kernel<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(keys, n, idx);
  return hipGetLastError();
}

int64_t terms_blocks(int64_t ns) { return ns > 0 ? (ns + kTermsBlock - 1) / kTermsBlock : 1; }

#endif  // !M3D_ICP_TERMS_ONLY
}  // namespace m3d

#if M3D_TERMS_CLOCK
extern "C" int m3d_debug_terms_clock(unsigned long long* out, int n) {
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(m3d::g_terms_clock), sizeof(unsigned long long) * (size_t)n) == hipSuccess ? 0 : -1;
}
#endif
#if M3D_TAIL_CLOCK
extern "C" int m3d_debug_tail_clock(unsigned long long* out, int n) {
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(m3d::g_tail_clock), sizeof(unsigned long long) * (size_t)n) == hipSuccess ? 0 : -1;
}
#endif
