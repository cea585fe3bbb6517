// nn_plan.h — the slice plan of the brute-force NN launch: how many blocks S_x
// each 512-query block x of nn_mfma_kernel gets, sized from the target tiles t_x the query block
// kept in the previous evaluation.  The rule, shared by the device planner (icp.hip: wave 1 of
// terms_solve_kernel's last block, and of reduce_solve_kernel), the host entry m3d_debug_nn_plan_host and the launch:
//   S_x(τ) = clamp(⌈t_x / τ⌉, 1, cap),  cap = min(S_max, ntiles),
//   τ = the smallest integer ≥ 1 with Σ_x S_x(τ) ≤ B (the block budget: the resident slots);
// Σ S_x(τ) does not grow with τ and equals n ≤ B at τ = max t_x, so a bisection over [1, max t_x]
// (plan_tau: a tighter upper end) finds it.
// The plan is a function of integers: the host divides in integers, the device takes the same
// quotient from an fp32 reciprocal corrected by an exact fma remainder (plan_slices), so both give
// the same plan (compared on the GPU, tests/test_gpu_nn_plan.py).
// Unweighted: a tile counts one, whichever of its halves the waves sweep, and a block has no fixed
// cost (EXPERIMENTS §R19).
// The table: B entries (x, y, S_x), slice y of query block x takes tiles y, y + S_x, …; in the
// order of the uniform launch — all x of slice 0, then of slice 1, … — so that equal counts give
// exactly the uniform assignment; the rest are kPlanEmpty.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define M3D_PLAN_HD __host__ __device__ inline
#else
#define M3D_PLAN_HD inline
#endif

namespace m3d {

constexpr uint32_t kPlanEmpty = 0xFFFFFFFFu;
constexpr int kPlanSmax = 8;            // S_max: most slices of one query block
constexpr int kPlanMaxQ = 512;          // query blocks the device planner holds (8 per lane)
constexpr uint32_t kPlanTmax = 1u << 20;  // counts are clamped here (exact in fp32)

M3D_PLAN_HD uint32_t plan_entry(uint32_t x, uint32_t y, uint32_t S) { return x | (y << 16) | (S << 24); }
M3D_PLAN_HD uint32_t plan_x(uint32_t e) { return e & 0xFFFFu; }
M3D_PLAN_HD uint32_t plan_y(uint32_t e) { return (e >> 16) & 0xFFu; }
M3D_PLAN_HD uint32_t plan_S(uint32_t e) { return e >> 24; }

M3D_PLAN_HD uint32_t plan_cap(int64_t smax, int64_t ntiles) {
  const int64_t c = smax < ntiles ? smax : ntiles;
  return (uint32_t)(c < 1 ? 1 : (c > 255 ? 255 : c));
}

// S_x(τ); t ≤ kPlanTmax, τ ≥ 1
M3D_PLAN_HD uint32_t plan_slices(uint32_t t, uint32_t tau, uint32_t cap) {
#if defined(__HIP_DEVICE_COMPILE__)
  // ⌈t / τ⌉ without the integer division sequence, in full-rate fp32: both operands and every
  // product here are integers below 2²⁴, so the remainder by fma is exact and corrects the
  // quotient estimate, which is off by at most one either way
  const float af = (float)(t + tau - 1u), tf = (float)tau;
  float qf = __builtin_floorf(af * __builtin_amdgcn_rcpf(tf));
  const float r = __builtin_fmaf(-qf, tf, af);
  qf += r >= tf ? 1.0f : 0.0f;
  qf -= r < 0.0f ? 1.0f : 0.0f;
  const uint32_t q = (uint32_t)qf;
#else
  const uint32_t q = (t + tau - 1u) / tau;
#endif
  return q < 1u ? 1u : (q > cap ? cap : q);
}

// The bisection; sum(τ) = Σ_x S_x(τ) (a loop on the host, a wave reduction on the device).  The
// bracket's upper end: τ = max t_x fits (every S is 1), and so does any τ ≥ Σt / (B − n), since
// S_x(τ) ≤ t_x / τ + 1 — at cfg1 that is two or three probes instead of five.
template <class SumFn>
M3D_PLAN_HD uint32_t plan_tau(uint32_t tmax, uint32_t tsum, uint32_t n, uint32_t budget, SumFn sum) {
  uint32_t lo = 1u, hi = tmax < 1u ? 1u : tmax;
  if (budget > n) {
    const uint32_t by_sum = (tsum + (budget - n) - 1u) / (budget - n);
    hi = by_sum < 1u ? 1u : (by_sum < hi ? by_sum : hi);
  }
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2u;
    if (sum(mid) <= budget) hi = mid;
    else lo = mid + 1u;
  }
  return lo;
}

// Host form of the whole rule: counts t[0 .. n) → S[0 .. n) (may be null) and the table of
// `budget` entries (may be null).  Returns τ, 0 when n > budget (no plan: every S would be < 1).
inline uint32_t plan_host(const uint32_t* t, int64_t n, int64_t budget, int64_t smax, int64_t ntiles,
                          uint32_t* S, uint32_t* table) {
  if (n < 1 || n > budget || n > 0xFFFF || n > 2048) return 0u;  // (Σt fits 32 bits)
  const uint32_t cap = plan_cap(smax, ntiles);
  const auto tc = [&](int64_t x) { return t[x] < kPlanTmax ? t[x] : kPlanTmax; };
  uint32_t tmax = 0, tsum = 0;
  for (int64_t x = 0; x < n; ++x) {
    tmax = tc(x) > tmax ? tc(x) : tmax;
    tsum += tc(x);
  }
  const uint32_t tau = plan_tau(tmax, tsum, (uint32_t)n, (uint32_t)budget, [&](uint32_t m) {
    uint32_t a = 0;
    for (int64_t x = 0; x < n; ++x) a += plan_slices(tc(x), m, cap);
    return a;
  });
  int64_t pos = 0;
  for (uint32_t y = 0; y < cap; ++y)
    for (int64_t x = 0; x < n; ++x) {
      const uint32_t Sx = plan_slices(tc(x), tau, cap);
      if (y == 0 && S != nullptr) S[x] = Sx;
      if (Sx > y && table != nullptr) table[pos++] = plan_entry((uint32_t)x, y, Sx);
    }
  if (table != nullptr)
    for (; pos < budget; ++pos) table[pos] = kPlanEmpty;
  return tau;
}

// The table of a given S[0 .. n) (the forced plan of m3d_debug_icp_nn_plan), same order
inline void plan_table_of(const uint32_t* S, int64_t n, int64_t budget, uint32_t* table) {
  int64_t pos = 0;
  for (uint32_t y = 0; y < 255u; ++y)
    for (int64_t x = 0; x < n; ++x)
      if (S[x] > y && pos < budget) table[pos++] = plan_entry((uint32_t)x, y, S[x]);
  for (; pos < budget; ++pos) table[pos] = kPlanEmpty;
}

// kernel view of a loop's plan arrays (n = 0: the loop has none)
struct PlanArgs {
  uint32_t* cnt = nullptr;    // n: tiles kept per query block since the planner last read them
  uint32_t* seen = nullptr;   // n: the counts the planner last read
  uint32_t* table = nullptr;  // budget entries
  int32_t n = 0, budget = 0, cap = 0;
};

}  // namespace m3d
