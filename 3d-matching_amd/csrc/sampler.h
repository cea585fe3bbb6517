// sampler.h — the counter-based sampler of every randomised kernel (ransac.hip, plane.hip, feat.hip,
// fgr.hip) and the 64-bit mix behind it (also iss.hip's set signature).  Hypothesis h of a call with
// `seed` owns the stream splitmix64(base + 0), splitmix64(base + 1), …; nothing is shared between
// hypotheses, so a result does not depend on how they are batched or sharded.  The oracles restate
// these functions bit for bit (oracle/ransac_oracle.py::native_triples, tests/plane_restatement.py
// native_sample, tests/fgr_restatement.py trial_rows): change them together or not at all.
#pragma once

#include <stdint.h>

#include <hip/hip_runtime.h>

namespace m3d {

__device__ __forceinline__ uint64_t splitmix64(uint64_t x) {
  uint64_t z = x + 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// the start of hypothesis h's stream
__device__ __forceinline__ uint64_t sample_base(uint64_t seed, int64_t h) {
  return splitmix64(seed ^ ((uint64_t)h * 0x9E3779B97F4A7C15ull));
}

// draw k of a stream, in [0, n): the high word of a 32 × 32-bit product
__device__ __forceinline__ int64_t sample_draw(uint64_t base, uint64_t k, int64_t n) {
  return (int64_t)(((splitmix64(base + k) >> 32) * (uint64_t)n) >> 32);
}

// m DISTINCT indices of [0, n), n ≥ m: the stream's draws in order, repeats skipped
// (oracle/ransac_oracle.py::native_triples restates it bit for bit)
__device__ inline void native_sample(uint64_t seed, int64_t h, int64_t n, int m, int32_t* out) {
  const uint64_t base = sample_base(seed, h);
  int got = 0;
  for (uint64_t k = 0; got < m && k < (1u << 20); ++k) {
    const int32_t idx = (int32_t)sample_draw(base, k, n);
    bool dup = false;
    for (int j = 0; j < got; ++j) dup |= (out[j] == idx);
    if (!dup) out[got++] = idx;
  }
  for (; got < m; ++got) out[got] = got;  // unreachable for n ≥ m
}

// three rows of [0, n) WITH replacement, like Open3D's rand_gen() per row
__device__ __forceinline__ void trial_rows(uint64_t seed, int64_t h, int64_t n, int64_t r[3]) {
  const uint64_t base = sample_base(seed, h);
#pragma unroll
  for (int k = 0; k < 3; ++k) r[k] = sample_draw(base, (uint64_t)k, n);
}

}  // namespace m3d
