// robust_rows.h — the pieces of a robust terms pass that robust.hip and colored.hip share: the
// weight of a residual, the weighted row added to the 30 sums, and the dispatch on a checked
// kernel kind.  The operation order of each is stated in robust.hip's header.
#pragma once

#include <type_traits>

#include "m3d_internal.h"

namespace m3d {

constexpr int kRobustUsed = 30;

template <int K>
__device__ __forceinline__ double robust_weight(double r, double k) {
  if (K == M3D_KERNEL_L1) return 1.0 / fabs(r);
  if (K == M3D_KERNEL_HUBER) return k / fmax(fabs(r), k);
  if (K == M3D_KERNEL_CAUCHY) return 1.0 / (1.0 + (r / k) * (r / k));
  if (K == M3D_KERNEL_GM) return k / ((k + r * r) * (k + r * r));
  if (K == M3D_KERNEL_TUKEY) {
    const double t = fmin(1.0, fabs(r / k));
    const double u = 1.0 - t * t;
    return u * u;
  }
  return 1.0;
}

// v += the weighted row (J, r)
__device__ __forceinline__ void add_row(double (&v)[kRobustUsed], const double (&J)[6], double r, double w) {
  int k = 0;
#pragma unroll
  for (int a = 0; a < 6; ++a) {
    const double wa = w * J[a];
#pragma unroll
    for (int c = a; c < 6; ++c) v[k++] += wa * J[c];
    v[21 + a] += wa * r;
  }
  v[27] += r * r;
}

// f(integral_constant<int, kind>) for a checked kind
template <class F>
void with_kind(int32_t kind, F f) {
  switch (kind) {
    case M3D_KERNEL_L1: f(std::integral_constant<int, M3D_KERNEL_L1>{}); break;
    case M3D_KERNEL_HUBER: f(std::integral_constant<int, M3D_KERNEL_HUBER>{}); break;
    case M3D_KERNEL_CAUCHY: f(std::integral_constant<int, M3D_KERNEL_CAUCHY>{}); break;
    case M3D_KERNEL_GM: f(std::integral_constant<int, M3D_KERNEL_GM>{}); break;
    case M3D_KERNEL_TUKEY: f(std::integral_constant<int, M3D_KERNEL_TUKEY>{}); break;
    default: f(std::integral_constant<int, M3D_KERNEL_L2>{}); break;
  }
}

}  // namespace m3d
