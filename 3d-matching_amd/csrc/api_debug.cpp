// api_debug.cpp — test hooks of the C ABI (include/m3d.h) that touch no library state: linalg.h, ddmath.h and
// nn_plan.h compiled for the host, and the acos probe.  A hook that reads or writes an object's state
// lives in the file of the code it probes.
#include "api_internal.h"
#include "ddmath.h"
#include "linalg.h"

using namespace m3d;
using namespace m3d::api;

extern "C" {

int m3d_debug_kabsch3_host(const double* src9, const double* tgt9, double* T16) {
  if (!src9 || !tgt9 || !T16) return M3D_ERR_INVALID;
  double ps[3][3], qs[3][3];
  for (int i = 0; i < 3; ++i)
    for (int k = 0; k < 3; ++k) {
      ps[i][k] = src9[3 * i + k];
      qs[i][k] = tgt9[3 * i + k];
    }
  return kabsch3(ps, qs, T16);
}

int m3d_debug_ldlt6_host(const double* A36, const double* b6, double* x6) {
  if (!A36 || !b6 || !x6) return M3D_ERR_INVALID;
  if (!ldlt6_solve_spd(A36, b6, x6)) ldlt6_solve(A36, b6, x6);  // the device solve's rule (icp.hip)
  return M3D_OK;
}

int m3d_debug_rotation_from_cov_host(const double* H9, double* R9) {
  if (!H9 || !R9) return M3D_ERR_INVALID;
  return rotation_from_cov(H9, R9);
}

int m3d_debug_sym3_eigenvalues_host(const double* sym6, double* lam3) {
  if (!sym6 || !lam3) return M3D_ERR_INVALID;
  sym3_eigenvalues(sym6[0], sym6[1], sym6[2], sym6[3], sym6[4], sym6[5], lam3);
  return M3D_OK;
}

int m3d_debug_sym3_eigen_host(const double* sym6, double* lam3, double* V9) {
  if (!sym6 || !lam3 || !V9) return M3D_ERR_INVALID;
  sym3_eigen(sym6[0], sym6[1], sym6[2], sym6[3], sym6[4], sym6[5], lam3, V9);
  return M3D_OK;
}

int m3d_debug_acos_cr(const double* u, int64_t n, double* out) {
  if (n < 0 || (n > 0 && (!u || !out))) return M3D_ERR_INVALID;
  for (int64_t k = 0; k < n; ++k) out[k] = acos_cr(u[k]);  // the device's code, compiled for the host
  return M3D_OK;
}

int m3d_debug_acos_device(m3d_ctx* ctx, const double* u, int64_t n, double* out, int mode, void* stream) {
  if (!ctx) return M3D_ERR_INVALID;
  CHECK_ARG(ctx, n >= 0 && (n == 0 || (u && out)) && (mode == 0 || mode == 1), "invalid arguments");
  hipSetDevice(ctx->device);
  HIPX(ctx, launch_acos_probe(u, n, out, mode, S(stream)));
  return M3D_OK;
}

int m3d_debug_nn_plan_host(const uint32_t* counts, int64_t n, int64_t budget, int64_t smax, int64_t ntiles,
                           uint32_t* out) {
  if (!counts || !out || smax < 1 || ntiles < 1) return M3D_ERR_INVALID;
  const uint32_t tau = plan_host(counts, n, budget, smax, ntiles, nullptr, out);
  return tau == 0 ? M3D_ERR_INVALID : (int)tau;
}

}  // extern "C"
