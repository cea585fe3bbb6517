// api_ransac.cpp — correspondence sets and the RANSAC drivers of the C ABI (include/m3d.h): kabsch3 batch /
// one, scoring, the device loop m3d_ransac_run(_async), the MT19937 replay of the reference RNG
// (m3d_replay_triples: the only numerical work on the host), feature matching and feature RANSAC.
// Scratch: the context's arena, and for feature RANSAC allocations of the call's own (api_internal.h).
#include <string.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "api_internal.h"

using namespace m3d;
using namespace m3d::api;

namespace {
constexpr int64_t kCorrPad = 2048;  // score kernel block footprint (ransac.hip kBlockCorr)

// deterministic mean of an n×3 device array (block partials summed in fixed order on host)
int device_mean3(m3d_ctx* ctx, const double* a, int64_t n, double out[3], hipStream_t st) {
  out[0] = out[1] = out[2] = 0.0;
  if (n == 0) return M3D_OK;
  const int blocks = 128;
  double* part = nullptr;
  int rc = dev_alloc(ctx, &part, blocks * 3);
  if (rc) return rc;
  hipError_t e = launch_sum3(a, n, part, blocks, st);
  std::vector<double> h(blocks * 3);
  if (e == hipSuccess) e = hipMemcpyAsync(h.data(), part, sizeof(double) * blocks * 3,
                                          hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  hipFree(part);
  if (e != hipSuccess) return m3d_fail(ctx, M3D_ERR_HIP, hipGetErrorString(e));
  for (int b = 0; b < blocks; ++b)
    for (int k = 0; k < 3; ++k) out[k] += h[3 * b + k];
  for (int k = 0; k < 3; ++k) out[k] /= (double)n;
  return M3D_OK;
}

int center_pack(m3d_ctx* ctx, const double* a, int64_t n, int64_t n_pad, const double c[3],
                float4* out, float pad, double* maxv, hipStream_t st) {
  *maxv = 0.0;
  if (n_pad == 0) return M3D_OK;
  const int blocks = (int)std::min<int64_t>(1024, (n_pad + 255) / 256);
  float* part = nullptr;
  int rc = dev_alloc(ctx, &part, blocks);
  if (rc) return rc;
  hipError_t e = launch_center_pack(a, n, n_pad, c, out, pad, part, blocks, 1, st);
  std::vector<float> h(blocks);
  if (e == hipSuccess)
    e = hipMemcpyAsync(h.data(), part, sizeof(float) * blocks, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  hipFree(part);
  if (e != hipSuccess) return m3d_fail(ctx, M3D_ERR_HIP, hipGetErrorString(e));
  float m = 0.0f;
  for (float v : h) m = std::max(m, v);
  *maxv = (double)m * (1.0 + 1e-6);
  return M3D_OK;
}

// ------------------------------------------------------------------------------- corrset
int corrset_build(m3d_ctx* ctx, const double* src, int64_t ns, const double* tgt, int64_t nt,
                         const int32_t* corr, const double* p_src, const double* p_tgt, int64_t nc,
                         void* stream, m3d_corrset** out) {
  CHECK_ARG(ctx, out != nullptr, "null output");
  CHECK_ARG(ctx, nc >= 0 && nc < (int64_t)1 << 31, "correspondence count out of range");
  hipSetDevice(ctx->device);
  hipStream_t st = S(stream);
  std::vector<int32_t> fixed;
  const int32_t* corr_dev = corr;
  int32_t* corr_tmp = nullptr;
  if (corr != nullptr && nc > 0) {
    // validate rows like numpy fancy indexing: negative indices wrap once, others raise
    fixed.resize(2 * nc);
    HIPX(ctx, hipMemcpyAsync(fixed.data(), corr, sizeof(int32_t) * 2 * nc, hipMemcpyDeviceToHost, st));
    HIPX(ctx, hipStreamSynchronize(st));
    bool changed = false;
    for (int64_t i = 0; i < nc; ++i) {
      for (int c = 0; c < 2; ++c) {
        int64_t lim = c == 0 ? ns : nt;
        int64_t v = fixed[2 * i + c];
        if (v < 0) {
          v += lim;
          changed = true;
        }
        if (v < 0 || v >= lim)
          return m3d_fail(ctx, M3D_ERR_INVALID, "correspondence index " +
                                                    std::to_string(fixed[2 * i + c]) +
                                                    " out of bounds for axis 0 with size " +
                                                    std::to_string(lim));
        fixed[2 * i + c] = (int32_t)v;
      }
    }
    if (changed) {
      int rc = dev_alloc(ctx, &corr_tmp, 2 * nc);
      if (rc) return rc;
      HIPX(ctx, hipMemcpyAsync(corr_tmp, fixed.data(), sizeof(int32_t) * 2 * nc,
                               hipMemcpyHostToDevice, st));
      corr_dev = corr_tmp;
    }
  }
  m3d_corrset* cs = new m3d_corrset();
  cs->ctx = ctx;
  cs->nc = nc;
  cs->nc_pad = nc > 0 ? round_up(nc, kCorrPad) : 0;
  int rc = dev_alloc(ctx, &cs->p64, 3 * nc);
  if (!rc) rc = dev_alloc(ctx, &cs->q64, 3 * nc);
  if (!rc) rc = dev_alloc(ctx, &cs->p32, cs->nc_pad);
  if (!rc) rc = dev_alloc(ctx, &cs->q32, cs->nc_pad);
  if (rc) {
    if (corr_tmp) hipFree(corr_tmp);
    m3d_corrset_destroy(cs);
    return rc;
  }
  hipError_t e = launch_pack_corr(src, tgt, corr_dev, nc, p_src, p_tgt, cs->p64, cs->q64, st);
  if (e != hipSuccess) {
    if (corr_tmp) hipFree(corr_tmp);
    m3d_corrset_destroy(cs);
    return m3d_fail(ctx, M3D_ERR_HIP, hipGetErrorString(e));
  }
  rc = device_mean3(ctx, cs->p64, nc, cs->cs, st);
  if (!rc) rc = device_mean3(ctx, cs->q64, nc, cs->ct, st);
  // pad: source 0, target far away → padded pairs are never inliers nor ambiguous
  if (!rc) rc = center_pack(ctx, cs->p64, nc, cs->nc_pad, cs->cs, cs->p32, 0.0f, &cs->pmax2, st);
  if (!rc) rc = center_pack(ctx, cs->q64, nc, cs->nc_pad, cs->ct, cs->q32, kFar, &cs->qmaxinf, st);
  if (!rc) {
    hipError_t e2 = launch_corr16(cs, st);  // MFMA scoring operands (ransac.hip)
    if (e2 != hipSuccess) rc = m3d_fail(ctx, M3D_ERR_HIP, hipGetErrorString(e2));
  }
  if (corr_tmp) {
    hipStreamSynchronize(st);
    hipFree(corr_tmp);
  }
  if (rc) {
    m3d_corrset_destroy(cs);
    return rc;
  }
  *out = cs;
  return M3D_OK;
}

// ------------------------------------------------------------------------------- a2/a3
struct ScoreScratch {
  HypF32* hypf;
  ScoreMf mf;
};

constexpr int kScoreSlots = 3;
void score_layout(Arena& a, int64_t H, size_t* o) {
  const int64_t hp = score_mf_hpad(std::max<int64_t>(H, 1));
  o[0] = a.take(sizeof(HypF32) * std::max<int64_t>(H, 1));
  o[1] = a.take(sizeof(uint4) * 6 * hp);
  o[2] = a.take(sizeof(float) * hp);
}

ScoreScratch score_bind(const Arena& a, const size_t* o) {
  ScoreScratch s;
  s.hypf = a.at<HypF32>(o[0]);
  s.mf.hb16 = a.at<uint4>(o[1]);
  s.mf.heps = a.at<float>(o[2]);
  return s;
}

double thr_sq_of(double thr, int mode) { return mode == M3D_SCORE_SQUARED ? thr : thr * thr; }

// score H transforms T (device) whose fp32 blocks are already in s.hypf and whose counts were
// zeroed by the kernel that produced them
hipError_t score_enqueue(m3d_ctx* ctx, const m3d_corrset* cs, const double* T, int64_t H,
                         double thr, int mode, int32_t* counts, const ScoreScratch& s,
                         const int32_t* done, hipStream_t st, bool prepared = false) {
  // prepared: kabsch3 already wrote the MFMA operands (ScoreFuse)
  hipError_t e = prepared ? hipSuccess : launch_score_prep(cs, T, H, thr, mode, s.mf, st);
  if (e != hipSuccess) return e;
  KTimer kt(ctx, M3D_KERNEL_SCORE, st);
  return launch_score(cs, s.hypf, H, counts, T, thr, mode, ctx->stats, done, s.mf, st);
}

// ------------------------------------------------------------------------------- one hypothesis
constexpr size_t kPinT = 0, kPinStatus = 128, kPinCount = 136;  // in the pinned page, below kPinRead
template <class T>
T* pin_at(const m3d_ctx* ctx, size_t o, bool dev) {
  return reinterpret_cast<T*>(static_cast<char*>(dev ? ctx->pin_dev : ctx->pin) + o);
}

// ------------------------------------------------------------------------------- MT19937 replay
struct MT {
  uint32_t key[624];
  int pos;
  void gen() {
    const uint32_t A = 0x9908b0dfu, UP = 0x80000000u, LO = 0x7fffffffu;
    int i;
    uint32_t y;
    for (i = 0; i < 624 - 397; ++i) {
      y = (key[i] & UP) | (key[i + 1] & LO);
      key[i] = key[i + 397] ^ (y >> 1) ^ ((0u - (y & 1u)) & A);
    }
    for (; i < 623; ++i) {
      y = (key[i] & UP) | (key[i + 1] & LO);
      key[i] = key[i + (397 - 624)] ^ (y >> 1) ^ ((0u - (y & 1u)) & A);
    }
    y = (key[623] & UP) | (key[0] & LO);
    key[623] = key[396] ^ (y >> 1) ^ ((0u - (y & 1u)) & A);
    pos = 0;
  }
  static uint32_t temper(uint32_t y) {
    y ^= (y >> 11);
    y ^= (y << 7) & 0x9d2c5680u;
    y ^= (y << 15) & 0xefc60000u;
    y ^= (y >> 18);
    return y;
  }
  uint32_t next() {
    if (pos >= 624) gen();
    return temper(key[pos++]);
  }
};
}  // namespace

extern "C" {

int m3d_corrset_create(m3d_ctx* ctx, const double* src_xyz, int64_t ns, const double* tgt_xyz,
                       int64_t nt, const int32_t* corr, int64_t nc, void* stream,
                       m3d_corrset** out) {
  if (!ctx) return M3D_ERR_INVALID;
  CHECK_ARG(ctx, nc == 0 || (src_xyz && tgt_xyz && corr), "null device pointer");
  CHECK_ARG(ctx, ns >= 0 && nt >= 0, "negative size");
  return corrset_build(ctx, src_xyz, ns, tgt_xyz, nt, corr, nullptr, nullptr, nc, stream, out);
}

int m3d_corrset_create_gathered(m3d_ctx* ctx, const double* p_src, const double* p_tgt,
                                int64_t nc, void* stream, m3d_corrset** out) {
  if (!ctx) return M3D_ERR_INVALID;
  CHECK_ARG(ctx, nc == 0 || (p_src && p_tgt), "null device pointer");
  return corrset_build(ctx, nullptr, 0, nullptr, 0, nullptr, p_src, p_tgt, nc, stream, out);
}

void m3d_corrset_destroy(m3d_corrset* cs) {
  if (!cs) return;
  hipFree(cs->p64);
  hipFree(cs->q64);
  hipFree(cs->p32);
  hipFree(cs->q32);
  hipFree(cs->ca16);
  delete cs;
}

int64_t m3d_corrset_size(const m3d_corrset* cs) { return cs ? cs->nc : -1; }

// ------------------------------------------------------------------------------- a1
int m3d_kabsch3_batch(m3d_ctx* ctx, const m3d_corrset* cs, const int32_t* triples, uint64_t seed,
                      int64_t hyp0, int64_t H, double* T_out, uint8_t* status, void* stream) {
  if (!ctx) return M3D_ERR_INVALID;
  CHECK_ARG(ctx, cs != nullptr && H >= 0 && (H == 0 || T_out), "invalid arguments");
  CHECK_ARG(ctx, triples != nullptr || cs->nc >= 3 || cs->nc < 3, "");
  hipSetDevice(ctx->device);
  Arena a(ctx, S(stream));
  size_t o_h = a.take(sizeof(HypF32) * (size_t)std::max<int64_t>(H, 1));
  int rc = a.commit();
  if (rc) return rc;
  hipError_t e = launch_kabsch3(cs, triples, seed, hyp0, H, 0.0, T_out, status,
                                a.at<HypF32>(o_h), nullptr, ZeroArgs{}, S(stream));
  if (e != hipSuccess) return m3d_fail(ctx, M3D_ERR_HIP, hipGetErrorString(e));
  return M3D_OK;
}

int m3d_ransac_score(m3d_ctx* ctx, const m3d_corrset* cs, const double* T, int64_t H, double thr,
                     int mode, int32_t* counts, void* stream) {
  if (!ctx) return M3D_ERR_INVALID;
  CHECK_ARG(ctx, cs != nullptr && H >= 0, "invalid arguments");
  CHECK_ARG(ctx, H == 0 || (T && counts), "null device pointer");
  CHECK_ARG(ctx, mode == M3D_SCORE_SQUARED || mode == M3D_SCORE_NORM, "unknown score mode");
  if (H == 0) return M3D_OK;
  hipSetDevice(ctx->device);
  hipStream_t st = S(stream);
  if (cs->nc == 0) {  // ransac.py:220-221 — ratio 0.0
    HIPX(ctx, hipMemsetAsync(counts, 0, sizeof(int32_t) * H, st));
    return M3D_OK;
  }
  Arena a(ctx, S(stream));
  size_t o[kScoreSlots];
  score_layout(a, H, o);
  int rc = a.commit();
  if (rc) return rc;
  ScoreScratch s = score_bind(a, o);
  hipError_t e = launch_hypf_from_T(cs, T, H, thr_sq_of(thr, mode), s.hypf, ZeroArgs{counts}, st);
  if (e == hipSuccess) e = score_enqueue(ctx, cs, T, H, thr, mode, counts, s, nullptr, st);
  if (e != hipSuccess) return m3d_fail(ctx, M3D_ERR_HIP, hipGetErrorString(e));
  return M3D_OK;
}

int m3d_kabsch3_one(m3d_ctx* ctx, const m3d_corrset* cs, const int32_t* triple, double* T_out,
                    int32_t* status, void* stream) {
  if (!ctx) return M3D_ERR_INVALID;
  CHECK_ARG(ctx, cs != nullptr && triple != nullptr && T_out != nullptr, "invalid arguments");
  hipSetDevice(ctx->device);
  int rc = pin_ensure(ctx);
  if (rc) return rc;
  hipStream_t st = S(stream);
  // the library's own staging: ordered after earlier scratch users on other streams
  Arena a(ctx, st);
  hipError_t e = launch_kabsch3_one(cs, triple, pin_at<double>(ctx, kPinT, true),
                                    pin_at<int32_t>(ctx, kPinStatus, true), st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return m3d_fail(ctx, M3D_ERR_HIP, hipGetErrorString(e));
  memcpy(T_out, pin_at<double>(ctx, kPinT, false), sizeof(double) * 16);
  if (status) *status = *pin_at<int32_t>(ctx, kPinStatus, false);
  return M3D_OK;
}

int m3d_ransac_score_one(m3d_ctx* ctx, const m3d_corrset* cs, const double* T, double thr, int mode,
                         int64_t* count, void* stream) {
  if (!ctx) return M3D_ERR_INVALID;
  CHECK_ARG(ctx, cs != nullptr && T != nullptr && count != nullptr, "invalid arguments");
  CHECK_ARG(ctx, mode == M3D_SCORE_SQUARED || mode == M3D_SCORE_NORM, "unknown score mode");
  if (cs->nc == 0) {  // ransac.py:220-221
    *count = 0;
    return M3D_OK;
  }
  hipSetDevice(ctx->device);
  int rc = pin_ensure(ctx);
  if (rc) return rc;
  hipStream_t st = S(stream);
  hipError_t e;
  {
    Arena a(ctx, st);
    const int64_t nb = count_one_blocks(cs->nc);
    const size_t o_p = a.take(sizeof(int32_t) * nb);
    rc = a.commit();
    if (rc) return rc;
    e = launch_count_one(cs, T, thr, mode, a.at<int32_t>(o_p), nb, ctx->one_ticket,
                         pin_at<int64_t>(ctx, kPinCount, true), st);
  }
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return m3d_fail(ctx, M3D_ERR_HIP, hipGetErrorString(e));
  *count = *pin_at<int64_t>(ctx, kPinCount, false);
  return M3D_OK;
}

// ------------------------------------------------------------------------------- a4
int m3d_ransac_run_async(m3d_ctx* ctx, const m3d_corrset* cs, const m3d_ransac_params* p,
                         const int32_t* triples, int32_t* counts_out,
                         m3d_ransac_result* result_dev, void* stream) {
  if (!ctx) return M3D_ERR_INVALID;
  CHECK_ARG(ctx, cs && p && result_dev, "invalid arguments");
  CHECK_ARG(ctx, p->max_iter >= 0, "max_iter must be >= 0");
  CHECK_ARG(ctx, p->mode == M3D_SCORE_SQUARED || p->mode == M3D_SCORE_NORM, "unknown score mode");
  hipSetDevice(ctx->device);
  hipStream_t st = S(stream);
  const int64_t nc = cs->nc;
  const int64_t max_iter = p->max_iter;
  int64_t B = p->batch;
  if (B <= 0) {
    // ~1e10 pair evaluations per batch (≤ 2^18 hypotheses, ~80 MB of scratch) amortise the
    // per-batch kabsch3/select latency and give the scoring grid more blocks (cfg2, 1e5
    // hypotheses: 10k per batch 2.15 ms, 25k 1.66 ms, 100k 1.55 ms — tools/ransac_batch.py);
    // early stop caps it (the stop is decided per batch)
    B = nc > 0 ? std::max<int64_t>(1024, std::min<int64_t>((int64_t)1 << 18,
                                                           (int64_t)1e10 / std::max<int64_t>(nc, 1)))
               : 1024;
    if (p->early_stop) B = std::min<int64_t>(B, 16384);
  }
  B = std::max<int64_t>(1, std::min<int64_t>(B, std::max<int64_t>(max_iter, 1)));
  const double thr_sq = thr_sq_of(p->thr, p->mode);
  Arena a(ctx, S(stream));
  size_t o[kScoreSlots];
  score_layout(a, B, o);
  size_t o_T = a.take(sizeof(double) * 16 * B);
  size_t o_c = a.take(sizeof(int32_t) * B);
  int rc = a.commit();
  if (rc) return rc;
  ScoreScratch s = score_bind(a, o);
  double* Tb = a.at<double>(o_T);
  int32_t* cb = a.at<int32_t>(o_c);
  // counts of the hypotheses after an early stop are never scored: they read 0
  if (counts_out != nullptr && max_iter > 0)
    HIPX(ctx, hipMemsetAsync(counts_out, 0, sizeof(int32_t) * max_iter, st));
  HIPX(ctx, launch_ransac_init(ctx->rstate, ctx->stats, max_iter == 0 ? 1 : 0, st));
  const int32_t* done = &ctx->rstate->done;
  for (int64_t b0 = 0; b0 < max_iter; b0 += B) {
    const int64_t n = std::min(B, max_iter - b0);
    const int32_t* tri = triples ? triples + 3 * b0 : nullptr;
    int32_t* cnt = counts_out ? counts_out + b0 : cb;
    hipError_t e;
    {
      KTimer kt(ctx, M3D_KERNEL_KABSCH, st);
      const ScoreFuse fz{&s.mf, p->thr, p->mode};
      e = launch_kabsch3(cs, tri, p->seed, p->hyp0 + b0, n, thr_sq, Tb, nullptr, s.hypf, done,
                         ZeroArgs{cnt}, st, nc > 0 ? &fz : nullptr);
    }
    if (e == hipSuccess) {
      if (nc > 0) {
        e = score_enqueue(ctx, cs, Tb, n, p->thr, p->mode, cnt, s, done, st, true);
      } else {
        e = hipMemsetAsync(cnt, 0, sizeof(int32_t) * n, st);
      }
    }
    if (e == hipSuccess)
      e = launch_select(cnt, b0, n, std::max<int64_t>(nc, 1), max_iter, p->early_stop,
                        p->es_threshold, p->es_confidence, Tb, ctx->rstate, st);
    if (e != hipSuccess) return m3d_fail(ctx, M3D_ERR_HIP, hipGetErrorString(e));
  }
  hipError_t e = launch_copy_result(ctx->rstate, nc, ctx->stats, result_dev, st);
  if (e != hipSuccess) return m3d_fail(ctx, M3D_ERR_HIP, hipGetErrorString(e));
  return M3D_OK;
}

int m3d_ransac_run(m3d_ctx* ctx, const m3d_corrset* cs, const m3d_ransac_params* p,
                   const int32_t* triples, m3d_ransac_result* out, void* stream) {
  if (!ctx) return M3D_ERR_INVALID;
  CHECK_ARG(ctx, out != nullptr, "null output");
  m3d_ransac_result* dres = nullptr;
  int rc = dev_alloc(ctx, &dres, 1);
  if (rc) return rc;
  hipMemsetAsync(dres, 0, sizeof(*dres), S(stream));
  rc = m3d_ransac_run_async(ctx, cs, p, triples, nullptr, dres, stream);
  if (!rc) {
    hipError_t e = hipMemcpyAsync(out, dres, sizeof(*out), hipMemcpyDeviceToHost, S(stream));
    if (e == hipSuccess) e = hipStreamSynchronize(S(stream));
    if (e != hipSuccess) rc = m3d_fail(ctx, M3D_ERR_HIP, hipGetErrorString(e));
  }
  hipFree(dres);
  return rc;
}

int m3d_replay_triples(uint32_t* mt_key, int32_t* mt_pos, int64_t nc, int64_t H,
                       int32_t* triples_out) {
  if (!mt_key || !mt_pos || (H > 0 && !triples_out)) return M3D_ERR_INVALID;
  if (nc < 3 || nc > 0xffffffffll) return M3D_ERR_INVALID;
  if (*mt_pos < 0 || *mt_pos > 624) return M3D_ERR_INVALID;
  MT mt;
  memcpy(mt.key, mt_key, sizeof(mt.key));
  mt.pos = *mt_pos;
  // legacy RandomState.choice(nc, 3, replace=False) == permutation(nc)[:3]; permutation shuffles
  // arange(nc) with i = nc-1 .. 1, j_i = random_interval(i), swap(x[i], x[j_i]).  Only positions
  // 0..2 are needed: the draws are stored (sequential writes), then each position is traced back
  // through the swaps in reverse order (i = 1 .. nc-1: p == i → j_i, p == j_i → i), which lands
  // on the initial index, i.e. the value.  Sequential passes, no O(nc) value array.
  thread_local std::vector<uint32_t> jbuf;
  if (jbuf.size() < (size_t)nc + 64) jbuf.resize((size_t)nc + 64);
  uint32_t* j = jbuf.data();
  uint32_t tk[624];  // the tempered outputs of the current key block
  auto temper_block = [&](int from) {
    for (int k = from; k < 624; ++k) tk[k] = MT::temper(mt.key[k]);  // vectorised
  };
  if (mt.pos < 624) temper_block(mt.pos);
  for (int64_t h = 0; h < H; ++h) {
    // random_interval(i) for i = nc-1 .. 1, branch-free: every MT output is a candidate
    // (y & mask(i), mask = 2^(⌊log2 i⌋+1) − 1) that is kept iff ≤ i — the rejection loop's
    // outcome is unpredictable, a branch on it costs more than the generator.  The mask is
    // constant while i stays above mask >> 1, so the dependency chain per output is the compare
    // and the decrement.
    int64_t i = nc - 1;
    while (i >= 1) {
      const uint32_t mask = 0xFFFFFFFFu >> __builtin_clz((uint32_t)i);
      const int64_t lo = (int64_t)(mask >> 1);
      while (i > lo) {
        if (mt.pos >= 624) {
          mt.gen();
          temper_block(0);
        }
        // at least i − lo more outputs are needed before i reaches lo (each output lowers i by
        // at most one), so that many run without a bound check
        const int k0 = mt.pos;
        const int n = (int)std::min<int64_t>(624 - k0, i - lo);
        uint32_t ii = (uint32_t)i;
        for (int k = k0; k < k0 + n; ++k) {
          const uint32_t v = tk[k] & mask;
          j[ii] = v;
          ii -= (uint32_t)(v <= ii);
        }
        mt.pos = k0 + n;
        i = ii;
      }
    }
    // trace positions 0..2 back through the swaps (i ascending).  After step i a traced
    // position p is ≤ i, so from i = 3 on it can only move when j_i == p (then p := i): a
    // vectorised search for the next index whose draw equals one of the three positions
    uint32_t p[3] = {0, 1, 2};
    for (int64_t a = 1; a < std::min<int64_t>(nc, 3); ++a) {
      const uint32_t ji = j[a], ia = (uint32_t)a;
      for (int q = 0; q < 3; ++q) p[q] = p[q] == ia ? ji : (p[q] == ji ? ia : p[q]);
    }
    int64_t a = 3;
    constexpr int kW = 32;
    while (a < nc) {
      const int64_t e = std::min<int64_t>(nc, a + kW);
      uint32_t any = 0;
      if (e - a == kW) {
        const uint32_t p0 = p[0], p1 = p[1], p2 = p[2];
        for (int t = 0; t < kW; ++t) {
          const uint32_t v = j[a + t];
          any |= (uint32_t)(v == p0) | (uint32_t)(v == p1) | (uint32_t)(v == p2);
        }
      } else {
        any = 1;
      }
      if (any) {
        for (int64_t b = a; b < e; ++b)
          for (int q = 0; q < 3; ++q) p[q] = j[b] == p[q] ? (uint32_t)b : p[q];
      }
      a = e;
    }
    triples_out[3 * h + 0] = (int32_t)p[0];
    triples_out[3 * h + 1] = (int32_t)p[1];
    triples_out[3 * h + 2] = (int32_t)p[2];
  }
  memcpy(mt_key, mt.key, sizeof(mt.key));
  *mt_pos = mt.pos;
  return M3D_OK;
}

// ------------------------------------------------------------------------------- feature matching
int m3d_feature_correspondences(m3d_ctx* ctx, const double* f_src, int64_t ns, const double* f_tgt,
                                int64_t nt, int32_t dim, int32_t mutual_filter,
                                double mutual_consistent_ratio, int32_t* corr_out, int64_t* n_out,
                                void* stream) {
  if (!ctx) return M3D_ERR_INVALID;
  CHECK_ARG(ctx, dim == 33, "feature dimension must be 33 (FPFH)");
  CHECK_ARG(ctx, n_out && ns >= 0 && nt >= 0 && ns < ((int64_t)1 << 31) && nt < ((int64_t)1 << 31),
            "invalid arguments");
  CHECK_ARG(ctx, (ns == 0 || (f_src && corr_out)) && (nt == 0 || f_tgt), "null device pointer");
  hipSetDevice(ctx->device);
  HIPX(ctx, feature_correspondences(f_src, ns, f_tgt, nt, mutual_filter, mutual_consistent_ratio,
                                    corr_out, n_out, S(stream)));
  return M3D_OK;
}

int m3d_ransac_on_correspondences(m3d_ctx* ctx, const m3d_cloud* src, const m3d_cloud* tgt,
                                  const int32_t* corr, int64_t nc,
                                  const m3d_feature_ransac_params* p,
                                  m3d_feature_ransac_result* out, int32_t* corr_set_out,
                                  void* stream) {
  if (!ctx) return M3D_ERR_INVALID;
  CHECK_ARG(ctx, src && tgt && p && out, "invalid arguments");
  CHECK_ARG(ctx, p->ransac_n <= 3, "ransac_n > 3 is not supported (the reference uses 3)");
  CHECK_ARG(ctx, p->max_iteration >= 0, "max_iteration must be >= 0");
  hipSetDevice(ctx->device);
  hipStream_t st = S(stream);
  Touch tch{ctx, st};
  memset(out, 0, sizeof(*out));
  for (int k = 0; k < 16; ++k) out->T[k] = (k % 5 == 0) ? 1.0 : 0.0;
  out->best_index = -1;
  const int64_t ns = src->n;
  if (corr_set_out && ns > 0) HIPX(ctx, hipMemsetAsync(corr_set_out, 0xFF, 4 * ns, st));
  // Open3D returns an empty RegistrationResult for these (Registration.cpp)
  if (p->ransac_n < 3 || nc < p->ransac_n || !(p->max_correspondence_distance > 0.0) ||
      p->max_iteration == 0 || ns == 0 || tgt->n == 0) {
    HIPX(ctx, hipStreamSynchronize(st));
    return M3D_OK;
  }
  CHECK_ARG(ctx, corr != nullptr, "null correspondence pointer");
  const int64_t H = p->max_iteration;
  DevTmp<double> T;
  DevTmp<int32_t> pass;
  int rc = dev_alloc(ctx, &T.p, 16 * H);
  if (!rc) rc = dev_alloc(ctx, &pass.p, H);
  if (rc) return rc;
  HIPX(ctx, launch_feat_hyp(src->xyz64, tgt->xyz64, corr, nc, p->seed, H, p->edge_length,
                            p->distance, T.p, pass.p, st));
  std::vector<int32_t> hpass(H);
  HIPX(ctx, hipMemcpyAsync(hpass.data(), pass.p, 4 * H, hipMemcpyDeviceToHost, st));
  HIPX(ctx, hipStreamSynchronize(st));
  const m3d_icp_params ip = probe_params(M3D_EST_POINT_TO_POINT, M3D_NN_GRID);
  ScopedLoop s;
  rc = m3d_icp_create(ctx, src, tgt, p->max_correspondence_distance, &ip, &s.s);
  if (rc) return rc;
  // Validation of the checker-passing hypotheses in batches (grid.hip validate_kernel: one launch
  // evaluates a whole batch), each batch followed by Open3D's sequential selection over it:
  // IsBetterRANSACThan and the early exit at est_k (a hypothesis at or past est_k is never
  // validated).  Batches grow from 64 so the reference's iteration = 30 costs one small launch;
  // a batch that straddles est_k only computes results the selection then ignores.
  std::vector<int32_t> list;
  for (int64_t h = 0; h < H; ++h)
    if (hpass[h]) list.push_back((int32_t)h);
  const int64_t npass = (int64_t)list.size();
  const int64_t cap = std::min<int64_t>(
      npass, std::max<int64_t>(64, std::min<int64_t>(8192, ((int64_t)1 << 23) / std::max<int64_t>(ns, 1))));
  const int64_t nbq = validate_blocks(ns);
  DevTmp<int32_t> dlist, vcorr;
  DevTmp<IcpState> vst;
  DevTmp<double> vpart, vres;
  if (npass > 0) {
    rc = dev_alloc(ctx, &dlist.p, npass);
    if (!rc) rc = dev_alloc(ctx, &vst.p, cap);
    if (!rc) rc = dev_alloc(ctx, &vpart.p, cap * nbq * 2);
    if (!rc) rc = dev_alloc(ctx, &vres.p, cap * 2);
    if (!rc) rc = dev_alloc(ctx, &vcorr.p, cap);
    if (rc) return rc;
  }
  hipError_t e = hipSuccess;
  if (npass > 0)
    e = hipMemcpyAsync(dlist.p, list.data(), 4 * npass, hipMemcpyHostToDevice, st);
  int64_t est_k = H, best = -1;
  double best_fit = 0.0, best_rmse = 0.0, corres_ratio = 0.0;
  std::vector<double> hs;
  std::vector<int32_t> hc;
  for (int64_t c0 = 0, bsz = std::min<int64_t>(64, cap); c0 < npass && e == hipSuccess;
       c0 += bsz, bsz = std::min<int64_t>(cap, 2 * bsz)) {
    if (list[c0] >= est_k) break;
    const int64_t n = std::min<int64_t>(bsz, npass - c0);
    e = launch_val_states(s, T.p, dlist.p + c0, n, vst.p, st);
    if (e == hipSuccess)
      e = launch_validate(s->sgrid, ns, s->src->xyz64, s->tgrid, tgt->xyz64, tgt->n, vst.p, n, vpart.p,
                          vres.p, st);
    // the exit rule's correspondence inlier counts of the same batch (one small launch; only a
    // new best's is read)
    if (e == hipSuccess)
      e = launch_corres_inlier(src->xyz64, tgt->xyz64, corr, nc, T.p, dlist.p + c0, n,
                               p->max_correspondence_distance, vcorr.p, st);
    hs.resize(2 * (size_t)n);
    hc.resize((size_t)n);
    if (e == hipSuccess)
      e = hipMemcpyAsync(hs.data(), vres.p, sizeof(double) * 2 * n, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess)
      e = hipMemcpyAsync(hc.data(), vcorr.p, sizeof(int32_t) * n, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) break;
    for (int64_t k = 0; k < n; ++k) {
      const int64_t h = list[c0 + k];
      if (h >= est_k) break;
      out->validations += 1;
      const double cnt = hs[2 * k], se = hs[2 * k + 1];
      const double fit = cnt > 0.0 ? cnt / (double)ns : 0.0;
      const double rmse = cnt > 0.0 ? std::sqrt(se / cnt) : 0.0;
      if (fit > best_fit || (fit == best_fit && rmse < best_rmse)) {  // IsBetterRANSACThan
        best = h;
        best_fit = fit;
        best_rmse = rmse;
        // Open3D 0.19 (Registration.cpp RegistrationRANSACBasedOnCorrespondence): the exit
        // estimate comes from the new best's CORRESPONDENCE inlier ratio
        // (EvaluateInlierCorrespondenceRatio), not from its fitness:
        //   est_k_d = log(1 − confidence) / log(1 − ratio^ransac_n); est_k ← ceil(est_k_d) if smaller.
        // ratio = 1: log(0) = −inf, est_k_d = −0.0 → 0.  ratio = 0: a division by +0.0 → −inf,
        // whose int conversion upstream is INT_MIN on x86 → stop (0 here).  NaN: no change.
        const double ratio = (double)hc[k] / (double)nc;
        corres_ratio = ratio;
        const double kd = std::log(1.0 - p->confidence) /
                          std::log(1.0 - std::pow(ratio, (double)p->ransac_n));
        if (kd < (double)est_k) est_k = std::isfinite(kd) ? (int64_t)std::ceil(kd) : 0;
      }
    }
  }
  if (e != hipSuccess) return m3d_fail(ctx, M3D_ERR_HIP, std::string("feature RANSAC: ") + hipGetErrorString(e));
  if (best >= 0) {
    e = hipMemcpyAsync(out->T, T.p + 16 * best, sizeof(double) * 16, hipMemcpyDeviceToHost, st);
    out->fitness = best_fit;
    out->inlier_rmse = best_rmse;
    out->best_index = best;
    out->corres_ratio = corres_ratio;
    if (e == hipSuccess && corr_set_out) {
      e = launch_icp_set_T(s, T.p + 16 * best, st);
      s->points_moved = true;  // set_T, then the terms pass below
      if (e == hipSuccess) e = enqueue_nn(s, 0, st);
      if (e == hipSuccess) e = launch_icp_terms_mode(s, 0, nullptr, nullptr, st);
      if (e == hipSuccess)
        e = launch_scatter_i32(s->corr, s->src->slot, ns, corr_set_out, st);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st);
  }
  if (e != hipSuccess) return m3d_fail(ctx, M3D_ERR_HIP, hipGetErrorString(e));
  return M3D_OK;
}

}  // extern "C"
