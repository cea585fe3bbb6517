// nn_brute.hip — the brute-force nearest-neighbour scan of the ICP loop for gfx950 (icp.hip's "nn"
// step, O(Ns·Nt)): the target's MFMA operand tiles and their boxes (build_mfma_tiles), the box
// cull (box_out_of_reach), nn_mfma_kernel and its launcher.  Per query the scan state (k1, near2)
// of nnkey.h; the target tiles are dealt to grid.y in strides and the blocks merge with a 64-bit
// atomicMin on packed (bits(d²) << 32 | idx): order independent → deterministic, lowest index wins
// exact ties.  Shares only IcpState and nnkey.h with the fp64 tail in icp.hip.
#include <algorithm>

#include "lds_dma.h"
#include "m3d_internal.h"
#include "nnkey.h"

// Two translation units.  nn_mfma_kernel (the 2-D launch) and nn_mfma_plan_kernel (the planned 1-D
// launch) instantiate one body (nn_mfma_body), and each sits at 128 VGPRs without scratch only when
// it is the one NN kernel of its translation unit: with both in one, the 2-D kernel — otherwise the
// code from before the plan but for nine scalar instructions, same descriptor — spills 12 B and the planned one 8 B (the shared
// helpers are inlined in another order).  So nn_brute_plan.hip compiles this file again with
// M3D_NN_BRUTE_PLAN_TU=1 and keeps only the device code, the planned kernel and its launcher;
// this file's own compilation keeps everything else.  Clock builds (M3D_NN_CLOCK, one record array)
// keep both kernels here and leave nn_brute_plan.hip empty.
#ifndef M3D_NN_BRUTE_PLAN_TU
#define M3D_NN_BRUTE_PLAN_TU 0
#endif
#ifndef M3D_NN_CLOCK
#define M3D_NN_CLOCK 0
#endif
// A third unit, nn_brute_terms.hip (M3D_NN_BRUTE_TERMS_TU=1), holds nn_mfma_terms_kernel: the planned
// kernel whose blocks also run their query block's terms pass (nn_terms_handoff below), with
// icp.hip's terms pass compiled into it (M3D_ICP_TERMS_ONLY).  One kernel per unit, as above.
#ifndef M3D_NN_BRUTE_TERMS_TU
#define M3D_NN_BRUTE_TERMS_TU 0
#endif
#define M3D_NN_TU_MAIN (!M3D_NN_BRUTE_PLAN_TU && !M3D_NN_BRUTE_TERMS_TU)
#define M3D_NN_TU_PLAN_KERNEL (M3D_NN_BRUTE_PLAN_TU ? !M3D_NN_CLOCK : (M3D_NN_TU_MAIN && M3D_NN_CLOCK))
#define M3D_NN_TU_TERMS_KERNEL (M3D_NN_BRUTE_TERMS_TU ? !M3D_NN_CLOCK : (M3D_NN_TU_MAIN && M3D_NN_CLOCK))
#if M3D_NN_TU_MAIN || M3D_NN_TU_PLAN_KERNEL || M3D_NN_TU_TERMS_KERNEL
#if M3D_NN_TU_TERMS_KERNEL
// the terms pass (terms_block, TermsArgs, NnTermsDev) without the tail's clock stamps
#undef M3D_TAIL_CLOCK
#undef M3D_TERMS_CLOCK
#define M3D_TAIL_CLOCK 0
#define M3D_TERMS_CLOCK 0
#define M3D_ICP_TERMS_ONLY 1
#include "icp.hip"
#endif

namespace m3d {

// ------------------------------------------------------------------------------- NN, MFMA screen
// The screen key |t|² − 2q·t is a rank-4 contraction over (x, y, z, 1): here it runs on the
// matrix cores.  One v_mfma_f32_32x32x16_f16 computes S²·(key − thr) for 32 targets (A rows) ×
// 32 queries (B columns) from fp16 hi/lo splits of the S-scaled operands, K = 16:
//   A (target) = [xh, xh, xl, yh, yh, yl, zh, zh | zl, wh, wl, 1,   1,   0, 0, 0]
//   B (query)  = [ah, al, ah, bh, bl, bh, ch, cl | ch, 1,  1,  −Th, −Tl, 0, 0, 0]
// (a,b,c) = −2S·q; Th + Tl = the query's threshold S²·thr split in fp16 (thr_split).  Products
// of fp16 are exact in fp32; the bound on the key error is screen_eps_m (refresh_rt32) plus the
// threshold terms' share of the accumulation and split error (thr_operand).  So a target can
// only be a candidate if its value is negative, and the screen is a sign test: per MFMA a lane
// ORs the bit patterns of its 16 values with v_bitop3_b32 — a full-rate 3-input op on gfx950,
// where v_min3/v_minimum3/v_or3 issue at half rate (tools/ubench_ops.hip) — and tests bit 31.
// A lane holds column c = lane & 31 (its query) and 16 of the 32 rows; the lane pair (c, c + 32)
// covers all 32.  A sub-tile that hits anywhere in the wave runs the fp32 exact path
// (direct d², lexicographic (d², index)) over the lane's 16 rows, and the pair merges its two
// states with one shuffle.  Result: the same key as a full direct scan and as the grid search.
typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef float floatx16 __attribute__((ext_vector_type(16)));

constexpr int kMG = 2;        // 32-query groups per wave
constexpr int kMTile = 256;   // targets per half tile (8 sub-tiles of 32)
constexpr int kTH = 4;        // half tiles per LDS tile
constexpr int kMTilePad = 1024; // MFMA operand arrays are padded to a multiple of every tile size
constexpr int kMBlock = 512;  // 8 waves × kMG × 32 = 512 queries per block: every target tile
                              // staged in LDS serves 512 queries (L2→LDS traffic per pair halved)
constexpr int kMQueries = (kMBlock / 64) * kMG * 32;  // queries per block

__device__ __forceinline__ void split16(float x, _Float16& hi, _Float16& lo) {
  hi = (_Float16)x;
  lo = (_Float16)(x - (float)hi);
}

union H8 {
  uint4 u;
  half8 h;
};

// Sign bits of 16 screen values ORed by a full-rate tree: 7 v_bitop3_b32 (a | b | c) + 1 v_or.
__device__ __forceinline__ uint32_t or16(const floatx16& k) {
  const auto b = [&](int i) { return __float_as_uint(k[i]); };
  const uint32_t o0 = __builtin_amdgcn_bitop3_b32(b(0), b(1), b(2), 0xFE);
  const uint32_t o1 = __builtin_amdgcn_bitop3_b32(b(3), b(4), b(5), 0xFE);
  const uint32_t o2 = __builtin_amdgcn_bitop3_b32(b(6), b(7), b(8), 0xFE);
  const uint32_t o3 = __builtin_amdgcn_bitop3_b32(b(9), b(10), b(11), 0xFE);
  const uint32_t o4 = __builtin_amdgcn_bitop3_b32(b(12), b(13), b(14), 0xFE);
  const uint32_t o5 = __builtin_amdgcn_bitop3_b32(o0, o1, o2, 0xFE);
  const uint32_t o6 = __builtin_amdgcn_bitop3_b32(o3, o4, b(15), 0xFE);
  return o5 | o6;
}

// The query's threshold as B operand elements 11-12 (lane half 1), in S² units.  thr0 =
// ((best − |q|²) + eps)·S² carries the key's error bound; the threshold terms add their own
// share of the MFMA's accumulation bound (32u·|thr|, as for the other products) and of the fp16
// split (u16²|thr| + σ), with 5 % slack that also covers this sum's fp32 rounding, so that every
// candidate's value is strictly negative.  |thr| is clamped to 32768 (fp16 range): clamping a
// negative threshold up only adds false hits; a positive threshold that large (radius far
// beyond the cloud's extent) sets `force`, and the group then runs the exact path everywhere.
__device__ __forceinline__ void thr_operand(half8& b, float thr0, bool& force) {
  const float extra = 1.05f * ((32.0f * 1.01f * 5.9604645e-08f + 2.3841858e-07f) * fabsf(thr0) +
                               5.9604645e-08f);
  float thr = thr0 + extra;
  force = thr > 32768.0f;
  thr = fminf(fmaxf(thr, -32768.0f), 32768.0f);
  const _Float16 th = (_Float16)thr;
  const _Float16 tl = (_Float16)(thr - (float)th);
  b[3] = -th;
  b[4] = -tl;
}

#if M3D_NN_TU_MAIN
// target operand rows in Morton order of the grid's cells (build_mfma_tiles); 0 (A/B builds):
// row-major cells
#ifndef M3D_NN_TILE_MORTON
#define M3D_NN_TILE_MORTON 1
#endif
// MFMA screen operands of a cloud (A rows of nn_mfma_kernel), rows in Morton order of its grid's
// cells — or in the grid's row-major cell order, M3D_NN_TILE_MORTON=0 (build_mfma_tiles):
// mf16 = fp16 split (+ the two constant-1 threshold slots), mf32 = (x, y, z, original index
// bits).  Pads: key 65504 (never hit),
// far-away coordinates (never accepted by the exact path).
__global__ __launch_bounds__(256) void pack16_sorted_kernel(const float4* __restrict__ sorted,
                                                            const int32_t* __restrict__ perm,
                                                            const float4* __restrict__ xyz32,
                                                            int64_t n, int64_t n_pad, float S,
                                                            uint4* __restrict__ mf16,
                                                            float4* __restrict__ mf32) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= n_pad) return;
  H8 a, b;
  a.u = make_uint4(0, 0, 0, 0);
  b.u = make_uint4(0, 0, 0, 0);
  if (k < n) {
    // row k: the k-th point of `sorted` (cell order), or of its permutation perm
    const int32_t idx = __float_as_int(sorted[perm != nullptr ? perm[k] : k].w);
    const float4 t = xyz32[idx];  // w = |t|² (center_pack)
    _Float16 xh, xl, yh, yl, zh, zl, wh, wl;
    split16(t.x * S, xh, xl);
    split16(t.y * S, yh, yl);
    split16(t.z * S, zh, zl);
    split16(t.w * (S * S), wh, wl);
    a.h = half8{xh, xh, xl, yh, yh, yl, zh, zh};
    b.h = half8{zl, wh, wl, (_Float16)1, (_Float16)1, (_Float16)0, (_Float16)0, (_Float16)0};
    mf32[k] = make_float4(t.x, t.y, t.z, __int_as_float(idx));
  } else {
    b.h[1] = (_Float16)65504.0f;  // value ≥ 65504 − 32768 > 0: never a hit
    b.h[3] = (_Float16)1;
    b.h[4] = (_Float16)1;
    mf32[k] = make_float4(1.0e18f, 1.0e18f, 1.0e18f, __int_as_float(-1));
  }
  mf16[k] = a.u;  // two planes: elements 0-7 (lane half 0), elements 8-15 (lane half 1)
  mf16[n_pad + k] = b.u;
}

// Box of each 256-row half tile of mf32 (one block per half): box[2·half] = (lo.xyz, ·),
// box[2·half + 1] = (hi.xyz, ·) over the rows' exact fp32 coordinates — the values nn_exact_rows
// feeds to d2f — pads (index bits < 0) left out; an all-pad half keeps lo = +inf, hi = −inf.
__global__ __launch_bounds__(kMTile) void tile_box_kernel(const float4* __restrict__ mf32,
                                                          float4* __restrict__ box) {
  const float4 t = mf32[(int64_t)blockIdx.x * kMTile + threadIdx.x];
  const bool real = __float_as_int(t.w) >= 0;
  float v[6] = {real ? t.x : kInf,  real ? t.y : kInf,  real ? t.z : kInf,
                real ? t.x : -kInf, real ? t.y : -kInf, real ? t.z : -kInf};
#pragma unroll
  for (int o = 1; o < 64; o <<= 1)
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      const float w = __shfl_xor(v[k], o);
      v[k] = k < 3 ? fminf(v[k], w) : fmaxf(v[k], w);
    }
  __shared__ float part[kMTile / 64][6];
  if ((threadIdx.x & 63) == 0)
#pragma unroll
    for (int k = 0; k < 6; ++k) part[threadIdx.x >> 6][k] = v[k];
  __syncthreads();
  if (threadIdx.x != 0) return;
#pragma unroll
  for (int w = 1; w < kMTile / 64; ++w)
#pragma unroll
    for (int k = 0; k < 6; ++k) v[k] = k < 3 ? fminf(v[k], part[w][k]) : fmaxf(v[k], part[w][k]);
  box[2 * (int64_t)blockIdx.x] = make_float4(v[0], v[1], v[2], 0.0f);
  box[2 * (int64_t)blockIdx.x + 1] = make_float4(v[3], v[4], v[5], 0.0f);
}

hipError_t build_mfma_tiles(const m3d_cloud* c, Grid* g, TmpArena* ta, hipStream_t st) {
  const int64_t n = c->n;
  const int64_t n_pad = std::max<int64_t>((n + kMTilePad - 1) / kMTilePad * kMTilePad, kMTilePad);
  const int32_t* perm = nullptr;  // (setup arena: consumed by pack16_sorted_kernel below)
  hipError_t e = M3D_NN_TILE_MORTON ? grid_morton_perm(g, ta, st, &perm) : hipSuccess;
  if (e != hipSuccess) return e;
  e = block_alloc(reinterpret_cast<void**>(&g->mf16), sizeof(uint4) * 2 * n_pad, st);
  if (e == hipSuccess) e = block_alloc(reinterpret_cast<void**>(&g->mf32), sizeof(float4) * n_pad, st);
  if (e == hipSuccess)
    e = block_alloc(reinterpret_cast<void**>(&g->mfbox), sizeof(float4) * 2 * (n_pad / kMTile), st);
  if (e != hipSuccess) {  // all three or none (mf16 != nullptr marks the tiles as built)
    block_release(g->mf16);
    block_release(g->mf32);
    block_release(g->mfbox);
    g->mf16 = nullptr;
    g->mf32 = nullptr;
    g->mfbox = nullptr;
    return e;
  }
  g->mf_npad = n_pad;
  // Row order (private to nn_mfma_kernel: the exact path takes the original index from mf32.w):
  // the grid's row-major cell order, where a 1024-row tile is a thin z-slab, or Morton order of
  // the same cells, where it is a compact patch that fewer query boxes reach (M3D_NN_TILE_MORTON)
  pack16_sorted_kernel<<<(unsigned)((n_pad + 255) / 256), 256, 0, st>>>(
      g->pts, perm, c->xyz32, n, n_pad, (float)c->s16, g->mf16, g->mf32);
  // the target of a loop never moves: the boxes are built once per (cloud, cell size) and serve
  // every evaluation of every loop on this grid
  tile_box_kernel<<<(unsigned)(n_pad / kMTile), kMTile, 0, st>>>(g->mf32, g->mfbox);
  return hipGetLastError();  // asynchronous (stream order); m3d_icp_create synchronises once
}

#endif  // M3D_NN_TU_MAIN

// Self-seeding (single-device fused loop, m3d_icp_step): the fused tail of the previous
// iteration left every key at kKeyNone, so instead of a keyinit launch every block computes
// its queries' starting key itself (nnkey.h seed_key: the previous correspondence, exact — one
// target load per query) and the blocks of grid.y == 0 also publish it; the MIN over the
// blocks' atomics is the keyinit → scan result bit for bit.
// With seed records (on == 2: the fused tail left, per query, its correspondence's fp32 point and
// index, icp.hip terms_block) the key comes from the query's record, read beside src32[i] — the
// same fp32 operations on the same bits (nnkey.h seed_key_rec) without the dependent, random
// gather of tgt[prev[i]].  The records' pointer travels in `tgt`: a fifth member made the kernels
// spill (docs/EXPERIMENTS.md §R22).
struct SeedArgs {
  const int32_t* prev;  // corr of the previous evaluation
  const float4* tgt;    // the target cloud's centred fp32 points, original order; on == 2: the
                        // seed records in slot order instead (prev and nt unused)
  int64_t nt;           // its size
  int on;               // 0: keys[] holds the starting keys; 1: prev / tgt; 2: seed records
};

// Query i's seed record where the tail left none (sa.on == 1): the same record formed from prev /
// tgt (a previous correspondence outside the shard seeds nothing here: seed_key without dprev)
__device__ __forceinline__ float4 seed_rec_prev(const SeedArgs& sa, int64_t i, int64_t off) {
  const int64_t j = sa.prev[i];
  float4 r = make_float4(0.0f, 0.0f, 0.0f, __int_as_float(-1));
  if (j >= off && j < off + sa.nt) {
    r = sa.tgt[j - off];
    r.w = __int_as_float((int32_t)j);
  }
  return r;
}

// A block's place in the launch: slice y of the S slices of query block x (NnSlice, below)
struct NnSlice {
  unsigned x, y, S;
};
// The planned (1-D) launch of nn_mfma_kernel: the loop's table of `budget` entries and per query
// block tile counts (nn_plan.h), and the uniform assignment — nq query blocks × S slices, what
// nn_grid_y gives — for a loop state without a valid plan.  table = null: the 2-D launch.
struct NnPlan {
  const uint32_t* table;
  uint32_t* cnt;
  int nq, S;
};

// whether a block publishes its k1: it changed, or (self-seeding) the slice 0 blocks publish
// the seed every block started from
__device__ __forceinline__ bool publish_k1(const SeedArgs& sa, unsigned y, uint64_t k1, bool changed) {
  return changed || (sa.on && y == 0 && key_real(k1));
}

// Exact fallback of nn_mfma_kernel when the scaled operands do not fit fp16 (mfma_ok == 0, a
// far-off transform): the same scan state over the block's slice by a plain scan, one thread
// per query.
__device__ void nn_slice_scan(const float4* __restrict__ src32, int64_t ns, const float4* __restrict__ tgt32,
                              int64_t jb, int64_t je, int64_t off, const IcpState* __restrict__ s,
                              int64_t* __restrict__ keys, uint32_t* __restrict__ near2,
                              const SeedArgs& sa, int64_t q0, unsigned bsx, unsigned bsy) {
  const float* Rt = s->Rt32;
  const float r2_hi = s->r2_hi;
  for (int qs = threadIdx.x; qs < kMQueries; qs += kMBlock) {
    const int64_t slot = q0 + (int64_t)bsx * kMQueries + qs;
    if (slot >= ns) return;
    const int64_t i = slot;
    float qx, qy, qz;
    const float4 p = src32[i];
    xform32(Rt, p, qx, qy, qz);
    const int64_t key = sa.on == 0 ? keys[i]  // keyinit's starting key
                                   : seed_key_rec(s, sa.on == 2 ? sa.tgt[i] : seed_rec_prev(sa, i, off), qx, qy, qz);
    uint64_t k1 = key == kKeyNone ? make_key(r2_hi, 0xFFFFFFFFu) : (uint64_t)key;
    float k1d = key_real_d2(k1), n2 = kInf;
    const uint64_t k10 = k1;
    for (int64_t j = jb; j < je; ++j) {
      const float4 t = tgt32[j];
      if (__float_as_int(t.w) < 0) continue;  // pad
      const float d2 = d2f(qx, qy, qz, t.x, t.y, t.z);
      if (d2 <= r2_hi) near_push(k1, k1d, n2, make_key(d2, (uint32_t)(off + __float_as_int(t.w))), d2);
    }
    const bool pk = publish_k1(sa, bsy, k1, k1 != k10);
    if (pk || n2 < kInf) near_publish((unsigned long long*)&keys[i], &near2[i], k1, n2, pk);
  }
}

// 16 target rows (x, y, z, index bits) pushed into a query's scan state: direct d²
__device__ __forceinline__ void nn_push_rows(const float4 (&t)[16], int64_t off, float qx, float qy, float qz,
                                             float r2_hi, uint64_t& k1, float& k1d, float& n2) {
#pragma unroll
  for (int reg = 0; reg < 16; ++reg) {
    const float d2 = d2f(qx, qy, qz, t[reg].x, t[reg].y, t[reg].z);
    const uint64_t kc = make_key(d2, (uint32_t)(off + __float_as_int(t[reg].w)));
    if (d2 <= r2_hi) near_push(k1, k1d, n2, kc, d2);
  }
}

// Exact fp32 pass of nn_mfma_kernel over one flagged sub-tile (32 targets from `rows`), of which
// this lane takes its 16 MFMA rows: direct d² pushed into the lane's scan state.  Pads: far
// coordinates, d² ~ 1e36 > r2_hi.
__device__ __forceinline__ void nn_exact_rows(const float4* __restrict__ rows, int64_t off, int h,
                                              float qx, float qy, float qz, float r2_hi,
                                              uint64_t& k1, float& k1d, float& n2) {
  float4 t[16];  // all 16 loads in flight before the first use (one memory latency per sub-tile)
#pragma unroll
  for (int reg = 0; reg < 16; ++reg) t[reg] = rows[(reg & 3) + 8 * (reg >> 2) + 4 * h];
  nn_push_rows(t, off, qx, qy, qz, r2_hi, k1, k1d, n2);
}

__device__ __forceinline__ uint64_t shfl_xor64(uint64_t v, int m) {
  const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, m);
  const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), m);
  return ((uint64_t)hi << 32) | lo;
}

// OR of v over the wave's 64 lanes (all active), wave-uniform: DPP inside each row of 16 lanes,
// then the four rows by v_readlane.
__device__ __forceinline__ uint32_t wave_or32(uint32_t v) {
  int x = (int)v;
  x |= __builtin_amdgcn_mov_dpp(x, 0xB1, 0xF, 0xF, false);   // lane ^ 1
  x |= __builtin_amdgcn_mov_dpp(x, 0x4E, 0xF, 0xF, false);   // lane ^ 2
  x |= xor4_dpp(x);
  x |= __builtin_amdgcn_mov_dpp(x, 0x128, 0xF, 0xF, false);  // row_ror:8
  return (uint32_t)(__builtin_amdgcn_readlane(x, 0) | __builtin_amdgcn_readlane(x, 16) |
                    __builtin_amdgcn_readlane(x, 32) | __builtin_amdgcn_readlane(x, 48));
}

// min / max of v over the wave's 64 lanes (all active), wave-uniform: as wave_or32
template <bool kMax>
__device__ __forceinline__ float wave_minmax(float v) {
  const auto mm = [](float a, float b) { return kMax ? fmaxf(a, b) : fminf(a, b); };
  v = mm(v, __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0xB1, 0xF, 0xF, false)));
  v = mm(v, __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x4E, 0xF, 0xF, false)));
  v = mm(v, __int_as_float(xor4_dpp(__float_as_int(v))));
  v = mm(v, __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x128, 0xF, 0xF, false)));
  const int x = __float_as_int(v);
  return mm(mm(__int_as_float(__builtin_amdgcn_readlane(x, 0)), __int_as_float(__builtin_amdgcn_readlane(x, 16))),
            mm(__int_as_float(__builtin_amdgcn_readlane(x, 32)), __int_as_float(__builtin_amdgcn_readlane(x, 48))));
}

// Box cull of the brute-force sweep.  A set of queries is summarised by the box
// [lo, hi] of their fp32 coordinates and Xmax = the largest search bound X among them; a set of
// targets by the box of their fp32 coordinates (Grid::mfbox).  G = d2f(g, 0) with, per axis,
// g = max(0, qlo − thi, tlo − qhi) in fp32.
// Lemma: d2f(q, t) ≥ G for every q in the query box and t in the target box, with no epsilon.
//   * fp32 round-to-nearest is monotone: q − t ≥ qlo − thi in the reals gives fl(q − t) ≥
//     fl(qlo − thi), likewise fl(t − q) ≥ fl(tlo − qhi); so |fl(q − t)| ≥ g on each axis (g = 0
//     where the boxes overlap), and g − 0 is exact;
//   * d2f's chain fma(dz, dz, fma(dy, dy, dx·dx)) is monotone in |dx|, |dy|, |dz|: each step is a
//     monotone real function of non-negative arguments followed by one monotone rounding.
// So a target set with G > Xmax holds only targets with d2f > Xmax ≥ X of every query concerned.
// Such a target cannot become k1 (band_of(d) ≥ d, so X ≥ min(d2f(k1), r2_hi), and the exact path
// takes d2f ≤ r2_hi only), and it cannot put a value ≤ search_bound(final k1) into near2: X only
// ever tightens during the sweep (k1 only decreases, band_of is monotone), and near2 is only ever
// compared with search_bound of the final k1 (nnkey.h winner_fp64; the bound-only seeds of target
// shards reach X through the same search_bound).  Skipping the set therefore leaves every key and
// every ambiguous / unambiguous classification as the every-pair sweep has them; near2's value
// may differ only above the band.  The test is `G > Xmax`, strict: G = d2f = X is kept.  A NaN
// coordinate never enters a box: fminf / fmaxf in the lane, wave and tile_box_kernel reductions
// return the other operand.  That is harmless: a NaN point has no finite d2f, fails d2f ≤ r2_hi
// and can never be a neighbour, swept or not.  (Should G itself come out NaN, e.g. from
// inf − inf of an empty box, `G > Xmax` is false and the set is kept.)  M3D_NN_CULL=0 (A/B
// build) sweeps every pair as before.
// Second level, the per-query reach test (point_out_of_reach, M3D_NN_REACH=0 builds without it):
// the same lemma with the query box shrunk to one query's point q (qlo = qhi = q) and Xmax
// replaced by that query's own current bound X_q — every target t of the box has d2f(q, t) ≥
// G_q = d2f(max(0, q − thi, tlo − q), 0), so G_q > X_q puts the whole box out of this query's
// reach, now and for the rest of the sweep (X_q only tightens).  A wave keeps a half tile that
// passed its box test only if one of its active queries reaches it, a block keeps a tile only if
// one of its waves keeps one of its halves.  The queries run in Morton order: a wave or block that
// straddles a Morton jump has a box far larger than the space its points occupy, and the box test
// alone keeps everything in between.  Same strictness (G_q = X_q is kept), a NaN query or G_q
// keeps the half, inactive queries never reach, and `force` groups are tested like any other
// (the lemma is about d2f, not about the screen).
#ifndef M3D_NN_CULL
#define M3D_NN_CULL 1
#endif
#ifndef M3D_NN_REACH
#define M3D_NN_REACH 1
#endif
// the deferred exact passes in batches through LDS (nn_mfma_kernel, after the sweep); 0 (A/B
// builds): one sub-tile per global round trip, as before
// the entry's state words and plan table entry in one scalar round trip (nn_mfma_body); 0 (A/B
// builds): behind one another's branches, as before
#ifndef M3D_NN_ENTRY
#define M3D_NN_ENTRY 1
#endif
// the self-seeded scan reads the tail's seed records (launch_icp_nn); 0 (A/B builds): prev / tgt
#ifndef M3D_NN_SEED_REC
#define M3D_NN_SEED_REC 1
#endif
#ifndef M3D_NN_DEFER_BATCH
#define M3D_NN_DEFER_BATCH 1
#endif
// the batched deferred pass pushes only the rows the screen flags for the lane's own query
// (nn_defer_hits / nn_push_hits); 0 (A/B builds): every lane pushes all 16 of its rows
#ifndef M3D_NN_DEFER_FILTER
#define M3D_NN_DEFER_FILTER 1
#endif
// diagnostic builds only (tools/nn_clock.py): per-block timeline and tile counts of the last
// nn_mfma_kernel launch, s_memrealtime (100 MHz: one clock for every block, whichever XCD runs it)
#if M3D_NN_CLOCK
constexpr int kClkBlocks = 16384, kClkWords = 10;  // words 8, 9: nn_terms_handoff's stamps
__device__ unsigned long long g_nn_clock[kClkWords * kClkBlocks];
#endif
struct QBox {
  float lo[3], hi[3], X;
};
__device__ __forceinline__ bool box_out_of_reach(const QBox& q, const float4& tlo, const float4& thi) {
  const float gx = fmaxf(0.0f, fmaxf(q.lo[0] - thi.x, tlo.x - q.hi[0]));
  const float gy = fmaxf(0.0f, fmaxf(q.lo[1] - thi.y, tlo.y - q.hi[1]));
  const float gz = fmaxf(0.0f, fmaxf(q.lo[2] - thi.z, tlo.z - q.hi[2]));
  return d2f(gx, gy, gz, 0.0f, 0.0f, 0.0f) > q.X;
}
// the same test for one query point against a target box (lo, hi), X = the query's own bound
__device__ __forceinline__ bool point_out_of_reach(float qx, float qy, float qz, float X, const float (&lo)[3],
                                                   const float (&hi)[3]) {
  const float gx = fmaxf(0.0f, fmaxf(qx - hi[0], lo[0] - qx));
  const float gy = fmaxf(0.0f, fmaxf(qy - hi[1], lo[1] - qy));
  const float gz = fmaxf(0.0f, fmaxf(qz - hi[2], lo[2] - qz));
  return d2f(gx, gy, gz, 0.0f, 0.0f, 0.0f) > X;
}

// ------------------------------------------------------------------------------- nn_mfma_kernel
// Tiles of kTH × 256 targets in LDS, [buffer][lane half][target]: a half-wave's 32 ds_read_b128 hit
// 32 consecutive 16-B slots.  The sweep runs the tile in halves of 8 sub-tiles (8 A-operand
// registers live), one barrier per tile.  The fp32 coordinates are read from global memory by the
// (rare) exact path only.
constexpr int kTT = kTH * kMTile;  // targets per tile
constexpr int kSub = kTT / 32;     // sub-tiles per tile
constexpr uint64_t kGMask = (kSub == 64) ? ~0ull : ((1ull << kSub) - 1ull);
constexpr int kDefer = 16;  // deferred entries per wave (more: resolved in the tile as before)
static_assert(kMBlock == 2 * kMTile, "one 16-B operand half per thread per half tile");
static_assert(kSub * kMG <= 64, "hit mask holds every (group, sub-tile)");
static_assert(kSub == 32, "one 32-bit hit record per group and tile");
static_assert(kMBlock / 64 == 8, "eight wave boxes, lanes ^1 ^2 ^4");

// A lane's query of one 32-query group (column c of the group's MFMAs) and its scan state
struct QState {
  float qx, qy, qz, qq;  // exact-path coordinates, |q|²
  int64_t qi;            // position in the visit order, −1: none
  uint64_t k1;           // scan state (nnkey.h)
  float k1d, n2;
  half8 bq;              // B operand of the lane half: −2S·q split | threshold
};

// every sub-tile bit of the groups in `bits`, as a (group, sub-tile) mask
__device__ __forceinline__ uint64_t group_mask(uint32_t bits) {
  uint64_t m = 0;
#pragma unroll
  for (int g = 0; g < kMG; ++g)
    if ((bits >> g) & 1u) m |= kGMask << (g * kSub);
  return m;
}

// The query at position `slot` of the visit order ([q0, ns): order, or the slots themselves;
// beyond ns: inactive): transform, starting key, B operand without its threshold; an active
// query widens lq, the lane's share of its wave's query box (box_out_of_reach).  Returns the
// search bound X, −1 for an inactive query.  p = the query's source point and, self-seeding,
// rec = its seed record: the caller loads them for all of the lane's queries before the first
// use (an inactive query's are slot 0's, unused).
__device__ __forceinline__ float load_query(QState& q, QBox& lq, int64_t slot, int h, float4 p, float4 rec,
                                            int64_t ns, const IcpState* __restrict__ s, const SeedArgs& sa,
                                            const int64_t* __restrict__ keys) {
  const float* Rt = s->Rt32;
  const float r2_hi = s->r2_hi, S = s->mfma_scale;
  const int64_t i = slot < ns ? slot : -1;
  q.qi = i;
  q.n2 = kInf;
  float X = -1.0f;
  if (i >= 0) {
    xform32(Rt, p, q.qx, q.qy, q.qz);
    const int64_t key = sa.on ? seed_key_rec(s, rec, q.qx, q.qy, q.qz) : keys[i];
    q.k1 = key == kKeyNone ? make_key(r2_hi, 0xFFFFFFFFu) : (uint64_t)key;
    X = search_bound(key_d2(q.k1), s->band_e, r2_hi);
    lq.lo[0] = fminf(lq.lo[0], q.qx);
    lq.lo[1] = fminf(lq.lo[1], q.qy);
    lq.lo[2] = fminf(lq.lo[2], q.qz);
    lq.hi[0] = fmaxf(lq.hi[0], q.qx);
    lq.hi[1] = fmaxf(lq.hi[1], q.qy);
    lq.hi[2] = fmaxf(lq.hi[2], q.qz);
    lq.X = fmaxf(lq.X, X);
  } else {
    q.qx = q.qy = q.qz = 0.0f;
    q.k1 = (uint64_t)kKeyNone;
  }
  q.k1d = key_real_d2(q.k1);
  q.qq = fmaf(q.qz, q.qz, fmaf(q.qy, q.qy, q.qx * q.qx));
  _Float16 ah, al, bh, bl, ch, cl;
  split16(-2.0f * S * q.qx, ah, al);
  split16(-2.0f * S * q.qy, bh, bl);
  split16(-2.0f * S * q.qz, ch, cl);
  const _Float16 one = (_Float16)1.0f, zero = (_Float16)0.0f;
  q.bq = h == 0 ? half8{ah, al, ah, bh, bl, bh, ch, cl} : half8{ch, one, one, zero, zero, zero, zero, zero};
  return X;
}

// The query's threshold for search bound X (< 0: never hits) into its B operand (thr_operand);
// returns whether it exceeds the fp16 range.  Setup and after every exact pass: the threshold
// only ever tightens, so a group that was not `force` at setup never becomes it.
__device__ __forceinline__ bool refresh_threshold(QState& q, int h, float X, float eps, float S2) {
  bool fg;
  half8 bt = q.bq;
  thr_operand(bt, X < 0.0f ? -1.0f : ((X - q.qq) + eps) * S2, fg);  // × power of two: exact
  if (h == 1) q.bq = bt;
  return fg;
}

// The cull's query boxes (box_out_of_reach above): the box and Xmax of each wave's active queries
// by a DPP reduction, published in LDS as qbox[wave] = (lo.xyz, Xmax), (hi.xyz, ·); the block's
// box, returned in SGPRs, is their union: lane l takes wave l & 7's, three DPP steps merge the
// eight.  (The wave boxes stay in LDS and are read back by the rare survivor rounds: held in
// registers across the sweep they cost spills.)
__device__ __forceinline__ QBox reduce_boxes(const QBox& lq, float4 (&qbox)[kMBlock / 64][2], int lane, int wave) {
  float wlo[3], whi[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    wlo[k] = wave_minmax<false>(lq.lo[k]);
    whi[k] = wave_minmax<true>(lq.hi[k]);
  }
  const float wX = wave_minmax<true>(lq.X);
  if (lane == 0) {
    qbox[wave][0] = make_float4(wlo[0], wlo[1], wlo[2], wX);
    qbox[wave][1] = make_float4(whi[0], whi[1], whi[2], 0.0f);
  }
  __syncthreads();
  float4 lo = qbox[lane & 7][0], hi = qbox[lane & 7][1];
#pragma unroll
  for (int o = 1; o < 8; o <<= 1) {
    const auto x = [&](float v) { return __int_as_float(xor_lane(__float_as_int(v), o, kWave)); };
    lo = make_float4(fminf(lo.x, x(lo.x)), fminf(lo.y, x(lo.y)), fminf(lo.z, x(lo.z)), fmaxf(lo.w, x(lo.w)));
    hi = make_float4(fmaxf(hi.x, x(hi.x)), fmaxf(hi.y, x(hi.y)), fmaxf(hi.z, x(hi.z)), 0.0f);
  }
  const auto u = [](float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); };
  return QBox{{u(lo.x), u(lo.y), u(lo.z)}, {u(hi.x), u(hi.y), u(hi.z)}, u(lo.w)};
}

// The block's surviving tiles, in order.  The block skips, block-uniformly, every tile of its
// strided set (tc, tc + ty, …) none of whose half tiles its box can reach (no DMA, no sweep, no
// barrier); inside a surviving tile a wave sweeps only the half tiles its own box can reach.
// 16 tiles per round: lane l tests half tile l & 3 of tile tc + (l >> 2)·ty against both boxes
// (one round of box loads per 16 tiles).  mb: half tiles the block reaches — a tile survives if
// any of its four bits is set; mw ⊆ mb: those this wave reaches.  Every wave computes mb from the
// same data by the same instructions.
// Per-query reach test (M3D_NN_REACH, point_out_of_reach): mw is refined to the half tiles some
// active query of the wave reaches with its own current bound — the boxes are in the lanes that
// loaded them, a scalar loop over the set bits of mw broadcasts each with v_readlane and every
// lane tests its kMG queries — and mb becomes the OR of the eight waves' refined masks, through
// one LDS word per wave, in the rounds where the block's box reaches a tile at all.  The barrier this
// puts into such a round is legal: every wave reaches next() with the same (tc, mb) and takes the
// box-level mb from the same box, so all of them run the same rounds and the same barriers.  Two slot sets by round parity: a
// wave writes the set of round n + 2 only after the barrier of round n + 1, which every wave
// passes after it has read the set of round n.  Every wave ORs the same eight words: mb stays
// block-uniform.
struct ReachArgs {
  const QState (&q)[kMG];
  const uint32_t& act;  // the lane's active groups
  float be, r2_hi;
  uint64_t (&slot)[2][kMBlock / 64];
  int wave;
};
struct TileCursor {
  const float4* tbox;   // Grid::mfbox
  const float4* wbox;   // this wave's box, qbox[wave] (LDS)
  QBox bx;              // the block's box
  int lane, ntile, ty;  // tiles in all, the set's stride (the query block's slices S)
  int tc;               // first tile of the current round
  uint64_t mb, mw;
  int par = 0;          // parity of the round (ReachArgs::slot)

  __device__ __forceinline__ void cull_round(const ReachArgs& ra) {
    const int tl = tc + (lane >> 2) * ty;
    bool kb = tl < ntile, kw = kb;
    float4 tlo = make_float4(0.0f, 0.0f, 0.0f, 0.0f), thi = tlo;
    if (M3D_NN_CULL && kb) {
      const int64_t hb = (int64_t)tl * kTH + (lane & 3);  // < nt_pad / kMTile
      tlo = tbox[2 * hb];
      thi = tbox[2 * hb + 1];
      const float4 l0 = wbox[0], u0 = wbox[1];
      const QBox wq{{l0.x, l0.y, l0.z}, {u0.x, u0.y, u0.z}, l0.w};
      kb = !box_out_of_reach(bx, tlo, thi);
      kw = !box_out_of_reach(wq, tlo, thi);
    }
    mb = __ballot(kb);
    mw = __ballot(kw);
#if M3D_NN_CULL && M3D_NN_REACH
    // a round the block's box reaches nothing of (mb from the block's box: block-uniform) needs no
    // second level, no exchange and no barrier — with grid.y = 1 on a large target most rounds
    if (mb == 0) return;
    float X[kMG];
#pragma unroll
    for (int g = 0; g < kMG; ++g)
      X[g] = (ra.act >> g) & 1u ? search_bound(key_d2(ra.q[g].k1), ra.be, ra.r2_hi) : -1.0f;
    uint64_t keep = 0;
    for (uint64_t m = mw; m != 0; m &= m - 1) {
      const int b = __builtin_amdgcn_readfirstlane(__builtin_ctzll(m));
      const auto rl = [&](float v) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), b)); };
      const float lo[3] = {rl(tlo.x), rl(tlo.y), rl(tlo.z)}, hi[3] = {rl(thi.x), rl(thi.y), rl(thi.z)};
      bool reach = false;
#pragma unroll
      for (int g = 0; g < kMG; ++g)
        reach |= ((ra.act >> g) & 1u) &&
                 !point_out_of_reach(ra.q[g].qx, ra.q[g].qy, ra.q[g].qz, X[g], lo, hi);
      if (__any(reach)) keep |= 1ull << b;
    }
    mw = keep;
    par ^= 1;
    if (lane == 0) ra.slot[par][ra.wave] = mw;
    __syncthreads();
    const uint64_t w = ra.slot[par][lane & 7];
    int wl = (int)(uint32_t)w, wh = (int)(uint32_t)(w >> 32);
#pragma unroll
    for (int o = 1; o < 8; o <<= 1) {
      wl |= xor_lane(wl, o, kWave);
      wh |= xor_lane(wh, o, kWave);
    }
    mb = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane(wh) << 32) |
         (uint32_t)__builtin_amdgcn_readfirstlane(wl);
#endif
  }
  // next surviving tile (ntile: none left) and this wave's half-tile mask of it
  __device__ __forceinline__ void next(int& t, uint32_t& hmask, const ReachArgs& ra) {
    for (;;) {
      if (mb != 0) {
        const int k = __builtin_ctzll(mb) >> 2;
        t = tc + k * ty;
        hmask = (uint32_t)(mw >> (4 * k)) & 15u;
        mb &= ~(15ull << (4 * k));
        return;
      }
      tc += 16 * ty;
      if (tc >= ntile) {
        t = ntile;
        hmask = 0;
        return;
      }
      cull_round(ra);
    }
  }
};

// Tile t's operands global → LDS: thread x stages kTH elements e = x + u·512, plane e / kTT,
// target e % kTT (mf16 is stored as two planes, so the loads are coalesced).  dma: by LDS DMA
// (lds_dma.h), no prefetch registers — a wave's 64 elements are one plane's 64 consecutive
// targets; the caller retires it with lds_dma_wait().
__device__ __forceinline__ void stage_tile(uint4 (&dst)[2][kTT], const uint4* __restrict__ tgt16,
                                           int64_t nt_pad, int t, bool dma) {
#pragma unroll
  for (int u = 0; u < kTH; ++u) {
    const int e = threadIdx.x + u * kMBlock;
    const uint4* src = tgt16 + (e / kTT) * nt_pad + (int64_t)t * kTT + e % kTT;
    if (dma)
      lds_dma16(src, &dst[e / kTT][(e % kTT) & ~63]);
    else
      dst[e / kTT][e % kTT] = *src;
  }
}

// Sweep of one tile: MFMA + sign-OR test for the tile's sub-tiles, branch-free.  A step records
// its sign bit in the lane's own shift register of its group (v_alignbit: rec = rec << 1 | sign),
// so the step is vector instructions only; the wave looks at the records once per tile
// (hit_mask).  Software-pipelined: the MFMA of step t+1 is issued before step t's tree, so a wave
// never waits on its own MFMA.  hmask: the half tiles this wave's box reaches.
__device__ __forceinline__ void sweep_tile(uint32_t (&rec)[kMG], const uint4 (&t16)[2][2][kTT], int buf,
                                           int h, int c, uint32_t hmask, const QState (&q)[kMG],
                                           const floatx16& zacc) {
#pragma unroll
  for (int g = 0; g < kMG; ++g) rec[g] = 0;
  constexpr int kSteps = 8 * kMG;  // (sub-tile, group) steps of one half tile
#pragma unroll
  for (int half = 0; half < kTH; ++half) {
    // a half tile out of this wave's reach (wave-uniform: a scalar branch): its 8 steps' bits
    // are zeros, so that bfrev / ctz still address the sub-tiles
    if (!((hmask >> half) & 1u)) {
#pragma unroll
      for (int g = 0; g < kMG; ++g) rec[g] <<= 8;
      continue;
    }
    H8 av[8];
#pragma unroll
    for (int sub = 0; sub < 8; ++sub) av[sub].u = t16[buf][h][half * kMTile + sub * 32 + c];
    floatx16 kc = __builtin_amdgcn_mfma_f32_32x32x16_f16(av[0].h, q[0].bq, zacc, 0, 0, 0);
#pragma unroll
    for (int t = 0; t < kSteps; ++t) {
      floatx16 kn;
      if (t + 1 < kSteps)
        kn = __builtin_amdgcn_mfma_f32_32x32x16_f16(av[(t + 1) / kMG].h, q[(t + 1) % kMG].bq, zacc, 0, 0, 0);
      // keep the pipeline the source states: without this fence the scheduler sinks each
      // MFMA next to its consumer (same accumulator registers, the VALU then waits out the
      // whole MFMA latency every step and the matrix pipe idles under the tree)
      __builtin_amdgcn_sched_barrier(0);
      // a candidate's value is strictly negative: OR of the 16 bit patterns, test bit 31
      rec[t % kMG] = __builtin_amdgcn_alignbit(rec[t % kMG], or16(kc), 31);
      __builtin_amdgcn_sched_barrier(0);
      if (t + 1 < kSteps) kc = kn;
    }
  }
}

// One wave-level test per tile (hits are rare): only a tile with a hit ORs the records over the
// wave into the (group, sub-tile) mask.  Sub-tile 0 was pushed first: bit 31, hence bfrev.
// `force` groups (force64) add every sub-tile of the half tiles swept (the lemma is about d2f).
__device__ __forceinline__ uint64_t hit_mask(const uint32_t (&rec)[kMG], uint32_t hmask, uint64_t force64) {
  uint64_t hm = 0;
  uint32_t any = rec[0];
#pragma unroll
  for (int g = 1; g < kMG; ++g) any |= rec[g];
  if (__any(any != 0)) {
#pragma unroll
    for (int g = 0; g < kMG; ++g) hm |= (uint64_t)wave_or32(__builtin_bitreverse32(rec[g])) << (g * kSub);
  }
  uint32_t sm = 0;
#pragma unroll
  for (int half = 0; half < kTH; ++half)
    if ((hmask >> half) & 1u) sm |= 0xFFu << (8 * half);
  uint64_t fm = 0;
#pragma unroll
  for (int g = 0; g < kMG; ++g) fm |= (uint64_t)sm << (g * kSub);
  return hm | (force64 & fm);
}

// Exact path for one group's flagged sub-tiles mg of the tile whose rows start at `tile`, every
// lane (exact for any lane): direct fp32 d² over the lane's 16 rows, then the lane pair
// (c, c + 32) merges its two states.  Returns whether k1 changed.
__device__ __forceinline__ bool nn_exact_subtiles(uint64_t mg, const float4* __restrict__ tile, int64_t off,
                                                  int h, float r2_hi, QState& q) {
  const uint64_t kb = q.k1;
  while (mg != 0) {
    const int sub = __builtin_ctzll(mg);
    mg &= mg - 1;
    nn_exact_rows(tile + sub * 32, off, h, q.qx, q.qy, q.qz, r2_hi, q.k1, q.k1d, q.n2);
    const uint64_t o1 = shfl_xor64(q.k1, 32);
    const float on2 = __shfl_xor(q.n2, 32);
    near_merge(q.k1, q.k1d, q.n2, o1, on2);
  }
  return q.k1 != kb;
}

// Filtered deferred pass (M3D_NN_DEFER_FILTER): of a flagged sub-tile a lane pushes only the rows
// the screen flags for its own query, instead of all 16 (cfg1 model, tools/nn_defer_model.py: the
// lane with the most hits has 2.1 at the mean, 6 at most).  nn_defer_hits runs the sub-tile's
// screen again — the sweep's MFMA on the same operands: `a` is the sub-tile's A operand from mf16,
// bq the group's current B operand — and returns the signs of the lane's 16 values, bit reg =
// value reg (the sweep's v_alignbit record, fed from 15 down so that no bfrev is needed);
// nn_push_hits walks the set bits, each lane its own, and reads row (reg & 3) + 8·(reg >> 2) + 4·h
// of the sub-tile from the LDS stash — the row register `reg` of nn_exact_rows holds — by a
// computed address (a register array indexed per lane would go to scratch).  A lane without bits
// left is masked; the loop ends when no lane of the wave has one.
// The result does not change:
//  1. a deferred group's bq carries the threshold of a bound X_q the query had at setup or at a
//     later in-tile refresh (refresh_threshold); the bound only tightens (k1 only decreases,
//     band_of is monotone), so X_q ≥ search_bound of the query's final k1;
//  2. thr_operand makes the screen value strictly negative for every target with d2f ≤ X_q,
//     whatever the MFMA's accumulation order (screen_eps_m plus the threshold terms' own share);
//  3. so the rows pushed are a superset of the targets with d2f ≤ search_bound(final k1);
//  4. k1 is the same: the minimum over the sub-tile lies inside the bound whenever it beats the
//     seed, and ties go to the lower index through the same key order; the seed's own target is
//     flagged and pushed, meets kc == k1 in near_push and counts once;
//  5. near2 falls at or below the band exactly when it does with all rows pushed; its stored value
//     may differ only above the band, where winner_fp64 does not look (it compares near2 with
//     search_bound(final k1) only) — the freedom the cull lemma already takes (box_out_of_reach).
// An inactive lane's query is the origin with threshold −1: its values are positive, its mask empty
// (and its state is never published).
__device__ __forceinline__ uint32_t nn_defer_hits(const half8& a, const half8& bq, const floatx16& zacc) {
  const floatx16 v = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, bq, zacc, 0, 0, 0);
  uint32_t m = 0;
#pragma unroll
  for (int reg = 15; reg >= 0; --reg) m = __builtin_amdgcn_alignbit(m, __float_as_uint(v[reg]), 31);
  return m;
}
__device__ __forceinline__ void nn_push_hits(uint32_t m, const float4* rows, int64_t off, int h, float qx,
                                             float qy, float qz, float r2_hi, uint64_t& k1, float& k1d,
                                             float& n2) {
  while (m != 0) {
    const int reg = __builtin_ctz(m);
    m &= m - 1;
    const float4 t = rows[(reg & 3) + 8 * (reg >> 2) + 4 * h];
    // branch-free (push_within): a flagged row is nearly always within r2_hi, and under a branch the
    // row's index would be a second, dependent LDS read
    push_within(k1, k1d, n2, d2f(qx, qy, qz, t.x, t.y, t.z), r2_hi, (uint32_t)(off + __float_as_int(t.w)));
  }
}

#if M3D_NN_TU_TERMS_KERNEL
// The per-query-block hand-off of nn_mfma_terms_kernel (DESIGN.md §3.6 "Hand-off", once per query
// block instead of once per launch).  A block calls it after its publish — agent-scope atomics on
// keys and near2 — and its count: every wave drains its own (vmcnt(0)), the block meets at a
// barrier, one lane adds to the query block's ticket.  The block whose add returns S − 1 is the
// last of the query block's S slices: every other slice's publish was drained before its add, so
// the keys are final, and this block runs the query block's terms pass right here — terms_block
// with sc1 loads of keys and near2 — exactly what block x of the fused tail's terms phase does:
// partial x (write-through), corr, seed records, pcd64, keys handed back as kKeyNone.  Then it
// clears the ticket for the next launch (nothing else adds to it in this one).  No block waits for
// another: the last adder does the work.
// clk (clock builds; null: none): the block's record — word 8 the ticket's return, word 9 the end
// of the terms pass where the block ran it, else 0.
__device__ __forceinline__ void nn_terms_handoff(const NnTermsDev* __restrict__ td, const IcpState* __restrict__ s,
                                                 unsigned x, unsigned S, unsigned long long* clk = nullptr) {
  __shared__ uint32_t tk_last;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t t = __hip_atomic_fetch_add(&td->tix[x], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    tk_last = t == S - 1u ? 1u : 0u;
#if M3D_NN_CLOCK
    if (clk != nullptr) {
      clk[8] = __builtin_amdgcn_s_memrealtime();
      clk[9] = 0;
    }
#endif
  }
  __syncthreads();
  if (!tk_last) return;
  terms_block<true, M3D_EST_POINT_TO_PLANE, true>(td->a, s, td->partials, x);
  if (threadIdx.x == 0) __hip_atomic_store(&td->tix[x], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#if M3D_NN_CLOCK
  if (clk != nullptr && threadIdx.x == 0) clk[9] = __builtin_amdgcn_s_memrealtime();
#endif
}
#endif

// The body of the two NN kernels below.  kPlan = false is nn_mfma_kernel, the 2-D launch: the
// block's slice is (blockIdx.x, blockIdx.y) of gridDim.y, from the hardware at every use, and none
// of the plan's code is in it — no table, no LDS word, no counter: the launches the plan does not
// apply to (the 1M source: 1954 query blocks; any grid.x) run the code they ran before the plan.
// kPlan = true is nn_mfma_plan_kernel, the 1-D launch of pl.budget blocks (at most kPlanMaxQ
// query blocks: x fits the 16 bits of a table entry and of the LDS word).
// kTerms (with kPlan) is nn_mfma_terms_kernel: the planned body, and at both of its ends — the
// publish and the plain scan — nn_terms_handoff; td = its NnTermsDev (null otherwise).
template <bool kPlan, bool kTerms = false>
__device__ __forceinline__ void nn_mfma_body(const float4* __restrict__ src32, int64_t ns,
                                             const uint4* __restrict__ tgt16, const float4* __restrict__ tgt32,
                                             const float4* __restrict__ tbox, int64_t nt_pad, int64_t off,
                                             const IcpState* __restrict__ s, int64_t* __restrict__ keys,
                                             uint32_t* __restrict__ near2, const SeedArgs& sa, int64_t q0,
                                             const NnPlan& pl, const void* td = nullptr) {
#if M3D_NN_ENTRY
  // One scalar round trip at entry: the block's table entry (the launch has exactly the table's
  // pl.budget blocks: blockIdx.x is in range whatever the state says) and the state words that
  // decide the block's path are loaded together and selected afterwards, instead of each behind
  // the previous one's branch.
  uint32_t e_tab = kPlanEmpty;
  if (kPlan && pl.table != nullptr) e_tab = pl.table[blockIdx.x];
  int32_t st_done = s->done, st_plan = s->plan_ok, st_mfma = s->mfma_ok;
  // (through an empty asm: or the compiler sinks each load back behind the branch that uses it)
  asm volatile("" : "+s"(st_done), "+s"(st_plan), "+s"(st_mfma), "+s"(e_tab));
  if (st_done) return;
#else
  if (s->done) return;
#endif
#if M3D_NN_CLOCK
  const unsigned long long clk0 = __builtin_amdgcn_s_memrealtime();
#endif
  // The block's slice.  2-D launch: block (x, y) of grid (query blocks, S).
  // 1-D launch of pl.budget blocks: the loop's plan table entry (IcpState::plan_ok; one scalar
  // load, the round trip of s->done), or without a valid plan the uniform assignment the 2-D
  // launch has — y = b / nq, x = b % nq, S = pl.S; an empty entry, or y ≥ S, has nothing to do.
  NnSlice bs{0u, 0u, 0u};  // (2-D launch: unused — the hardware's values at every use, as before the plan)
  if (kPlan && pl.table != nullptr) {
#if M3D_NN_ENTRY
    if (st_plan) {
      const uint32_t e = e_tab;
#else
    if (s->plan_ok) {
      const uint32_t e = pl.table[blockIdx.x];
#endif
      if (e == kPlanEmpty) return;
      bs = NnSlice{plan_x(e), plan_y(e), plan_S(e)};
    } else {
      const unsigned y = blockIdx.x / (unsigned)pl.nq;
      if (y >= (unsigned)pl.S) return;
      bs = NnSlice{blockIdx.x - y * (unsigned)pl.nq, y, (unsigned)pl.S};
    }
  }
  // slice y takes every S-th target tile (strided: a query block's few candidate tiles, adjacent
  // in row order, spread over its S blocks instead of landing in one)
#if M3D_NN_ENTRY
  if (!st_mfma) {  // the same tiles by a plain scan, unculled
#else
  if (!s->mfma_ok) {  // the same tiles by a plain scan, unculled
#endif
    const int64_t tstep = (int64_t)(kPlan ? bs.S : gridDim.y) * kTT;
    for (int64_t t0 = (int64_t)(kPlan ? bs.y : blockIdx.y) * kTT; t0 < nt_pad; t0 += tstep)
      nn_slice_scan(src32, ns, tgt32, t0, min(nt_pad, t0 + kTT), off, s, keys, near2, sa, q0,
                    kPlan ? bs.x : blockIdx.x, kPlan ? bs.y : blockIdx.y);
#if M3D_NN_TU_TERMS_KERNEL
    if constexpr (kTerms) nn_terms_handoff(static_cast<const NnTermsDev*>(td), s, bs.x, bs.S);
#endif
    return;
  }
  __shared__ uint4 t16[2][2][kTT];
  __shared__ uint64_t dlist[kMBlock / 64][kDefer];  // deferred: flagged (group, sub-tile) bits
  __shared__ uint32_t dtile[kMBlock / 64][kDefer];  // their tile's first target
  __shared__ float4 qbox[kMBlock / 64][2];
  __shared__ uint64_t rslot[2][kMBlock / 64];  // the waves' refined half masks of a cull round
#if M3D_NN_CLOCK
  __shared__ uint32_t clk_slow, clk_ticket;  // half tiles swept by the block's slowest wave
  __shared__ unsigned long long clk_exit;
  if (threadIdx.x == 0) {  // (visible after the boxes' barrier)
    clk_slow = 0;
    clk_ticket = 0;
    clk_exit = 0;
  }
  uint32_t clk_halves = 0;
#endif
  // tiles the block kept (block-uniform): the planner's count, and its parity the LDS buffer
  uint32_t kept = 0;
  // (x, y) again at the publish, from LDS: held in SGPRs across the sweep they cost spills
  __shared__ uint32_t slice_xy;
  // (kTerms: and S, for the hand-off — the table entry's own layout, nn_plan.h)
  if (kPlan && threadIdx.x == 0) slice_xy = bs.x | (bs.y << 16) | (kTerms ? bs.S << 24 : 0u);  // (visible after the boxes' barrier)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = lane & 31, h = lane >> 5;
  const float r2_hi = s->r2_hi, eps = s->screen_eps_m, S = s->mfma_scale, be = s->band_e;
  const float S2 = S * S;

  // queries: per-group state, the lane's box share, group masks
  QState q[kMG];
  uint32_t act = 0;    // groups whose query (column c) exists
  uint32_t force = 0;  // groups whose threshold exceeds the fp16 range: exact path everywhere
  uint32_t chg = 0;    // groups whose k1 left its starting key (k1 only ever decreases)
  QBox lq{{kInf, kInf, kInf}, {-kInf, -kInf, -kInf}, -1.0f};
  const int64_t slot0 = q0 + (kPlan ? (int64_t)bs.x : (int64_t)blockIdx.x) * kMQueries + wave * kMG * 32 + c;
  // source points and seed records of all the lane's queries in flight before the first use: one
  // round trip, not one per group (an inactive query loads slot 0's, unused)
  float4 qp[kMG], qr[kMG];
#pragma unroll
  for (int g = 0; g < kMG; ++g) {
    const int64_t slot = slot0 + g * 32;
    qp[g] = src32[slot < ns ? slot : 0];
    qr[g] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  }
  if (sa.on == 2) {
#pragma unroll
    for (int g = 0; g < kMG; ++g) {
      const int64_t slot = slot0 + g * 32;
      qr[g] = sa.tgt[slot < ns ? slot : 0];
    }
  } else if (sa.on) {
#pragma unroll
    for (int g = 0; g < kMG; ++g) {
      const int64_t slot = slot0 + g * 32;
      qr[g] = seed_rec_prev(sa, slot < ns ? slot : 0, off);
    }
  }
#pragma unroll
  for (int g = 0; g < kMG; ++g) {
    const int64_t slot = slot0 + g * 32;
    const float X = load_query(q[g], lq, slot, h, qp[g], qr[g], ns, s, sa, keys);
    if (q[g].qi >= 0) act |= 1u << g;
    if (__any(refresh_threshold(q[g], h, X, eps, S2))) force |= 1u << g;
  }
  const floatx16 zacc = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f,
                         0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  // Deferred exact passes: a group whose every query starts from a real seed already screens
  // with (nearly) its final threshold, so its flagged sub-tiles need not be resolved inside the
  // tile — where one wave's exact pass holds the block's other 7 waves at the tile barrier —
  // but can wait in a per-wave list (tile offset, flagged bits) until after the sweep (−2.2 %
  // per launch at cfg1).  The candidates evaluated are the same sub-tiles' rows, so
  // the key is the same.  Unseeded groups and a full list resolve in the tile, where the
  // threshold refresh still prunes the rest of the sweep.
  uint32_t dfr = 0;
#pragma unroll
  for (int g = 0; g < kMG; ++g)
    if (!((force >> g) & 1u) && __all(q[g].qi < 0 || key_real(q[g].k1))) dfr |= 1u << g;
  int dn = 0;
  uint64_t dmask = group_mask(dfr);
  dmask = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(dmask >> 32)) << 32) |
          (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)dmask);  // wave-uniform: SGPRs

  const QBox bx = reduce_boxes(lq, qbox, lane, wave);
  const int ntile = (int)(nt_pad / kTT);
  const ReachArgs ra{q, act, be, r2_hi, rslot, wave};
  TileCursor cur{tbox, qbox[wave], bx, lane, ntile, (int)(kPlan ? bs.S : gridDim.y), (int)(kPlan ? bs.y : blockIdx.y), 0, 0};
  cur.cull_round(ra);
  int t0, t1;
  uint32_t h0, h1;  // the wave's half-tile masks of tiles t0, t1
  cur.next(t0, h0, ra);
  if (t0 < ntile) stage_tile(t16[0], tgt16, nt_pad, t0, false);
  const uint64_t force64 = group_mask(force);
  __syncthreads();
#if M3D_NN_CLOCK
  const unsigned long long clk1 = __builtin_amdgcn_s_memrealtime();
#endif
  int tog = 0;
  for (; t0 < ntile; t0 = t1, h0 = h1) {
    const int buf = kPlan ? (int)(kept & 1u) : tog;
    const int64_t j0 = (int64_t)t0 * kTT;
    if (kPlan || M3D_NN_CLOCK) ++kept;
#if M3D_NN_CLOCK
    clk_halves += (uint32_t)__builtin_popcount(h0);
#endif
    cur.next(t1, h1, ra);
    // the next surviving tile while this one is swept
    if (t1 < ntile) stage_tile(t16[buf ^ 1], tgt16, nt_pad, t1, true);
    uint32_t rec[kMG];
    sweep_tile(rec, t16, buf, h, c, h0, q, zacc);
    uint64_t hm = hit_mask(rec, h0, force64);
    const uint64_t hd = hm & dmask;
    if (hd != 0 && dn < kDefer) {
      if (lane == 0) {
        dlist[wave][dn] = hd;
        dtile[wave][dn] = (uint32_t)j0;
      }
      ++dn;
      hm &= ~hd;
    }
#pragma unroll
    for (int g = 0; g < kMG; ++g) {
      const uint64_t mg = (hm >> (g * kSub)) & kGMask;
      if (mg == 0) continue;
      chg |= (uint32_t)nn_exact_subtiles(mg, tgt32 + j0, off, h, r2_hi, q[g]) << g;
      refresh_threshold(q[g], h, (act >> g) & 1u ? search_bound(key_d2(q[g].k1), be, r2_hi) : -1.0f, eps, S2);
    }
    lds_dma_wait();
    __syncthreads();
    if (!kPlan) tog ^= 1;
  }
#if M3D_NN_CLOCK
  const unsigned long long clk2 = __builtin_amdgcn_s_memrealtime();
  if (lane == 0) atomicMax(&clk_slow, clk_halves);
#endif
  // The deferred exact passes.  The tiles have left LDS and the fp32 rows come from global memory:
  // one sub-tile at a time that is one dependent round trip per flagged sub-tile, and the slowest
  // wave's list is what a block spends most of its life on (tools/nn_clock.py: 11 of 25 µs at
  // cfg1).  So the wave fetches its flagged sub-tiles kStash at a time — a lane loads one row of
  // eight of them, all in flight together — into its own eighth of the operand buffers (free:
  // the loop's last barrier is behind every wave) and runs the exact pass from there.  Per group
  // the rows are pushed in the same order as before, each by the lane that would have pushed it;
  // the lane pair merges once at the end instead of after every sub-tile, which gives the same
  // state: (k1, near2) is a function of the set of keys pushed — the minimum and the smallest d²
  // of any other; a key held by both lanes (the seed, an earlier merge) counts once (near_push).
  // Filtered (M3D_NN_DEFER_FILTER, the default): of a slot's rows a lane pushes only those the
  // screen, run again for the slot, flags for its own query (nn_defer_hits: why that is the same
  // result) — the pushes of all 16 rows by every lane were most of the phase (tools/nn_clock.py:
  // 11.8 → 5.7 µs mean at cfg1, EXPERIMENTS §R12).  Batches of 8, A operands in registers.
#if M3D_NN_DEFER_BATCH
  if (dn > 0) {
#if M3D_NN_DEFER_FILTER
    // filtered (nn_defer_hits): 8 sub-tiles per batch — with the fp32 rows a lane loads the A
    // operand of each of the batch's sub-tiles (4 registers a slot), all in one round trip
    constexpr int kStash = 8;
#else
    constexpr int kStash = 16;  // sub-tiles per batch: 16 × 32 rows × 16 B = 8 KiB per wave
#endif
    static_assert(kStash * kMG <= 32, "a batch's group flags in one word");
    static_assert(sizeof(t16) >= sizeof(float4) * (kMBlock / 64) * kStash * 32, "a stash per wave");
    float4* const stash = reinterpret_cast<float4*>(&t16[0][0][0]) + wave * (kStash * 32);
    const auto uni = [](uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); };
    // cursor over the list's flagged (entry, sub-tile) pairs, wave-uniform
    int e = 0;
    uint64_t ent = dlist[wave][0];
    ent = ((uint64_t)uni((uint32_t)(ent >> 32)) << 32) | uni((uint32_t)ent);
    uint32_t base = uni(dtile[wave][0]);
    const auto subs = [](uint64_t m) {
      uint32_t u = 0;
#pragma unroll
      for (int g = 0; g < kMG; ++g) u |= (uint32_t)(m >> (g * kSub)) & (uint32_t)kGMask;
      return u;
    };
    uint32_t U = subs(ent);
    // next pair: its first row and the groups that flagged it (0: the list is exhausted)
    const auto pop = [&](uint32_t& row0, uint32_t& gs) {
      row0 = 0;
      gs = 0;
      while (U == 0) {
        if (e + 1 >= dn) return;
        ++e;
        ent = dlist[wave][e];
        ent = ((uint64_t)uni((uint32_t)(ent >> 32)) << 32) | uni((uint32_t)ent);
        base = uni(dtile[wave][e]);
        U = subs(ent);
      }
      const int sub = __builtin_ctz(U);
      U &= U - 1;
      row0 = base + (uint32_t)sub * 32u;
#pragma unroll
      for (int g = 0; g < kMG; ++g) gs |= (uint32_t)((ent >> (g * kSub + sub)) & 1u) << g;
    };
    uint64_t kb[kMG];
#pragma unroll
    for (int g = 0; g < kMG; ++g) kb[g] = q[g].k1;
    for (;;) {
      uint32_t gsel = 0;  // kMG bits per stash slot
      float4 ld[kStash / 2];
#if M3D_NN_DEFER_FILTER
      H8 av[kStash];  // the slots' A operands (an empty slot: row 0's, unused)
#endif
#pragma unroll
      for (int k = 0; k < kStash / 2; ++k) {  // slots 2k (lanes 0–31) and 2k + 1 (lanes 32–63)
        uint32_t ra, ga, rb, gb;
        pop(ra, ga);
        pop(rb, gb);
        gsel |= (ga | (gb << kMG)) << (2 * kMG * k);
        ld[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (h == 0 ? ga != 0 : gb != 0) ld[k] = tgt32[(int64_t)(h == 0 ? ra : rb) + c];  // < nt_pad
#if M3D_NN_DEFER_FILTER
        av[2 * k].u = tgt16[(int64_t)h * nt_pad + ra + c];  // row0 + c < nt_pad
        av[2 * k + 1].u = tgt16[(int64_t)h * nt_pad + rb + c];
#endif
      }
#pragma unroll
      for (int k = 0; k < kStash / 2; ++k) stash[(2 * k + h) * 32 + c] = ld[k];
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#if M3D_NN_DEFER_FILTER
#pragma unroll
      for (int sl = 0; sl < kStash; ++sl) {  // (unrolled: av[sl] stays in registers)
        const uint32_t gs = (gsel >> (kMG * sl)) & ((1u << kMG) - 1u);
        if (gs == 0) break;  // the slots fill in order
        uint32_t hit[kMG];
#pragma unroll
        for (int g = 0; g < kMG; ++g) hit[g] = (gs >> g) & 1u ? nn_defer_hits(av[sl].h, q[g].bq, zacc) : 0u;
#pragma unroll
        for (int g = 0; g < kMG; ++g)
          if ((gs >> g) & 1u)
            nn_push_hits(hit[g], stash + sl * 32, off, h, q[g].qx, q[g].qy, q[g].qz, r2_hi, q[g].k1, q[g].k1d,
                         q[g].n2);
      }
#else
#pragma unroll 1
      for (int sl = 0; sl < kStash; ++sl) {
        const uint32_t gs = (gsel >> (kMG * sl)) & ((1u << kMG) - 1u);
        if (gs == 0) break;  // the slots fill in order
        float4 t[16];
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) t[reg] = stash[sl * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * h];
#pragma unroll
        for (int g = 0; g < kMG; ++g)
          if ((gs >> g) & 1u) nn_push_rows(t, off, q[g].qx, q[g].qy, q[g].qz, r2_hi, q[g].k1, q[g].k1d, q[g].n2);
      }
#endif
      if (U == 0 && e + 1 >= dn) break;
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();  // the next batch overwrites the stash
    }
#pragma unroll
    for (int g = 0; g < kMG; ++g) {
      const uint64_t o1 = shfl_xor64(q[g].k1, 32);
      const float on2 = __shfl_xor(q[g].n2, 32);
      near_merge(q[g].k1, q[g].k1d, q[g].n2, o1, on2);
      chg |= (uint32_t)(q[g].k1 != kb[g]) << g;
    }
  }
#else
  for (int e = 0; e < dn; ++e) {
    const uint64_t ent = dlist[wave][e];
    const float4* tile = tgt32 + (int64_t)dtile[wave][e];
#pragma unroll
    for (int g = 0; g < kMG; ++g)
      chg |= (uint32_t)nn_exact_subtiles((ent >> (g * kSub)) & kGMask, tile, off, h, r2_hi, q[g]) << g;
  }
#endif
#if M3D_NN_CLOCK
  const unsigned long long clk2b = __builtin_amdgcn_s_memrealtime();
#endif
  const uint32_t sxy = kPlan ? slice_xy : 0u;
  const int64_t sxl = (int64_t)(sxy & 0xFFFFu);
  const unsigned syl = kTerms ? (sxy >> 16) & 0xFFu : sxy >> 16;
// (macros, not values: the 2-D kernel reads the hardware's coordinates at each use, as before)
#define M3D_NN_SX (kPlan ? sxl : (int64_t)blockIdx.x)
#define M3D_NN_SY (kPlan ? syl : blockIdx.y)
#pragma unroll
  for (int g = 0; g < kMG; ++g) {
    if (h != 0 || q[g].qi < 0) continue;
#if (M3D_NN_CULL && M3D_NN_REACH) || M3D_NN_DEFER_BATCH
    // the query's position again from the block's coordinates (through an empty asm, or the
    // compiler keeps the value of the setup): held across the sweep it is two registers per group,
    // which the reach test's rounds and the batched deferred passes no longer leave — the kernel
    // would spill
    int cq = c;
    asm volatile("" : "+v"(cq));
    const int64_t qi = q0 + M3D_NN_SX * kMQueries + (wave * kMG + g) * 32 + cq;
#else
    const int64_t qi = q[g].qi;
#endif
    const bool pk = publish_k1(sa, M3D_NN_SY, q[g].k1, (chg >> g) & 1u);
    if (pk || q[g].n2 < kInf) near_publish((unsigned long long*)&keys[qi], &near2[qi], q[g].k1, q[g].n2, pk);
  }
  // the tiles this block kept, into its query block's count (the planner of the fused tail reads
  // and zeroes it): one word per block, beside the publish
  if (kPlan && pl.cnt != nullptr && threadIdx.x == 0) atomicAdd(&pl.cnt[M3D_NN_SX], kept);
#if M3D_NN_CLOCK
  // the block's record, written by its last wave out (LDS ticket; a wave's LDS operations execute
  // in order, so every earlier wave's maximum is in): entry, setup done, tile loop done (the
  // writer's own stamps: the latter two follow block barriers), the last wave's exit, the tiles
  // the block kept, the half tiles its slowest wave swept
  {
    const unsigned long long clk3 = __builtin_amdgcn_s_memrealtime();
    const int64_t blk = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;  // launch order in both forms
    if (lane == 0) {
      atomicMax(&clk_exit, clk3);
      if (atomicAdd(&clk_ticket, 1u) == kMBlock / 64 - 1 && blk < kClkBlocks) {
        unsigned long long* rec = g_nn_clock + kClkWords * blk;
        rec[0] = clk0;
        rec[1] = clk1;
        rec[2] = clk2;
        rec[3] = atomicMax(&clk_exit, 0ull);
        rec[4] = kept;
        rec[5] = atomicMax(&clk_slow, 0u);
        rec[6] = (unsigned long long)M3D_NN_SX | ((unsigned long long)M3D_NN_SY << 32) | ((unsigned long long)cur.ty << 48);
        rec[7] = clk2b;  // the deferred passes done (the writer's own: the last wave out)
        if (!kTerms) rec[8] = rec[9] = 0;  // (kTerms: thread 0, behind the hand-off's barrier)
      }
    }
  }
#endif
  // (behind the clock builds' record: its exit stamp is the publish's end)
#if M3D_NN_TU_TERMS_KERNEL
#if M3D_NN_CLOCK
  if constexpr (kTerms)
    nn_terms_handoff(static_cast<const NnTermsDev*>(td), s, (unsigned)sxl, sxy >> 24,
                     blockIdx.x < kClkBlocks ? g_nn_clock + kClkWords * (int64_t)blockIdx.x : nullptr);
#else
  if constexpr (kTerms) nn_terms_handoff(static_cast<const NnTermsDev*>(td), s, (unsigned)sxl, sxy >> 24);
#endif
#endif
}

#undef M3D_NN_SX
#undef M3D_NN_SY
#define M3D_NN_KERNEL_ARGS                                                                            \
  const float4 *__restrict__ src32, int64_t ns, const uint4 *__restrict__ tgt16,                      \
      const float4 *__restrict__ tgt32, const float4 *__restrict__ tbox, int64_t nt_pad, int64_t off, \
      const IcpState *__restrict__ s, int64_t *__restrict__ keys, uint32_t *__restrict__ near2, SeedArgs sa, int64_t q0
#if M3D_NN_TU_MAIN
__global__ __launch_bounds__(kMBlock) __attribute__((amdgpu_waves_per_eu(4))) void nn_mfma_kernel(M3D_NN_KERNEL_ARGS) {
  nn_mfma_body<false>(src32, ns, tgt16, tgt32, tbox, nt_pad, off, s, keys, near2, sa, q0, NnPlan{nullptr, nullptr, 0, 0});
}
#endif
// the planned kernel's launch (grid = the plan's budget) and its resident blocks per CU (0: unknown),
// from whichever translation unit holds the kernel
hipError_t launch_nn_plan_kernel(unsigned blocks, hipStream_t st, M3D_NN_KERNEL_ARGS, NnPlan pl);
int nn_plan_kernel_blocks_per_cu();
#if M3D_NN_TU_PLAN_KERNEL
__global__ __launch_bounds__(kMBlock) __attribute__((amdgpu_waves_per_eu(4))) void nn_mfma_plan_kernel(
    M3D_NN_KERNEL_ARGS, NnPlan pl) {
  nn_mfma_body<true>(src32, ns, tgt16, tgt32, tbox, nt_pad, off, s, keys, near2, sa, q0, pl);
}
hipError_t launch_nn_plan_kernel(unsigned blocks, hipStream_t st, M3D_NN_KERNEL_ARGS, NnPlan pl) {
  nn_mfma_plan_kernel<<<dim3(blocks), kMBlock, 0, st>>>(src32, ns, tgt16, tgt32, tbox, nt_pad, off, s, keys, near2, sa,
                                                        q0, pl);
  return hipGetLastError();
}
int nn_plan_kernel_blocks_per_cu() {
  int per = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, nn_mfma_plan_kernel, kMBlock, 0) != hipSuccess) return 0;
  return per > 0 ? per : 1;
}
#endif
// nn_mfma_terms_kernel's launch and resident blocks per CU, likewise; td: the loop's NnTermsDev
hipError_t launch_nn_terms_kernel(unsigned blocks, hipStream_t st, M3D_NN_KERNEL_ARGS, NnPlan pl, const void* td);
int nn_terms_kernel_blocks_per_cu();
#if M3D_NN_TU_TERMS_KERNEL
__global__ __launch_bounds__(kMBlock) __attribute__((amdgpu_waves_per_eu(4))) void nn_mfma_terms_kernel(
    M3D_NN_KERNEL_ARGS, NnPlan pl, const NnTermsDev* __restrict__ td) {
  nn_mfma_body<true, true>(src32, ns, tgt16, tgt32, tbox, nt_pad, off, s, keys, near2, sa, q0, pl, td);
}
hipError_t launch_nn_terms_kernel(unsigned blocks, hipStream_t st, M3D_NN_KERNEL_ARGS, NnPlan pl, const void* td) {
  nn_mfma_terms_kernel<<<dim3(blocks), kMBlock, 0, st>>>(src32, ns, tgt16, tgt32, tbox, nt_pad, off, s, keys, near2, sa,
                                                         q0, pl, static_cast<const NnTermsDev*>(td));
  return hipGetLastError();
}
int nn_terms_kernel_blocks_per_cu() {
  int per = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, nn_mfma_terms_kernel, kMBlock, 0) != hipSuccess) return 0;
  return per > 0 ? per : 1;
}
#endif
#undef M3D_NN_KERNEL_ARGS
#if M3D_NN_TU_MAIN

// grid.y of nn_mfma_kernel for bx query blocks and ntiles target tiles (block y takes every
// grid.y-th tile); slots = the blocks resident on the device at once, 0 = unknown.
// Every-pair sweep (M3D_NN_CULL=0): pick S in [S0, 2·S0], S0 = 2048 / grid.x, so that the block
// count fills the resident block slots in whole rounds (the last partial round of equal-length
// blocks idles the rest of the chip: 196 × 11 blocks on 512 slots = 4.2 rounds ran as 5).  Culled
// sweep: a block keeps only a few of its tiles, its setup (query load, seed gather, boxes,
// survivor round) weighs as much as what is left of the sweep, and the blocks' lengths differ —
// the most slices whose blocks are all resident at once, S = ⌊slots / grid.x⌋, at least 1.  A
// second, partial round of blocks starts when the first blocks end and ends the launch a whole
// block later (tools/nn_clock.py: 588 blocks on 512 slots, the last 76 started at 16–22 µs of 54);
// with the per-query reach test the tile lists are short and even enough that fewer, longer blocks
// in one round win (EXPERIMENTS §R10: cfg1 51 µs at S = 2 against 54 at 3, 60 at 4–5, 65 at 1; the
// 1M pair fastest at S = 1, which both ⌊⌋ and the earlier ⌈⌉ give).  The rule rests on those two
// shapes only.  With few query blocks it degenerates to one tile per block (grid.x = 1 gives
// S = ntiles, the clamp): every block then pays the setup for at most one tile.
// Unknown slots: S0 blocks per query block, evened out to equal tile counts.
// Since the slice plan (nn_plan.h, launch_icp_nn below) this is the DEFAULT assignment: the 2-D
// launch's grid.y, and in the planned 1-D launch what every block derives from its index while the
// loop state has no valid plan (the first evaluation after a reset, one-shot paths); with a plan,
// query block x gets S_x blocks from the table instead, Σ S_x ≤ slots.
static int64_t nn_grid_y(int64_t bx, int64_t ntiles, int64_t slots, bool cull) {
  const auto clamped = [&](int64_t S) { return std::min(std::max<int64_t>(S, 1), ntiles); };
  const int64_t s0 = clamped((2048 + bx - 1) / bx);
  if (slots <= 0 || ntiles <= 1) {
    const int64_t per = (ntiles + s0 - 1) / s0;  // tiles per block
    return (ntiles + per - 1) / per;
  }
  if (cull) return clamped(slots / bx);
  int64_t best = s0;
  double best_eff = 0.0;
  for (int64_t S = s0; S <= std::min(2 * s0, ntiles); ++S) {
    const int64_t blocks = bx * S, rounds = (blocks + slots - 1) / slots;
    const double eff = (double)blocks / (double)(rounds * slots);
    if (eff > best_eff + 1e-9) {
      best_eff = eff;
      best = S;
    }
  }
  return best;
}

#if M3D_NN_CLOCK
}  // namespace m3d
extern "C" int m3d_debug_nn_clock(unsigned long long* out, int n) {
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(m3d::g_nn_clock), sizeof(unsigned long long) * (size_t)n) == hipSuccess ? 0 : -1;
}
namespace m3d {
#endif
static bool icp_nn_uses_mfma(const m3d_icp* s) {
  return s->tgrid != nullptr && s->tgrid->mf16 != nullptr;
}

// whether the loop's NN can run on a slot range [q0, q1) of the visit order: the grid form needs
// the source's Morton query grid; the brute form always can (m3d_icp_create builds its tiles)
bool icp_nn_range_ok(const m3d_icp* s) {
  if (s->params.nn_method == M3D_NN_GRID) return s->sgrid != nullptr && s->sgrid->mpts != nullptr;
  return icp_nn_uses_mfma(s);
}

// Brute-force NN into s->keys (after launch_icp_keyinit, or self_seed: keys all kKeyNone, see
// SeedArgs): nn_mfma_kernel alone (its exact in-kernel scan covers transforms whose operands do
// not fit fp16).  m3d_icp_create builds the target's MFMA tiles for every brute-force loop.
// The launch's shape for queries [q0, ns): query blocks, the uniform slices, and whether it is the
// planned (1-D) one — whenever the loop's plan can apply: the whole source, M3D_NN_PLAN on, and
// (nn_plan_shape, at create) resident slots known and more of them than query blocks.
struct NnLaunchShape {
  int64_t bx, gy;
  bool planned;
};
static NnLaunchShape nn_launch_shape(const m3d_icp* s, int64_t q0, int64_t ns) {
  const int64_t tt = (int64_t)kTH * kMTile;
  const int64_t bx = (ns - q0 + kMQueries - 1) / kMQueries;
  const int64_t gy = nn_grid_y(bx, s->tgrid->mf_npad / tt, nn_resident_slots(), M3D_NN_CULL != 0);
  const bool planned = nn_plan_on() && s->nn_qblocks > 0 && q0 == 0 && ns == s->src->n && bx == s->nn_qblocks &&
                       bx * gy <= s->nn_budget;
  return NnLaunchShape{bx, gy, planned};
}

// whether the whole-source launch of this loop is the planned one (and launches at all)
bool icp_nn_planned(const m3d_icp* s) {
  if (s->src->n <= 0 || s->tgt->n == 0 || !icp_nn_uses_mfma(s) || s->tgrid->mf_npad % ((int64_t)kTH * kMTile) != 0)
    return false;
  return nn_launch_shape(s, 0, s->src->n).planned;
}

// with_terms: nn_mfma_terms_kernel, whose blocks also run the terms pass (the caller has checked
// nn_terms_selected: the launch is the planned one)
hipError_t launch_icp_nn(const m3d_icp* s, int64_t off, bool self_seed, hipStream_t st, int64_t q0,
                         int64_t q1, bool with_terms) {
  const int64_t ns = q1 < 0 ? s->src->n : q1;  // queries: visit positions [q0, ns)
  if (ns <= q0 || s->tgt->n == 0) return with_terms ? hipErrorInvalidValue : hipSuccess;
  const Grid* tg = s->tgrid;
  const int64_t tt = (int64_t)kTH * kMTile;
  if (!icp_nn_uses_mfma(s) || tg->mf_npad % tt != 0) return hipErrorInvalidValue;  // pack16 pads to kMTilePad
  const NnLaunchShape sh = nn_launch_shape(s, q0, ns);
  const int64_t bx = sh.bx, gy = sh.gy;
  // (the records exist where the fused tail wrote them: icp.hip terms_args, the same condition)
  const bool by_rec = M3D_NN_SEED_REC != 0 && self_seed && off == 0 && s->tgt->rec64 != nullptr && s->seed != nullptr;
  const SeedArgs sa{s->corr, by_rec ? s->seed : s->tgt->xyz32, s->tgt->n, by_rec ? 2 : self_seed ? 1 : 0};
  const bool planned = sh.planned;
  if (with_terms) {
    if (!planned || s->nn_targs == nullptr) return hipErrorInvalidValue;
    return launch_nn_terms_kernel((unsigned)s->nn_budget, st, s->src->xyz32, ns, tg->mf16, tg->mf32, tg->mfbox,
                                  tg->mf_npad, off, s->state, s->keys, s->near2, sa, q0,
                                  NnPlan{s->nn_table, s->nn_cnt, (int)bx, (int)gy}, s->nn_targs);
  }
  if (planned)
    return launch_nn_plan_kernel((unsigned)s->nn_budget, st, s->src->xyz32, ns, tg->mf16, tg->mf32, tg->mfbox,
                                 tg->mf_npad, off, s->state, s->keys, s->near2, sa, q0,
                                 NnPlan{s->nn_table, s->nn_cnt, (int)bx, (int)gy});
  nn_mfma_kernel<<<dim3((unsigned)bx, (unsigned)gy), kMBlock, 0, st>>>(
        s->src->xyz32, ns, tg->mf16, tg->mf32, tg->mfbox, tg->mf_npad, off, s->state, s->keys, s->near2, sa, q0);
  return hipGetLastError();
}

int64_t nn_resident_slots() {
  static const int64_t slots = [] {
    int dev = 0, per = 0;
    hipDeviceProp_t p;
    if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&p, dev) != hipSuccess) return (int64_t)0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, nn_mfma_kernel, kMBlock, 0) != hipSuccess)
      return (int64_t)0;
    // all three kernels hold two blocks per CU (128 VGPRs, 67 KB of LDS); the smaller count if they ever differ
    const int pp = nn_plan_kernel_blocks_per_cu(), pt = nn_terms_kernel_blocks_per_cu();
    per = per > 0 ? per : 1;
    if (pp > 0 && pp < per) per = pp;
    if (pt > 0 && pt < per) per = pt;
    return (int64_t)p.multiProcessorCount * per;
  }();
  return slots;
}

// M3D_NN_PLAN=0 in the environment: every launch as the uniform 2-D one
bool nn_plan_on() {
  static const bool on = [] {
    const char* e = getenv("M3D_NN_PLAN");
    return !(e && atoi(e) == 0);
  }();
  return on;
}

// The plan shape of a brute-force loop over ns sources: its query blocks and the block budget (the
// resident slots); 0 / 0 where no plan applies — slots unknown, at least as many query blocks as
// slots (the 1M source: 1954 query blocks, uniform S = 1 stays), or more than the planner holds.
void nn_plan_shape(int64_t ns, int32_t* qblocks, int32_t* budget) {
  const int64_t slots = nn_resident_slots(), bx = (ns + kMQueries - 1) / kMQueries;
  const bool ok = M3D_NN_CULL != 0 && slots > 0 && bx >= 1 && bx < slots && bx <= kPlanMaxQ && slots <= 0xFFFF;
  *qblocks = ok ? (int32_t)bx : 0;
  *budget = ok ? (int32_t)slots : 0;
}

PlanArgs nn_plan_args(const m3d_icp* s) {
  PlanArgs pa;
  if (!nn_plan_on() || s->nn_qblocks <= 0 || s->tgrid == nullptr) return pa;
  pa.cnt = s->nn_cnt;
  pa.seen = s->nn_seen;
  pa.table = s->nn_table;
  pa.n = s->nn_qblocks;
  pa.budget = s->nn_budget;
  pa.cap = (int32_t)plan_cap(kPlanSmax, s->tgrid->mf_npad / ((int64_t)kTH * kMTile));
  return pa;
}

#endif  // M3D_NN_TU_MAIN

}  // namespace m3d
#endif  // this translation unit holds something
