/*
 * m3d.h — C ABI of the MI355X-native point-cloud registration core (libm3d.so, gfx950).
 *
 * Drop-in boundary for the hot path of KTC-Security-Circle/3d-matching `src/matcher`
 * (SURVEY.md §8(b)).  The reference has no FFI of its own: its "plugin API" is the Python
 * functions of `src/matcher/ransac.py` and `src/matcher/icp.py`, which call numpy and the
 * Open3D 0.19 C++ registration pipeline.  Each entry point below names the reference interface
 * it replaces; the Python mirror (3d-matching_amd/matcher) binds them through ctypes.
 *
 * Conventions
 *   - Plain C types only; no torch types.  Array arguments marked [device] are caller-owned
 *     device allocations (e.g. torch.cuda tensors' data_ptr()); [host] are host memory.
 *   - Point arrays are float64 AoS N×3 (24 B/pt), exactly the layout of Open3D's
 *     Vector3dVector / numpy (N,3) the reference uses; correspondences are int32 N×2.
 *   - 4×4 transforms are float64 row-major (numpy order).
 *   - `stream` is a hipStream_t (NULL = legacy default stream).  Every entry point only
 *     enqueues work on `stream` unless documented as synchronous (the *_run functions and the
 *     object constructors return host values and synchronise the stream).
 *   - Return value: M3D_OK (0) or a negative M3D_ERR_*; m3d_last_error(ctx) explains it.
 *     Numerical failure of a hypothesis is NOT an error: as in the reference
 *     (ransac.py:134-140,184-192) it yields the identity transform and a per-hypothesis status.
 *   - One context per (host thread, device).  A context owns its scratch memory; the library
 *     never frees caller memory.  Calls on one context that use its scratch (the RANSAC entry
 *     points) may pass different streams: a call on another stream than the previous one first
 *     waits on the device for the previous call's work (no host synchronisation), so such calls
 *     are ordered, not concurrent.
 */
#ifndef M3D_H_
#define M3D_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define M3D_ABI_VERSION 13

/* return codes */
#define M3D_OK 0
#define M3D_ERR_INVALID (-1)  /* bad argument (sizes, null pointers, missing normals, ...) */
#define M3D_ERR_HIP (-2)      /* HIP runtime error */
#define M3D_ERR_OOM (-3)      /* device allocation failed */
#define M3D_ERR_NODEVICE (-4) /* no usable gfx950 device */
#define M3D_ERR_COMM (-5)     /* a peer rank failed, or the communicator was aborted (ABI 8) */

/* per-hypothesis status (ransac.py:134-140,184-192) */
#define M3D_HYP_OK 0
#define M3D_HYP_DEGENERATE 1 /* fewer than 3 correspondences -> identity */
#define M3D_HYP_NONFINITE 2  /* NaN/Inf in the estimate -> identity */

/* inlier comparator */
#define M3D_SCORE_SQUARED 0 /* Σd² < thr   (evaluate_inlier_ratio_fast, ransac.py:274-277) */
#define M3D_SCORE_NORM 1    /* ‖d‖ < thr    (evaluate_inlier_ratio,      ransac.py:233-236) */

/* ICP estimators (Open3D TransformationEstimation*) */
#define M3D_EST_POINT_TO_POINT 0
#define M3D_EST_POINT_TO_PLANE 1

typedef struct m3d_ctx m3d_ctx;
typedef struct m3d_corrset m3d_corrset; /* packed correspondence set (RANSAC) */
typedef struct m3d_cloud m3d_cloud;     /* packed point cloud (ICP / NN)      */
typedef struct m3d_icp m3d_icp;         /* device-resident ICP loop state     */
typedef struct m3d_mesh m3d_mesh;       /* triangle mesh (point-to-mesh distance) */

/* ------------------------------------------------------------------ context */
int m3d_abi_version(void);
int m3d_device_count(int* count);
int m3d_create(int device, m3d_ctx** out);
void m3d_destroy(m3d_ctx* ctx);
const char* m3d_last_error(const m3d_ctx* ctx);
/* Device-side hit counters (cumulative): [0] pairs rechecked in fp64 by the scoring screens
 * (guard band), [1] by full hypothesis; the others are reserved (0). */
int m3d_get_stats(m3d_ctx* ctx, int64_t* out8 /* [host] 8 values */);

/* Kernel timing with HIP events recorded on the launch stream immediately before and after each
 * launch of the named kernel (benchmarks / roofline).  Kernel ids: */
#define M3D_KERNEL_NN 0     /* ICP brute-force NN scan          */
#define M3D_KERNEL_SCORE 1  /* RANSAC fp32 scoring screen       */
#define M3D_KERNEL_KABSCH 2 /* RANSAC batched 3-point Kabsch    */
#define M3D_KERNEL_TERMS 3  /* ICP fp64 estimation terms        */
#define M3D_KERNEL_LOOP 4   /* the solve launch of the side-terms loops (robust, Generalized, Colored, mesh ICP);
                               also used by other calls' own stages (ABI 10-11: the persistent grid loop) */
#define M3D_KERNEL_COMM 5   /* RCCL all-reduces issued by the library, on their streams (ABI 10) */
int m3d_profile_enable(m3d_ctx* ctx, int enable);
/* Synchronises, returns Σ launch durations (ms) and launch count since the last read, resets. */
int m3d_profile_read(m3d_ctx* ctx, int kernel, double* total_ms, int64_t* launches);

/* ------------------------------------------------------------------ RANSAC */

/* Gather + pack a correspondence set: p_i = src[corr[i,0]], q_i = tgt[corr[i,1]].
 * Replaces the per-call gathers of evaluate_inlier_ratio (ransac.py:223-227) and the
 * pre-gather of _visualize_matcher.py:376-384.  Synchronous (computes centring offsets).
 * src_xyz [device] ns×3 f64, tgt_xyz [device] nt×3 f64, corr [device] nc×2 int32. */
int m3d_corrset_create(m3d_ctx* ctx, const double* src_xyz, int64_t ns, const double* tgt_xyz,
                       int64_t nt, const int32_t* corr, int64_t nc, void* stream,
                       m3d_corrset** out);
/* Same from pre-gathered pairs (the p_src / p_tgt arguments of evaluate_inlier_ratio_fast,
 * ransac.py:239-244): p_src, p_tgt [device] nc×3 f64. */
int m3d_corrset_create_gathered(m3d_ctx* ctx, const double* p_src, const double* p_tgt,
                                int64_t nc, void* stream, m3d_corrset** out);
void m3d_corrset_destroy(m3d_corrset* cs);
int64_t m3d_corrset_size(const m3d_corrset* cs);

/* a1, batched: H hypotheses of compute_step_transformation (ransac.py:104-192).
 * triples [device] H×3 int32 correspondence rows (replay mode: e.g. the rows the reference's
 * np.random.choice(n,3,replace=False) draws, see m3d_replay_triples), or NULL for the native
 * counter-based sampler keyed by (seed, hyp0 + h).
 * T_out [device] H×16 f64 row-major; status [device] H uint8 (may be NULL). */
int m3d_kabsch3_batch(m3d_ctx* ctx, const m3d_corrset* cs, const int32_t* triples,
                      uint64_t seed, int64_t hyp0, int64_t H, double* T_out, uint8_t* status,
                      void* stream);

/* a2/a3, batched: counts[h] = #{i : dist(T_h p_i, q_i) < thr} for H transforms.
 * mode M3D_SCORE_SQUARED: thr is the squared threshold (evaluate_inlier_ratio_fast);
 * mode M3D_SCORE_NORM:    thr is the distance threshold (evaluate_inlier_ratio).
 * T [device] H×16 f64; counts [device] H int32.  Counts are exact w.r.t. an fp64 evaluation
 * of the reference formula (fp32 screen + fp64 recheck of pairs inside a proven guard band). */
int m3d_ransac_score(m3d_ctx* ctx, const m3d_corrset* cs, const double* T, int64_t H, double thr,
                     int mode, int32_t* counts, void* stream);

/* a1 and a2/a3 for ONE hypothesis with host operands — the per-call form the reference harness
 * uses (benchmark_ransac.py:105-113: one compute_step_transformation + one
 * evaluate_inlier_ratio per iteration).  Synchronous; the operands travel as kernel arguments
 * and the results come back through the context's mapped pinned memory (one launch + one
 * stream sync each; a2/a3 evaluates the reference formula directly in fp64, numpy's order).
 * m3d_kabsch3_one: triple [host] 3 int32 rows; T_out [host] 16 f64; status [host] (may be
 * NULL) M3D_HYP_*.  Replaces compute_step_transformation (ransac.py:104-192) after its
 * np.random.choice draw (ransac.py:143).
 * m3d_ransac_score_one: T [host] 16 f64; *count [host] = inliers (thr / mode as in
 * m3d_ransac_score).  Replaces evaluate_inlier_ratio[_fast] (ransac.py:195-277). */
int m3d_kabsch3_one(m3d_ctx* ctx, const m3d_corrset* cs, const int32_t* triple, double* T_out,
                    int32_t* status, void* stream);
int m3d_ransac_score_one(m3d_ctx* ctx, const m3d_corrset* cs, const double* T, double thr,
                         int mode, int64_t* count, void* stream);

/* a4: the step-RANSAC loop (_visualize_matcher.py:343-470; benchmark_ransac.py:87-125 when
 * early_stop == 0), run on the device in batches with no host round trip per batch. */
typedef struct {
  int64_t max_iter;     /* MatcherSettings.ransac_iteration                          */
  uint64_t seed;        /* native sampler seed (ignored when triples are supplied)   */
  double thr;           /* comparator threshold (see mode)                           */
  int32_t mode;         /* M3D_SCORE_SQUARED (GUI loop, a3) or M3D_SCORE_NORM (a2)   */
  int32_t early_stop;   /* MatcherSettings.early_stop_enabled                        */
  double es_threshold;  /* MatcherSettings.early_stop_threshold (0.5)                */
  double es_confidence; /* MatcherSettings.early_stop_confidence (0.99)              */
  int64_t batch;        /* hypotheses per device batch (0 = automatic)               */
  int64_t hyp0;         /* first hypothesis id (multi-GPU hypothesis sharding)       */
} m3d_ransac_params;

typedef struct {
  double T[16];        /* best transform (row-major)                        */
  double fitness;      /* best inlier ratio = best_count / nc                */
  int64_t best_index;  /* 0-based iteration index of the best hypothesis     */
  int64_t iterations;  /* iter_num at exit (early stop or max_iter)          */
  int64_t best_count;  /* inlier count of the best hypothesis                */
  int64_t rechecked;   /* pairs re-evaluated in fp64 (guard band)            */
} m3d_ransac_result;

/* triples [device] max_iter×3 int32 or NULL (native sampler).  Synchronous. */
int m3d_ransac_run(m3d_ctx* ctx, const m3d_corrset* cs, const m3d_ransac_params* params,
                   const int32_t* triples, m3d_ransac_result* out, void* stream);
/* Asynchronous form: per-hypothesis counts of the whole run land in counts_out [device]
 * (max_iter int32, may be NULL; hypotheses after an early stop are not scored and read 0) and
 * the result struct in result_dev [device]. */
int m3d_ransac_run_async(m3d_ctx* ctx, const m3d_corrset* cs, const m3d_ransac_params* params,
                         const int32_t* triples, int32_t* counts_out, m3d_ransac_result* result_dev,
                         void* stream);

/* Host-side replay of the reference RNG: the rows H successive
 * `np.random.choice(nc, 3, replace=False)` calls of the legacy MT19937 RandomState draw
 * (ransac.py:143 ≡ permutation(nc)[:3]).  mt_key [host] 624 uint32 + *mt_pos is the state
 * `np.random.get_state()` returns; both are advanced in place exactly as numpy would.
 * triples_out [host] H×3 int32. */
int m3d_replay_triples(uint32_t* mt_key, int32_t* mt_pos, int64_t nc, int64_t H,
                       int32_t* triples_out);

/* ------------------------------------------------------------------ ICP */

/* Pack a cloud for NN / ICP: xyz [device] n×3 f64, normals [device] n×3 f64 or NULL.
 * Synchronous (computes the centring offset).  Replaces Open3D's PointCloud copy +
 * KDTreeFlann::SetGeometry (Registration.cpp RegistrationICP). */
int m3d_cloud_create(m3d_ctx* ctx, const double* xyz, const double* normals, int64_t n,
                     void* stream, m3d_cloud** out);
/* The same with an explicit centring offset center [host] 3 f64 instead of the cloud's mean.
 * Shards of one target cloud created with the same centre share one fp32 frame, so their NN
 * keys are comparable bit for bit: target-sharded ICP (m3d_icp_shard_nn on each rank, MIN of
 * the keys) then seeds the queries whose previous winner another rank owns with a distance
 * bound instead of the radius (nnkey.h seed_key) — same result, far fewer screen hits. */
int m3d_cloud_create_framed(m3d_ctx* ctx, const double* xyz, const double* normals, int64_t n,
                            const double* center, void* stream, m3d_cloud** out);
/* The same from HOST arrays (ABI 11): xyz [host] n×3 f64, normals [host] n×3 f64 or NULL, center
 * [host] 3 f64 or NULL (the cloud's mean).  The arrays go straight into the cloud's buffers
 * (one pageable copy each) instead of a caller's upload plus a device-to-device copy.  The same
 * cloud, bit for bit.  Synchronous. */
int m3d_cloud_create_host(m3d_ctx* ctx, const double* xyz, const double* normals, int64_t n,
                          const double* center, void* stream, m3d_cloud** out);
/* Destroy a cloud.  Its device blocks go to the library's block cache, marked after all work
 * its context had enqueued on any stream; a later allocation reuses them in stream order (the
 * allocating stream waits on the device; no host or device-wide synchronisation, ABI 12).
 * An m3d_icp created on this cloud may outlive it: the loop keeps the data it runs on and frees
 * it in m3d_icp_destroy (ABI 12); stepping a loop whose TARGET cloud is gone is undefined.
 * Destroy every object before its context. */
void m3d_cloud_destroy(m3d_cloud* c);
int64_t m3d_cloud_size(const m3d_cloud* c);
/* Give the block cache's idle blocks of ctx's device back to the driver (each after its release
 * point has passed on the device); freed_bytes may be NULL.  The Python layer calls this when a
 * device allocation fails; the library does so itself before retrying its own allocations, and
 * when the last context of a device is destroyed.  M3D_BLOCK_CACHE=<MiB> caps the cache (default
 * 2048, 0 = no cache).  ABI 12. */
int m3d_trim_block_cache(m3d_ctx* ctx, int64_t* freed_bytes);

/* Nearest-neighbour search method.  Both return the identical (d², index) result: BRUTE scans
 * every target (cfg1's LDS-tiled brute force), GRID visits only the uniform-grid cells that can
 * hold a target within the radius. */
#define M3D_NN_BRUTE 0
#define M3D_NN_GRID 1

/* Radius-bounded 1-NN (KDTreeFlann::SearchHybrid(p, r, 1) for every source point after T):
 * idx [device] ns int32 (-1 = no target with d² < r²), d2 [device] ns f64 (may be NULL). */
int m3d_nn1(m3d_ctx* ctx, const m3d_cloud* src, const m3d_cloud* tgt, const double* T_host,
            double max_dist, int32_t nn_method, int32_t* idx, double* d2, void* stream);

/* Evaluation of a given transform (Open3D EvaluateRegistration and
 * GetInformationMatrixFromPointClouds; added within ABI 13, the version number is unchanged).
 * The source is transformed by T_host [host] 16 f64 (NULL = identity) only when T_host is not
 * Eigen-isIdentity(), as in m3d_icp_reset(); each source point's correspondence is the winner
 * m3d_nn1() defines (the lexicographic (d², index) minimum over the targets with d² < max_dist²).
 *   fitness = matched / ns, inlier_rmse = sqrt(Σd² / matched), both 0 without a match;
 *   information (flags & M3D_EVAL_INFORMATION) = GᵀG over the matched TARGET points q = (x, y, z)
 *   in the target's original fp64 coordinates, rows G₁ = (0, z, −y, 1, 0, 0),
 *   G₂ = (−z, 0, x, 0, 1, 0), G₃ = (y, −x, 0, 0, 0, 1).
 * corr_idx [device] ns int32 or NULL: the matched target per source in the caller's order (-1 =
 * none); d2 [device] ns f64 or NULL: its d² (INFINITY = none).  All sums are fp64 and added in a
 * fixed order: both nn_methods, and repeated calls, return the same bits.  Synchronous (one host
 * sync).  M3D_ERR_INVALID for max_dist <= 0 or an unknown nn_method; M3D_ERR_HIP when the grid
 * NN's deferral list overflowed (as m3d_icp_result_get() reports it). */
#define M3D_EVAL_INFORMATION 1 /* flags: also fill information[] */
typedef struct {
  double fitness;              /* matched / ns  (0 when ns == 0) */
  double inlier_rmse;          /* sqrt(sum d2 / matched)  (0 when matched == 0) */
  int64_t num_correspondences;
  double information[36];      /* row-major GtG; zeros unless M3D_EVAL_INFORMATION */
} m3d_eval_result;
int m3d_evaluate_registration(m3d_ctx* ctx, const m3d_cloud* src, const m3d_cloud* tgt,
                              const double* T_host, double max_dist, int32_t nn_method, int32_t flags,
                              m3d_eval_result* out, int32_t* corr_idx, double* d2, void* stream);

typedef struct {
  double relative_fitness; /* ICPConvergenceCriteria defaults 1e-6 */
  double relative_rmse;    /* 1e-6 */
  int32_t max_iteration;   /* 30 */
  int32_t estimation;      /* M3D_EST_* */
  int32_t nn_method;       /* M3D_NN_* */
  int32_t flags;           /* M3D_ICP_* (ABI 10; 0 = defaults) */
} m3d_icp_params;
/* m3d_icp_params.flags 1 and 4 (ABI 10-11: the persistent grid loop on / off) are accepted and
 * ignored since ABI 12, which removed that loop (measured slower than the two-launch steps). */
#define M3D_ICP_NO_PERSIST 1
#define M3D_ICP_PERSIST 4
/* m3d_icp_params.flags: the target-shard loop exchanges all keys in one MIN instead of two halves
 * overlapped with the second half's NN (m3d_icp_shard_steps) */
#define M3D_ICP_NO_SPLIT 2

typedef struct {
  double T[16];
  double fitness;
  double inlier_rmse;
  int64_t num_correspondences;
  int32_t iterations; /* updates applied */
  int32_t converged;
  double update[16];  /* the last update ΔT (identity after a reset), ABI 12 */
} m3d_icp_result;

/* registration_icp (icp.py:42-48 → Open3D RegistrationICP).  init [host] 16 f64.
 * corr_idx [device] ns int32 or NULL: final correspondence target per source (-1 = none).
 * Synchronous. */
int m3d_icp_run(m3d_ctx* ctx, const m3d_cloud* src, const m3d_cloud* tgt, const double* init,
                double max_dist, const m3d_icp_params* params, m3d_icp_result* out,
                int32_t* corr_idx, void* stream);

/* Step-wise ICP driver (benchmarks, multi-GPU).  An m3d_icp holds the device-resident loop
 * state (T, fitness/rmse history, convergence flag); every call only enqueues work. */
int m3d_icp_create(m3d_ctx* ctx, const m3d_cloud* src, const m3d_cloud* tgt, double max_dist,
                   const m3d_icp_params* params, m3d_icp** out);
void m3d_icp_destroy(m3d_icp* s);
/* init [host] 16 f64 or NULL (identity).  As RegistrationICP (Registration.cpp): T starts at
 * init, and the loop's copy of the source is transformed by init only when init is not
 * Eigen-isIdentity() (|a − δ| ≤ 1e-12); every update ΔT then transforms that copy again
 * (pcd.Transform(update)), and each evaluation's fp64 queries are those points (ABI 12: before,
 * the queries were T·p of the original source). */
int m3d_icp_reset(m3d_icp* s, const double* init_host, void* stream);
/* The loop's fp64 points of the last evaluation (the source after init and every update but the
 * one the evaluation produced), dst [device] ns×3 f64 in the caller's source order.  After a reset
 * and before the first evaluation: the source with the init applied exactly as RegistrationICP's
 * pcd.Transform(init) (the source itself when init isIdentity()).  An evaluation counts from its
 * terms pass on: between m3d_icp_shard_terms and m3d_icp_solve (the shard protocol) the points are
 * already that evaluation's.  ABI 12; init applied ABI 13. */
int m3d_icp_copy_points(const m3d_icp* s, double* dst, void* stream);
/* One full iteration on one device: NN evaluation + estimation terms + solve/update. */
int m3d_icp_step(m3d_icp* s, void* stream);
/* n iterations (n × m3d_icp_step, enqueued from native code: no per-iteration host binding
 * overhead).  Iterations after convergence / max_iteration are device no-ops.  A sequence of n
 * steps requested a second time (from the same keys state) is captured into a HIP graph and
 * replayed as one launch from then on (M3D_ICP_GRAPH=0: plain enqueues); the results are the
 * same bits either way. */
int m3d_icp_steps(m3d_icp* s, int32_t n, void* stream);
/* Capture the n-step graph now, for the loop's current state (setup work, e.g. before a timed
 * region; nothing runs).  Later m3d_icp_steps(s, n) calls from that state replay it. */
int m3d_icp_prepare_steps(m3d_icp* s, int32_t n);
/* Multi-GPU pieces (icp.py:42-48 with the correspondence search split over ranks).
 * Result contract of every NN (nnkey.h): for each source point the lexicographic (d64, index)
 * minimum over the targets with d64 < r², d64 the fp64 d² of the fp64 transformed point —
 * identical on one device and over any number of target shards.
 *
 * Target shard (cfg3): `tgt` of m3d_icp_create is this rank's shard whose first point has global
 * index shard_offset (create every shard with the same centre, m3d_cloud_create_framed).  Per
 * iteration, with the exchanges done by the caller (or m3d_comm_*):
 *   m3d_icp_shard_nn(s, off, dkeys)      this shard's fp64 winners; dkeys [device] ns int64 =
 *                                        bits(d64) (INT64_MAX none)          → all-reduce MIN
 *   m3d_icp_shard_claim(s, dmin, claim)  claim [device] ns int32 = own target index where the own
 *                                        winner has the global d64, else INT32_MAX → all-reduce MIN
 *                                        (exact fp64 ties across shards → lowest index)
 *   m3d_icp_shard_terms(s, off, dmin, claim, sums)  terms of the owned winners; sums [device]
 *                                        32 f64                               → all-reduce SUM
 *   m3d_icp_solve(s, sums)               identical update on every rank.
 * Every per-source exchange buffer (dkeys, dmin, claim) is indexed by the loop's SOURCE SLOT: the
 * loop keeps its source in the Morton order of the source's grid (coalesced per-source arrays);
 * m3d_icp_copy_slots gives slot → source index.  Ranks that share one source cloud (the target
 * shard) get the same slots.
 * Source shard (SURVEY §8(e) "ICP alternative"): `src` is this rank's source shard, `tgt` the
 * whole target: m3d_icp_shard_nn(s, 0, NULL) + m3d_icp_shard_terms(s, 0, NULL, NULL, sums),
 * SUM of the sums, m3d_icp_solve; the fitness denominator is m3d_icp_set_source_total's. */
int m3d_icp_shard_nn(m3d_icp* s, int64_t shard_offset, int64_t* dkeys, void* stream);
/* m3d_icp_shard_nn for the source slots [q0, q1) only (dkeys entries outside stay untouched): the
 * pieces of the split exchange (ABI 8).  M3D_ERR_INVALID when the loop's NN has no range form. */
int m3d_icp_shard_nn_range(m3d_icp* s, int64_t shard_offset, int64_t q0, int64_t q1, int64_t* dkeys,
                           void* stream);
int m3d_icp_shard_claim(m3d_icp* s, const int64_t* dmin, int32_t* claim, void* stream);
int m3d_icp_shard_terms(m3d_icp* s, int64_t shard_offset, const int64_t* dmin, const int32_t* claim,
                        double* sums, void* stream);
int m3d_icp_solve(m3d_icp* s, const double* sums, void* stream);
/* Source-sharded runs: the source count over all ranks (0 = this shard's own count). */
int m3d_icp_set_source_total(m3d_icp* s, int64_t ns_total);
/* ------------------------------------------------------------------ RCCL inside the library
 * (SURVEY §8(b)/(e)): one communicator per (context, rank) over RCCL/xGMI; the caller only
 * carries the 128-byte unique id from rank 0 to the others (e.g. torch.distributed's
 * broadcast_object_list) — the collectives of the multi-GPU loops are issued by libm3d on the
 * caller's stream, with no host round trip. */
typedef struct m3d_comm m3d_comm;
#define M3D_COMM_ID_BYTES 128
#define M3D_DT_I32 0
#define M3D_DT_I64 1
#define M3D_DT_F64 2
#define M3D_OP_SUM 0
#define M3D_OP_MIN 1
#define M3D_OP_MAX 2
/* id_out [host] M3D_COMM_ID_BYTES bytes (ncclGetUniqueId), called on rank 0. */
int m3d_comm_unique_id(uint8_t* id_out);
/* Collective over the world's ranks (every rank calls it with the same id).  Synchronous.  Every
 * buffer the library's collectives use is allocated here or before a loop's first collective.
 * Failure contract (ABI 8): a loop object's first multi-GPU call allocates its exchange buffers
 * and all ranks agree on the outcome (a rank whose setup failed returns its error, its peers
 * M3D_ERR_COMM — nobody enters the loop); m3d_ransac_run_sharded is fail-soft (a failed local run
 * still joins the collectives, every rank returns an error); a launch or RCCL error inside a
 * collective loop aborts the communicator (ncclCommAbort) and every later call on it returns
 * M3D_ERR_COMM — peers already waiting in a collective cannot be reached from that rank, so the
 * caller must then tear down every rank (torch.distributed.run does when a worker fails). */
int m3d_comm_init(m3d_ctx* ctx, const uint8_t* id, int rank, int world, m3d_comm** out);
void m3d_comm_destroy(m3d_comm* c);
/* In-place all-reduce of buf [device] count elements of dtype M3D_DT_* with op M3D_OP_*. */
int m3d_comm_allreduce(m3d_comm* c, void* buf, int64_t count, int dtype, int op, void* stream);
/* n iterations of target-sharded ICP (the protocol of "Multi-GPU pieces" above) with the MIN /
 * MIN / SUM all-reduces issued inside; every rank calls it with its shard offset.  The sources
 * are split into two slot halves: the first half's d64 MIN runs on a library-owned exchange
 * stream while the second half's NN runs on `stream` (M3D_SHARD_SPLIT=0: one piece). */
int m3d_icp_shard_steps(m3d_icp* s, m3d_comm* c, int64_t shard_offset, int32_t n, void* stream);
/* n iterations of source-sharded ICP (one SUM of the 32 term slots per iteration). */
int m3d_icp_source_shard_steps(m3d_icp* s, m3d_comm* c, int32_t n, void* stream);
/* Hypothesis-sharded a4 without early stop (cfg2 at N > 1): after m3d_ransac_run_async on each
 * rank's id range [hyp0, hyp0 + max_iter), key_dev [device] 1 int64 ← MAX over ranks of
 * (best_count << 32) | (2³² − 1 − (hyp0 + best_index)): highest count, lowest global id. */
int m3d_ransac_best_allreduce(m3d_comm* c, const m3d_ransac_result* result_dev, int64_t hyp0,
                              int64_t* key_dev, void* stream);
/* The whole hypothesis-sharded run, synchronous (one host sync): out holds the global winner
 * (its transform's bits from the winning rank via an integer SUM; best_index = global id;
 * iterations and rechecked summed over ranks).  params->early_stop must be 0 and the native
 * sampler is used.  Scratch is the communicator's (no allocation per call). */
int m3d_ransac_run_sharded(m3d_ctx* ctx, m3d_comm* c, const m3d_corrset* cs,
                           const m3d_ransac_params* params, m3d_ransac_result* out, void* stream);
/* 1 once the communicator was aborted after a failure (M3D_ERR_COMM from then on), else 0. */
int m3d_comm_poisoned(const m3d_comm* c);

/* Read the loop state (synchronises the stream).  M3D_ERR_HIP when the grid NN's deferral list
 * overflowed since the last reset (its writes were dropped, the keys are not valid; ABI 13). */
int m3d_icp_result_get(m3d_icp* s, m3d_icp_result* out, void* stream);
/* The correspondence set of a per-source index array (RegistrationResult.correspondence_set,
 * icp.py:42 / ransac.py:42-59; ABI 11): pairs_out [host] with room for 2·n int32 receives
 * (i, corr_idx[i]) for every i with corr_idx[i] >= 0, in increasing i; *count [host] = the number
 * of pairs.  corr_idx [device] n int32 (m3d_icp_run's corr_idx, m3d_icp_copy_corr's dst, the
 * feature RANSAC's corr_set_out).  Compacted on the device; only the pairs cross to the host.
 * Synchronous. */
int m3d_corr_pairs(m3d_ctx* ctx, const int32_t* corr_idx, int64_t n, int32_t* pairs_out, int64_t* count,
                   void* stream);
/* Device pointer to the current correspondence index array (ns int32, -1 = none) in SOURCE SLOT
 * order (see m3d_icp_copy_slots); m3d_icp_copy_corr gives it in source order. */
const int32_t* m3d_icp_corr(const m3d_icp* s);
/* Copy the current correspondence array to dst [device] (ns int32, source order: dst[i] = target
 * index of source point i, -1 = none). */
int m3d_icp_copy_corr(const m3d_icp* s, int32_t* dst, void* stream);
/* dst [device] ns int32: dst[k] = the source point index held in slot k (ABI 8). */
int m3d_icp_copy_slots(const m3d_icp* s, int32_t* dst, void* stream);

/* ------------------------------------------------------------------ Generalized ICP (gicp.hip)
 * Open3D 0.19 registration_generalized_icp (GeneralizedICP.cpp, plane-to-plane), restated in
 * tests/gicp_restatement.py; added within ABI 13, the version number is unchanged.  It is
 * RegistrationICP with another ComputeTransformation: the NN search, the loop's transformed copy
 * of the source and the convergence rule are m3d_icp_run's.
 *
 * Covariances: every point carries a 3x3 covariance.  From a unit normal n
 * (InitializePointCloudForGeneralizedICP):  C = Rx diag(epsilon, 1, 1) Rx^T with
 * Rx = GetRotationFromE1ToX(n):  v = e1 x n, c = e1 . n;  Rx = I when c < -0.99, else
 * Rx = I + [v]x + [v]x^2 / (1 + c).  The library holds a covariance as its upper triangle (the
 * lower one is its mirror): of a caller's row-major 3x3 it reads entries 0 1 2 4 5 8.
 *
 * One update over the correspondence set, vs / Cs the loop's transformed source point and
 * covariance (every update dT rotates the covariances too, C <- R C R^T), vt / Ct the target's:
 *   d = vs - vt, M = Ct + Cs, J0 = [-[vs]x | I] (3x6),
 *   JtJ = sum J0^T M^-1 J0, Jtr = sum J0^T M^-1 d, sum r^2 = sum d^T M^-1 d
 * (Open3D's residual rows W d and Jacobian rows W J0 with W = M^(-1/2), unit weights), solved and
 * turned into dT exactly as point-to-plane (JtJ x = -Jtr, LDLT, TransformVector6dToMatrix4d); the
 * identity for an empty set.  fitness and inlier_rmse come from the NN distances.  All sums are
 * fp64 and added in a fixed order: both nn_methods, and repeated calls, return the same bits. */

/* cov_out[i] = the covariance of normals[i] (formula above).  normals [device] n x 3 f64, cov_out
 * [device] n x 9 f64 row-major (exactly symmetric).  M3D_ERR_INVALID for epsilon <= 0.  Only
 * enqueues work on stream. */
int m3d_covariances_from_normals(m3d_ctx* ctx, const double* normals, int64_t n, double epsilon,
                                 double* cov_out, void* stream);

/* One evaluation: the source (points and covariances) transformed by T_host [host] 16 f64 (NULL =
 * identity) only when T_host is not Eigen-isIdentity(), the radius-bounded exact 1-NN of m3d_nn1,
 * then the 30 sums over the matched pairs in the point-to-plane slot layout: sums_out [host] 32
 * f64 = JtJ upper triangle row-major (0..20), Jtr (21..26), sum r^2 (27), count (28), sum d^2
 * (29), 0, 0 — what a Gauss-Newton step of the caller's own needs (m3d_icp_solve takes the same
 * layout).  src_cov / tgt_cov [device] n x 9 f64 row-major in the cloud's point order, or NULL =
 * from the cloud's normals with epsilon (M3D_ERR_INVALID when it has none).  corr_idx [device] ns
 * int32 or NULL: the matched target per source in the caller's order (-1 = none).  An empty
 * source or target gives zeros.  M3D_ERR_INVALID for epsilon <= 0, max_dist <= 0 or an unknown
 * nn_method; M3D_ERR_HIP when the grid NN's deferral list overflowed.  Synchronous. */
int m3d_gicp_terms(m3d_ctx* ctx, const m3d_cloud* src, const m3d_cloud* tgt, const double* src_cov,
                   const double* tgt_cov, const double* T_host, double max_dist, int32_t nn_method,
                   double epsilon, double* sums_out, int32_t* corr_idx, void* stream);

typedef struct {
  double relative_fitness; /* ICPConvergenceCriteria defaults 1e-6 */
  double relative_rmse;    /* 1e-6 */
  int32_t max_iteration;   /* 30 */
  int32_t nn_method;       /* M3D_NN_* */
  double epsilon;          /* covariances from normals: 1e-3 */
} m3d_gicp_params;

/* registration_generalized_icp.  init [host] 16 f64 (applied to points and covariances unless
 * isIdentity()); src_cov / tgt_cov as in m3d_gicp_terms; out->T, fitness, inlier_rmse,
 * num_correspondences, iterations, converged, update as m3d_icp_run fills them; corr_idx [device]
 * ns int32 or NULL: the final correspondence per source (-1 = none).  The loop runs on one device,
 * enqueued in growing chunks with a look at the state's `done` in between, as m3d_icp_run.
 * M3D_ERR_INVALID as m3d_gicp_terms, and for max_iteration < 0; M3D_ERR_HIP for a deferral-list
 * overflow, as m3d_icp_result_get reports it.  Synchronous. */
int m3d_gicp_run(m3d_ctx* ctx, const m3d_cloud* src, const m3d_cloud* tgt, const double* src_cov,
                 const double* tgt_cov, const double* init, double max_dist, const m3d_gicp_params* params,
                 m3d_icp_result* out, int32_t* corr_idx, void* stream);

/* ------------------------------------------------------------------ robust kernels (robust.hip)
 * Open3D 0.19 RobustKernel.cpp inside TransformationEstimationPointToPlane(kernel) and
 * TransformationEstimationForGeneralizedICP(epsilon, kernel), restated in
 * tests/robust_restatement.py; added within ABI 13, the version number is unchanged.  A residual r
 * gets the weight w(r), k the kernel's scale:
 *   L2 1 | L1 1/|r| | Huber k/max(|r|, k) | Cauchy 1/(1 + (r/k)^2) | GM k/(k + r^2)^2 |
 *   Tukey (1 - min(1, |r/k|)^2)^2
 * and a row (J, r) adds w J J^T to JtJ, w J r to Jtr and r^2 (unweighted) to sum r^2.
 * Point-to-plane has one row per matched pair: r = (vs - vt) . nt, J = [vs x nt | nt].
 * Generalized ICP has three, each weighted on its own: W = (Ct + Cs)^(-1/2), the symmetric root,
 * r_j = W.row(j) d, J_j = (W J0).row(j).  L1 at r = 0 gives an infinite weight, literally: the
 * update is then non-finite and the loop replaces it by the identity, as for any non-finite
 * update.  Everything else (NN search, transformed copy, fitness / inlier_rmse from the NN
 * distances, convergence rule, LDLT solve, slot layout, fixed summation order) is m3d_icp_run's. */
#define M3D_KERNEL_L2 0
#define M3D_KERNEL_L1 1
#define M3D_KERNEL_HUBER 2
#define M3D_KERNEL_CAUCHY 3
#define M3D_KERNEL_GM 4
#define M3D_KERNEL_TUKEY 5

typedef struct {
  int32_t kind; /* M3D_KERNEL_L2 .. M3D_KERNEL_TUKEY */
  double k;     /* the scale; read by Huber, Cauchy, GM and Tukey: finite and > 0 */
} m3d_robust_kernel;

/* One point-to-plane evaluation with `kernel`, as m3d_gicp_terms: T_host applied unless
 * isIdentity(), the exact radius 1-NN, then sums_out [host] 32 f64 in the same layout.  Here, and
 * only here, kind L2 also runs through robust.hip's pass (its check against the point-to-plane
 * oracle).  M3D_ERR_INVALID for an unknown kind, a k <= 0 or non-finite for a kind that reads k, a
 * target without normals, max_dist <= 0 or an unknown nn_method.  Synchronous. */
int m3d_robust_terms(m3d_ctx* ctx, const m3d_cloud* src, const m3d_cloud* tgt, const double* T_host,
                     double max_dist, int32_t nn_method, const m3d_robust_kernel* kernel, double* sums_out,
                     int32_t* corr_idx, void* stream);

/* registration_icp with TransformationEstimationPointToPlane(kernel): m3d_icp_run's loop with the
 * robust point-to-plane terms, three launches per iteration.  params->estimation must be
 * M3D_EST_POINT_TO_PLANE (TransformationEstimationPointToPoint takes no kernel); other errors as
 * m3d_robust_terms and m3d_icp_run.  Synchronous. */
int m3d_robust_icp_run(m3d_ctx* ctx, const m3d_cloud* src, const m3d_cloud* tgt, const double* init,
                       double max_dist, const m3d_icp_params* params, const m3d_robust_kernel* kernel,
                       m3d_icp_result* out, int32_t* corr_idx, void* stream);

/* m3d_gicp_terms / m3d_gicp_run with a kernel (NULL or kind L2: exactly those calls). */
int m3d_gicp_terms_robust(m3d_ctx* ctx, const m3d_cloud* src, const m3d_cloud* tgt, const double* src_cov,
                          const double* tgt_cov, const double* T_host, double max_dist, int32_t nn_method,
                          double epsilon, const m3d_robust_kernel* kernel, double* sums_out, int32_t* corr_idx,
                          void* stream);
int m3d_gicp_run_robust(m3d_ctx* ctx, const m3d_cloud* src, const m3d_cloud* tgt, const double* src_cov,
                        const double* tgt_cov, const double* init, double max_dist,
                        const m3d_gicp_params* params, const m3d_robust_kernel* kernel, m3d_icp_result* out,
                        int32_t* corr_idx, void* stream);

/* ------------------------------------------------------------------ Colored ICP (colored.hip)
 * Open3D 0.19 registration_colored_icp (ColoredICP.cpp; Park, Zhou, Koltun 2017), restated in
 * tests/colored_restatement.py; added within ABI 13, the version number is unchanged.  It is
 * RegistrationICP with another ComputeTransformation: the NN search, the loop's transformed copy
 * of the source, fitness, the geometric inlier_rmse = sqrt(sum d^2 / count) and the convergence
 * rule are m3d_icp_run's.  Colours are n x 3 f64 in [0, 1] in the cloud's point order; the
 * intensity of a point is I = (r + g + b) / 3.
 *
 * Gradient of a target point (vt, unit normal nt, intensity it): its hybrid neighbour list (the
 * max_nn nearest with d^2 < radius^2, itself included, ordered by (d^2, index): m3d_hybrid_search's
 * list) of length nn; nn < 4 gives 0.  Else entry 0 is skipped whatever it is (Open3D's loop
 * starts at 1; among exact duplicates of the query FLANN's order is unpinned, here the lowest index
 * leads), every other entry p, ip gives the row A = (p - ((p - vt) . nt) nt) - vt, b = ip - it,
 * one more row is A = (nn - 1) nt, b = 0, and the gradient solves (A^T A) x = A^T b by LDLT.
 * Departure: a pivot that is not positive and finite, or a non-finite solution, gives 0.
 *
 * Terms of a matched pair (moved source vs, intensity is; target vt, nt, it, gradient dit), sg =
 * sqrt(lambda_geometric), sp = sqrt(1 - lambda_geometric):
 *   r0 = sg (vs - vt) . nt,            J0 = sg [vs x nt | nt]
 *   proj = vs - ((vs - vt) . nt) nt,   is0 = dit . (proj - vt) + it,   ditM = -(I - nt nt^T) dit
 *   r1 = sp (is - is0),                J1 = sp [vs x ditM | ditM]
 * each row weighted on its own by the robust kernel (NULL or L2: 1) and added as the robust
 * point-to-plane row is: w J J^T, w J r, r^2 unweighted.  All sums are fp64 and added in a fixed
 * order: both nn_methods, and repeated calls, return the same bits. */

/* out[i] = the colour gradient of point i.  cloud must carry normals; colors [device] n x 3 f64,
 * out [device] n x 3 f64.  M3D_ERR_INVALID for radius <= 0, max_nn outside [1, 64] (one list entry
 * per lane of a wave), a cloud without normals or null colours.  An empty cloud launches nothing.
 * Synchronous. */
int m3d_color_gradients(m3d_ctx* ctx, const m3d_cloud* cloud, const double* colors, double radius,
                        int32_t max_nn, double* out, void* stream);

/* One evaluation, as m3d_gicp_terms: T_host applied unless isIdentity(), the exact radius 1-NN,
 * then sums_out [host] 32 f64 in the point-to-plane slot layout.  src_colors / tgt_colors [device]
 * n x 3 f64; tgt_gradient [device] nt x 3 f64 or NULL = computed with radius 2 max_dist, max_nn 30
 * (KDTreeSearchParamHybrid).  kernel NULL or kind L2: unit weights.  corr_idx [device] ns int32 or
 * NULL.  An empty source or target gives zeros.  M3D_ERR_INVALID for max_dist <= 0,
 * lambda_geometric outside [0, 1], an unknown nn_method, a target without normals, null colours
 * of a non-empty cloud, or a bad kernel; M3D_ERR_HIP when the grid NN's deferral list overflowed.
 * Synchronous. */
int m3d_colored_terms(m3d_ctx* ctx, const m3d_cloud* src, const m3d_cloud* tgt, const double* src_colors,
                      const double* tgt_colors, const double* tgt_gradient, const double* T_host,
                      double max_dist, int32_t nn_method, double lambda_geometric,
                      const m3d_robust_kernel* kernel, double* sums_out, int32_t* corr_idx, void* stream);

typedef struct {
  double lambda_geometric; /* 0.968 */
  double relative_fitness; /* ICPConvergenceCriteria defaults 1e-6 */
  double relative_rmse;    /* 1e-6 */
  int32_t max_iteration;   /* 30 */
  int32_t nn_method;       /* M3D_NN_* */
} m3d_colored_params;

/* registration_colored_icp.  The target's gradients are built once (or taken from tgt_gradient),
 * then the loop runs as m3d_gicp_run does: three launches per iteration, enqueued in growing
 * chunks with a look at the state's `done` in between.  out and corr_idx as m3d_icp_run fills
 * them.  M3D_ERR_INVALID as m3d_colored_terms, and for max_iteration < 0; M3D_ERR_HIP for a
 * deferral-list overflow, as m3d_icp_result_get reports it.  Synchronous. */
int m3d_colored_icp_run(m3d_ctx* ctx, const m3d_cloud* src, const m3d_cloud* tgt, const double* src_colors,
                        const double* tgt_colors, const double* tgt_gradient, const double* init,
                        double max_dist, const m3d_colored_params* params, const m3d_robust_kernel* kernel,
                        m3d_icp_result* out, int32_t* corr_idx, void* stream);

/* ------------------------------------------------------------------ preprocessing
 * Open3D 0.19 semantics restated (oracle/prep_oracle.py); all fp64. */

/* PointCloud::VoxelDownSample (src/ply/ply.py:106).  xyz [device] n×3, normals [device] n×3 or
 * NULL; out_xyz / out_normals [device] with room for n×3; *out_n [host] = voxels.  Voxels come in
 * ascending (ix, iy, iz) order (Open3D: unordered_map order, unspecified).  Synchronous. */
int m3d_voxel_down_sample(m3d_ctx* ctx, const double* xyz, const double* normals, int64_t n,
                          double voxel_size, double* out_xyz, double* out_normals, int64_t* out_n,
                          void* stream);
/* KDTreeFlann::SearchHybrid(p_i, radius, max_nn) for every point of the cloud (strict d² < r²,
 * ascending (d², index)).  idx [device] n×max_nn int32 (-1 pad), d2 [device] n×max_nn f64,
 * count [device] n int32.  Synchronous. */
int m3d_hybrid_search(m3d_ctx* ctx, const m3d_cloud* cloud, double radius, int32_t max_nn,
                      int32_t* idx, double* d2, int32_t* count, void* stream);
/* PointCloud::EstimateNormals(KDTreeSearchParamHybrid(radius, max_nn)) (ply.py:110-112,133-135):
 * covariance of the hybrid neighbourhood → FastEigen3x3; the cloud's own normals, if any, orient
 * the result.  normals_out [device] n×3.  Synchronous. */
int m3d_estimate_normals(m3d_ctx* ctx, const m3d_cloud* cloud, double radius, int32_t max_nn,
                         double* normals_out, void* stream);
/* ComputeFPFHFeature(cloud, KDTreeSearchParamHybrid(radius, max_nn)) (ply.py:117-120).
 * normals [device] n×3; fpfh_out [device] n×33 row-major (Open3D's Feature.data is 33×n).
 * Synchronous. */
int m3d_compute_fpfh(m3d_ctx* ctx, const m3d_cloud* cloud, const double* normals, double radius,
                     int32_t max_nn, double* fpfh_out, void* stream);

/* ------------------------------------------------------------------ outlier removal (clean.hip)
 * What Open3D users run on a raw scan before registering it; the reference's Ply has no such step.
 * Exact fp64, d² = (dx·dx + dy·dy) + dz·dz, finite coordinates assumed. */

/* KDTreeFlann::SearchKNN(p_i, k) for every point of the cloud, the point itself included: the
 * min(k, n) lexicographically smallest (d², index) pairs over ALL points (no radius bound; ties by
 * lower index).  idx [device] n×k int32 (-1 pad), d2 [device] n×k f64 (INFINITY pad), count
 * [device] n int32 (= min(k, n)).  1 <= k <= 256 (else M3D_ERR_INVALID).  Synchronous. */
int m3d_knn_search(m3d_ctx* ctx, const m3d_cloud* cloud, int32_t k, int32_t* idx, double* d2,
                   int32_t* count, void* stream);

/* PointCloud::EstimateNormals(KDTreeSearchParamKNN(k)) — what registration_generalized_icp runs
 * (k = 20) on a cloud that has neither covariances nor normals: the covariance of each point's
 * m3d_knn_search list (the point itself included) -> FastEigen3x3, as m3d_estimate_normals does
 * with its hybrid list; fewer than 3 neighbours (k < 3 or n < 3) give (0, 0, 1); the cloud's own
 * normals, if any, orient the result.  normals_out [device] n x 3.  1 <= k <= 256.  Synchronous. */
int m3d_estimate_normals_knn(m3d_ctx* ctx, const m3d_cloud* cloud, int32_t k, double* normals_out,
                             void* stream);

/* PointCloud::RemoveStatisticalOutliers(nb_neighbors, std_ratio) (Open3D 0.19):
 *   avg[i]    = (Σ sqrt(d²) over point i's SearchKNN(nb_neighbors) list, in list order) / count,
 *   valid     = points with a non-empty list (n), mean = Σ{avg > 0} / valid,
 *   std_dev   = sqrt(Σ{(avg − mean)² : avg > 0} / (valid − 1)), threshold = mean + std_ratio·std_dev,
 *   kept      iff avg > 0 && avg < threshold
 * (so a point whose neighbours all coincide with it is dropped, nb_neighbors = 1 drops every point,
 * n = 1 gives a NaN threshold and nothing kept, n = 0 nothing without touching the device).
 * index_out [device] room for n int32: the kept indices in ascending order; *n_out [host] = their
 * number; stats [host] or NULL; avg_out [device] n f64 or NULL.  The sums are fp64 in a fixed
 * order: repeated calls return the same bits.  M3D_ERR_INVALID for nb_neighbors < 1 (or > 256)
 * or std_ratio <= 0 (Open3D: "Illegal input parameters").  Synchronous. */
typedef struct {
  int64_t kept, valid;
  double mean, std_dev, threshold;
} m3d_outlier_stats;
int m3d_remove_statistical_outlier(m3d_ctx* ctx, const m3d_cloud* cloud, int32_t nb_neighbors,
                                   double std_ratio, int32_t* index_out, int64_t* n_out,
                                   m3d_outlier_stats* stats, double* avg_out, void* stream);

/* PointCloud::RemoveRadiusOutliers(nb_points, radius): count[i] = #{j : d²(i, j) < radius²}
 * (strict, the point itself included); kept iff count[i] > nb_points.  index_out [device] room
 * for n int32: the kept indices in ascending order; *n_out [host]; count_out [device] n int32 or
 * NULL (given: every count is complete; NULL: a point's count stops once it exceeds nb_points).
 * M3D_ERR_INVALID for nb_points < 1 or radius <= 0.  Synchronous. */
int m3d_remove_radius_outlier(m3d_ctx* ctx, const m3d_cloud* cloud, int32_t nb_points, double radius,
                              int32_t* index_out, int64_t* n_out, int32_t* count_out, void* stream);

/* ------------------------------------------------------------------ plane segmentation (plane.hip)
 * PointCloud::SegmentPlane(distance_threshold, ransac_n, num_iterations, probability) (Open3D 0.19)
 * — the support plane of a scan, removed before the scan is registered.  All arithmetic is fp64 on
 * the cloud's original coordinates, every operation rounded on its own, in the order written:
 *   dist(π, p) = |((a·x + b·y) + c·z) + d|
 *   ransac_n == 3: e0 = p1 − p0, e1 = p2 − p0, abc = e0 × e1, norm = sqrt((abc.x² + abc.y²) + abc.z²);
 *                  norm == 0: the zero plane, else abc /= norm, d = −((abc.x·p0.x + abc.y·p0.y) + abc.z·p0.z)
 *   ransac_n  > 3: GetPlaneFromPoints over the sample in sample order — centroid = (Σp)/m, the six
 *                  sums of products of r = p − centroid, the largest of det_x, det_y, det_z picks the
 *                  axis, norm == 0: the zero plane, else abc /= norm, d = −abc·centroid
 * The loop is sequential over h = 0 … num_iterations − 1 with best_count = 0, best_rmse = 0,
 * best_index = −1, break_it = +inf, evaluated = 0:
 *   if evaluated > break_it: stop
 *   π = plane of sample h; all zero: continue (not counted)
 *   count = #{i : dist < thr}, err = Σ dist² over those, rmse = count ? err / sqrt(count) : 0
 *   count > best_count or (count == best_count and rmse < best_rmse):
 *     best ← (count, rmse, π, h); f = count / n;
 *     break_it = f < 1 ? trunc(min(log(1 − probability) / log(1 − pow(f, ransac_n)), num_iterations)) : 0
 *   evaluated += 1
 * then inliers = {i : dist(best plane, p_i) < thr} ascending and plane = GetPlaneFromPoints(inliers)
 * (two fixed-order fp64 reductions: repeated calls return the same bits); no best, or fewer than 3
 * inliers: the zero plane.  Samples: the caller's (`samples`) or the counter sampler of
 * m3d_kabsch3_batch generalised to ransac_n distinct indices. */
typedef struct {
  double distance_threshold;  /* Open3D default 0.01 */
  double probability;         /* 0.99999999 */
  uint64_t seed;              /* native sampler; ignored with samples */
  int32_t ransac_n;           /* 3 */
  int32_t num_iterations;     /* 100 */
  int32_t batch;              /* hypotheses per device batch, 0 = automatic; changes no result */
  int32_t reserved;
} m3d_plane_params;
typedef struct {
  double plane[4];         /* refit over the inliers (what Open3D returns) */
  double ransac_plane[4];  /* the best hypothesis's own plane (the one the inliers are tested against) */
  int64_t num_inliers, best_index, best_count, evaluated, iterations /* h at exit */;
  double best_rmse;
} m3d_plane_result;
/* samples [device] num_iterations × ransac_n int32 or NULL (native sampler); inliers_out [device]
 * room for n int32; counts_out [device] num_iterations int32 or NULL (−1 = degenerate or not
 * reached); err_out [device] num_iterations f64 or NULL (same rows, −1 likewise).
 * M3D_ERR_INVALID: ransac_n < 3 or > 32, n < ransac_n, probability <= 0 or > 1, num_iterations < 0,
 * distance_threshold negative or not finite, a sample index outside [0, n) (found on the device
 * before any point is read).  Synchronous. */
int m3d_segment_plane(m3d_ctx* ctx, const m3d_cloud* cloud, const m3d_plane_params* params,
                      const int32_t* samples, m3d_plane_result* out, int32_t* inliers_out,
                      int32_t* counts_out, double* err_out, void* stream);
/* Score H given planes: planes [device] H×4 f64 → counts [device] H int32, err [device] H f64 or
 * NULL.  A plane's count and err do not depend on H or on the planes beside it.  Only enqueues
 * work on stream; H == 0 or an empty cloud: nothing is touched. */
int m3d_plane_score(m3d_ctx* ctx, const m3d_cloud* cloud, const double* planes, int64_t H,
                    double distance_threshold, int32_t* counts, double* err, void* stream);
/* points per chunk of the score kernel's partial sums: a constant of the library (err is the
 * sequential sum inside a chunk, the chunk sums are added in a fixed order) */
int32_t m3d_plane_chunk(void);

/* ------------------------------------------------------------------ DBSCAN clustering (cluster.hip)
 * PointCloud::ClusterDBSCAN(eps, min_points) (Open3D 0.19) — what is left of a scan once its support
 * plane is gone, split into the object and the rest.
 *   nbs[i] = {j : d²(i, j) < eps²}: strict, the point itself included,
 *            d² = (dx·dx + dy·dy) + dz·dz in fp64 on the cloud's original coordinates
 *   core[i] = |nbs[i]| >= min_points
 * Open3D labels the points in index order, growing a cluster from every still unlabelled core
 * point through the neighbourhoods of the core points it reaches; whatever order its set pops in,
 * the labels are
 *   core point:   the rank of its connected component in the graph on the core points whose edges
 *                 join core pairs with d² < eps², components ranked by their smallest member index
 *   border point: (not core, at least one core point in nbs) the smallest label among its core
 *                 neighbours
 *   other points: −1 (noise)
 * and these are what the device computes (three box scans on the grid of cell eps and a lock-free
 * union–find with integer atomics only: repeated calls return the same bits).  The grid is cached
 * on the cloud like the radius filter's. */
typedef struct {
  int64_t num_clusters, num_core, num_noise;
  int64_t largest_label;  /* biggest cluster, lowest label on ties; -1 without a cluster */
  int64_t largest_size;
} m3d_dbscan_result;
/* labels_out [device] n int32 (-1 = noise); sizes_out [device] room for n int32 or NULL
 * (entries [0, num_clusters) are written); count_out [device] n int32 or NULL: every point's full
 * neighbour count (NULL: a count stops at min_points).  n == 0: zeros, no device work.
 * M3D_ERR_INVALID: eps not finite or <= 0, min_points < 1.  Synchronous. */
int m3d_cluster_dbscan(m3d_ctx* ctx, const m3d_cloud* cloud, double eps, int32_t min_points,
                       int32_t* labels_out, m3d_dbscan_result* out, int32_t* sizes_out,
                       int32_t* count_out, void* stream);

/* ------------------------------------------------------------------ ISS keypoints (iss.hip)
 * keypoint::ComputeISSKeypoints(input, salient_radius = 0, non_max_radius = 0, gamma_21 = 0.975,
 * gamma_32 = 0.975, min_neighbors = 5) (Open3D 0.19) — the few hundred repeatable points of a scan
 * whose FPFH rows go to the global registration.
 *   d²(i, j) = (dx·dx + dy·dy) + dz·dz in fp64 on the cloud's original coordinates, no contraction
 * Radii.  salient_radius == 0 or non_max_radius == 0 replaces BOTH: salient_radius = 6·res,
 *   non_max_radius = 4·res, res = (Σ_i sqrt(d² to the nearest other point)) / n — Open3D's
 *   ComputeModelResolution (SearchKNN(2), entry 1).  The per-point values are exact (the k-NN ladder
 *   at k = 2); the sum is the fixed-order fp64 reduction of the outlier statistics (256-point
 *   blocks, then one block; no floating-point atomics: repeated calls return the same bits).
 *   n = 1: res = 0.  A resolved radius of 0: no keypoints, no scan.
 * Saliency, for every i with S(i) = {j : d²(i, j) < salient_radius²} (strict, i itself included):
 *   count[i] = |S(i)|; fewer than min_neighbors: third[i] = 0
 *   the covariance of S(i), centred on the query: d = p_j − p_i in fp64, S1 = Σd, S2 = Σd dᵀ,
 *     m = S1 / count, C = S2 / count − m mᵀ;  all |C_ab| <= 1e-12 (Eigen's isZero): third[i] = 0
 *   λ0 <= λ1 <= λ2 the eigenvalues of C;  salient iff λ1 / λ2 < gamma_21 && λ0 / λ1 < gamma_32
 *     (the divisions as written: a NaN compares false);  third[i] = λ0 if salient, else 0
 * Non-maximum, for every i with third[i] > 0 and N(i) = {j : d²(i, j) < non_max_radius²}: i is a
 *   keypoint iff |N(i)| >= min_neighbors and no j in N(i) has S(j) != S(i) and third[j] > third[i].
 * Output: the keypoint indices, ascending (Open3D's order is that of its OpenMP critical section).
 *
 * Two deliberate differences from Open3D's arithmetic:
 * 1. Centred moments.  Open3D's ComputeCovariance sums raw coordinates and subtracts; against an
 *    80-bit reference its eigenvalues are off by 1.2e-11·λ2 on a unit shell near (10, −4, 2.5) and by
 *    9.8e-8·λ2 on a cloud offset by 500.  The centred fp64 sums stay within 2.1e-15·λ2 whatever the
 *    order of summation: the same quantity without the cancellation.
 * 2. The same-set rule (S(j) != S(i) above).  Two nearby points very often have the identical
 *    neighbour set; the covariance is translation invariant, so in exact arithmetic their third
 *    values are equal, neither is < the other and both can be keypoints.  Open3D decides such pairs
 *    by the rounding of two differently ordered sums of the same numbers (2.5–6 % of the points of
 *    the test clouds sit within 1e-12·λ2 of such a tie).  The device never compares third across
 *    equal sets.  It tells sets apart by a per-point integer signature (count, Σ_{j in S} mix64(j)
 *    mod 2⁶⁴, mix64 = splitmix64's finaliser): order independent, integer adds only.  Equal
 *    signatures are treated as equal sets; two different sets of equal size collide with
 *    probability 2⁻⁶⁴ per compared pair. */
typedef struct {
  double salient_radius, non_max_radius; /* 0: from the model resolution (see above) */
  double gamma_21, gamma_32;
  int32_t min_neighbors;
} m3d_iss_params;
typedef struct {
  int64_t num_keypoints;
  int64_t num_salient;  /* points with third > 0: the candidates of the non-maximum pass */
  int64_t num_counted;  /* points with count >= min_neighbors */
  double salient_radius, non_max_radius; /* as used */
  double resolution;    /* 0 when not computed */
} m3d_iss_result;
/* res_out [host].  n == 0: 0, no device work.  Synchronous. */
int m3d_model_resolution(m3d_ctx* ctx, const m3d_cloud* cloud, double* res_out, void* stream);
/* index_out [device] room for n int32 (entries [0, num_keypoints) are written); third_out [device] n
 * doubles or NULL; count_out [device] n int32 or NULL (zeros when a resolved radius is 0).
 * n == 0: zeros, no device work.  M3D_ERR_INVALID: a radius negative or not finite, a gamma not
 * finite, min_neighbors < 0.  Synchronous; the grids of cell salient_radius and non_max_radius are
 * cached on the cloud like the radius filter's. */
int m3d_compute_iss_keypoints(m3d_ctx* ctx, const m3d_cloud* cloud, const m3d_iss_params* params,
                              m3d_iss_result* out, int32_t* index_out, double* third_out,
                              int32_t* count_out, void* stream);

/* ------------------------------------------------------------------ feature matching (a5, a6) */

/* CorrespondencesFromFeatures (src/matcher/ransac.py:85): exact fp64 1-NN in feature space
 * (lowest index on ties), optional mutual filter with Open3D's fallback to the one-directional
 * set below mutual_consistent_ratio·ns pairs.  f_src [device] ns×dim, f_tgt [device] nt×dim
 * (dim = 33), corr_out [device] room for ns×2 int32, *n_out [host].  Synchronous. */
int m3d_feature_correspondences(m3d_ctx* ctx, const double* f_src, int64_t ns, const double* f_tgt,
                                int64_t nt, int32_t dim, int32_t mutual_filter,
                                double mutual_consistent_ratio, int32_t* corr_out, int64_t* n_out,
                                void* stream);

typedef struct {
  double max_correspondence_distance; /* ransac.py:41 1.5·v */
  double confidence;                  /* RANSACConvergenceCriteria.confidence (0.999) */
  double edge_length;                 /* CorrespondenceCheckerBasedOnEdgeLength (0.9); <= 0 off */
  double distance;                    /* CorrespondenceCheckerBasedOnDistance (1.5·v); <= 0 off */
  uint64_t seed;                      /* counter sampler seed */
  int32_t max_iteration;              /* RANSACConvergenceCriteria.max_iteration (30) */
  int32_t ransac_n;                   /* 3 (only value supported; < 3 → empty result) */
} m3d_feature_ransac_params;

typedef struct {
  double T[16];
  double fitness;
  double inlier_rmse;
  int64_t best_index;  /* hypothesis id of the best, -1 = none */
  int64_t validations; /* hypotheses that passed the checkers and were validated */
  double corres_ratio; /* the best's correspondence inlier ratio (the exit estimate's input; ABI 10) */
} m3d_feature_ransac_result;

/* RegistrationRANSACBasedOnCorrespondence (ransac.py:44-58 → Open3D): PointToPoint (no scaling),
 * rows drawn with replacement by the counter sampler, checkers, validation over all source
 * points (1-NN within max_correspondence_distance), IsBetterRANSACThan, early exit as Open3D
 * 0.19: after each new best k = ceil(log(1-c)/log(1-ratio^3)) with ratio = the share of the nc
 * input correspondences within max_correspondence_distance under that best (Registration.cpp
 * EvaluateInlierCorrespondenceRatio; ABI 10 — ABI ≤ 9 used the fitness).
 * corr [device] nc×2 int32 (source, target) rows.
 * corr_set_out [device] ns int32 or NULL: the best transform's correspondence per source point
 * (-1 none).  Synchronous. */
int m3d_ransac_on_correspondences(m3d_ctx* ctx, const m3d_cloud* src, const m3d_cloud* tgt,
                                  const int32_t* corr, int64_t nc,
                                  const m3d_feature_ransac_params* params,
                                  m3d_feature_ransac_result* out, int32_t* corr_set_out,
                                  void* stream);

/* ------------------------------------------------------------------ Fast Global Registration (fgr.hip)
 * Open3D 0.19 FastGlobalRegistration.cpp (Zhou, Park, Koltun) restated; tests/fgr_restatement.py is
 * the same text in numpy.  fp64 throughout, every operation rounded on its own in the order written.
 *   normalise   m0 = mean(S), m1 = mean(G); scale = max over both centred clouds of √((x² + y²) + z²);
 *               use_absolute_scale ? (g = 1, par₀ = scale) : (g = scale, par₀ = 1);
 *               P = (S − m0) / g, Q = (G − m1) / g
 *   tuple test  (tuple_test) with n rows, trials h = 0 … 100·n − 1 in order, each drawing three rows
 *               with replacement from the counter sampler of m3d_ransac_on_correspondences
 *               (base = splitmix64(seed ^ h·0x9E3779B97F4A7C15), row_k = ((splitmix64(base + k) >> 32)·n) >> 32);
 *               edges li = |P[i0] − P[i1]|, |P[i1] − P[i2]|, |P[i2] − P[i0]| (√((dx² + dy²) + dz²)), lj the
 *               same over Q; accepted iff li_k·tuple_scale < lj_k && lj_k < li_k / tuple_scale for all k;
 *               an accepted trial appends its three rows; the loop stops after the trial that brings
 *               the accepted count to >= maximum_tuple_count (0: after the first accepted trial).  The
 *               appended rows replace the row set, duplicates stay.
 *   optimise    fewer than 10 rows: T = I.  Else par = par₀, p_c = P[i_c], q_c = Q[j_c] (a copy that
 *               moves), and iteration_number times: r = p − q, s = (par / (((r_x² + r_y²) + r_z²) + par))²,
 *               JᵀJ = Σ s·J Jᵀ, Jᵀr = Σ s·J r over the rows Jx = (0, −q_z, q_y, −1, 0, 0),
 *               Jy = (q_z, 0, −q_x, 0, −1, 0), Jz = (−q_y, q_x, 0, 0, 0, −1); JᵀJ x = −Jᵀr by the ICP
 *               solve (unpivoted LDLᵀ while safe, else Eigen's pivot order; a non-finite δ is I),
 *               δ = TransformVector6dToMatrix4d(x), T ← δ·T, q_c ← δ·q_c; then, if decrease_mu and
 *               itr % 4 == 0 and par > maximum_correspondence_distance: par /= division_factor.
 *   result      T = (R, t) maps the normalised target onto the normalised source;
 *               O = (R, ((−R·m1) + g·t) + m0); the transformation returned is O⁻¹ = (Rᵀ, −Rᵀ·o);
 *               fitness, inlier_rmse and the correspondence set are m3d_evaluate_registration's at
 *               maximum_correspondence_distance under O⁻¹ (radius <= 0: zeros, no pairs).
 * Every sum (the means, the loop's sums) is taken in one order that depends on the element count
 * alone: repeated calls, and both loop paths, return the same bits. */
typedef struct {
  double division_factor;                 /* 1.4 */
  double maximum_correspondence_distance; /* 0.025 */
  double tuple_scale;                     /* 0.95 */
  uint64_t seed;                          /* counter sampler seed (Open3D's seed=None: 0) */
  int32_t iteration_number;               /* 64 */
  int32_t maximum_tuple_count;            /* 1000 */
  int32_t use_absolute_scale;             /* 0 */
  int32_t decrease_mu;                    /* 0 */
  int32_t tuple_test;                     /* 1 */
  int32_t path;                           /* loop: 0 automatic, 1 one workgroup, 2 one launch per iteration */
} m3d_fgr_params;
typedef struct {
  double T[16];                /* source → target, original scale */
  double fitness, inlier_rmse;
  int64_t n_input, n_rows;     /* rows given; rows optimised over */
  int64_t tuples, trials;      /* accepted trials kept; trials the sequential loop ran */
  double par_final, scale_global;
  double mean_src[3], mean_tgt[3];
  double T_norm[16];           /* the loop's T (normalised target → normalised source) */
} m3d_fgr_result;
/* Steps normalise … result.  corr [device] nc×2 int32 (source, target) rows; rows_out [device] room
 * for 3·max(maximum_tuple_count, 1)×2 int32 (tuple test; never more than 300·nc×2) or nc×2, or NULL:
 * the row set optimised over; corr_set_out [device] ns int32 or NULL (−1 none).  An empty cloud gives
 * T = I and zeros.  M3D_ERR_INVALID: a row index outside its cloud (found on the device before a
 * point is read through it), path 1 with more rows than the one-workgroup loop holds, a
 * tuple_scale outside (0, 1], division_factor <= 0, negative counts.  Synchronous. */
int m3d_fgr_on_correspondences(m3d_ctx* ctx, const m3d_cloud* src, const m3d_cloud* tgt, const int32_t* corr,
                               int64_t nc, const m3d_fgr_params* params, m3d_fgr_result* out,
                               int32_t* rows_out, int32_t* corr_set_out, void* stream);
/* Steps normalise and tuple test alone: rows_out as above (required), *n_rows_out and *trials_out
 * [host].  Synchronous. */
int m3d_fgr_tuple_test(m3d_ctx* ctx, const m3d_cloud* src, const m3d_cloud* tgt, const int32_t* corr,
                       int64_t nc, const m3d_fgr_params* params, int32_t* rows_out, int64_t* n_rows_out,
                       int64_t* trials_out, void* stream);
/* One iteration's sums over n given rows: p, q [device] n×3 f64 → sums27_out [host]: the 21 entries
 * of JᵀJ's upper triangle (row-major) and the 6 of Jᵀr.  n == 0: zeros.  Synchronous. */
int m3d_fgr_terms(m3d_ctx* ctx, const double* p, const double* q, int64_t n, double par, double* sums27_out,
                  void* stream);
/* constants of the library: trials per batch of the tuple test; the most rows the one-workgroup
 * loop holds (the sum order's segment is a fixed fraction of it) */
int32_t m3d_fgr_trial_batch(void);
int32_t m3d_fgr_one_wg_rows(void);

/* ------------------------------------------------------------------ point-to-mesh distance
 * (added within ABI 13)  Open3D t.geometry.RaycastingScene.compute_closest_points /
 * compute_distance: for every query the closest triangle of a mesh.  The contract (mesh.hip):
 * Ericson's closest point on a triangle in fp64 in one fixed operation order, d² = the fp64
 * squared distance to it, the winner the smallest (d², triangle index) over every usable triangle
 * (nine finite coordinates, ab × ac not three exact zeros) whose d² is not NaN.  The brute-force
 * path and the grid path return the same bits.
 *
 * m3d_mesh_create: vertices [device] nv×3 f64, triangles [device] nf×3 int32 (both copied).
 * M3D_ERR_INVALID: an index outside [0, nv) (found on the device before a vertex is read through
 * it), nf >= 2^26.  Synchronous. */
int m3d_mesh_create(m3d_ctx* ctx, const double* vertices, int64_t nv, const int32_t* triangles, int64_t nf,
                    m3d_mesh** out);
void m3d_mesh_destroy(m3d_mesh* mesh);
int64_t m3d_mesh_size(const m3d_mesh* mesh); /* triangles (−1: null) */
/* xyz [device] n×3 f64 queries; T [host] 16 doubles (row-major 4×4: the query is
 * ((T00·x + T01·y) + T02·z) + T03, …) or NULL.  path: 0 automatic, 1 brute force, 2 grid.  r0: the
 * grid path's first radius (<= 0: one cell); it changes the rounds, never the result.  Outputs
 * [device], each may be NULL: d2_out n f64, tri_out n int32, point_out n×3 f64, uv_out n×2 f64
 * (v, w: point ≈ (1−v−w)·a + v·b + w·c), region_out n uint8 (0 1 2: vertex a b c; 3 4 5: edge ab ac
 * bc; 6: face).  A query no triangle answers (a NaN query): d² +inf, triangle −1, NaN point and uv,
 * region 255.  M3D_ERR_INVALID: the mesh has no usable triangle.  Synchronous. */
int m3d_mesh_closest(m3d_ctx* ctx, m3d_mesh* mesh, const double* xyz, int64_t n, const double* T, int32_t path,
                     double r0, double* d2_out, int32_t* tri_out, double* point_out, double* uv_out,
                     uint8_t* region_out, void* stream);
/* out4 [host]: the grid's cells and references (0 0 before the first grid query), the cell-size
 * doublings of its build, the ladder rounds of the last call (0: it ran brute force). */
int m3d_mesh_grid_info(const m3d_mesh* mesh, int64_t* out4);
/* constants of the library: triangles per LDS tile of the brute-force kernel; the triangle count up
 * to which path 0 takes it */
int32_t m3d_mesh_brute_tile(void);
int32_t m3d_mesh_auto_brute_max(void);

/* ------------------------------------------------------------------ ray casting (mesh_ray.hip)
 * (added within ABI 13, the version number is unchanged)  Open3D
 * t.geometry.RaycastingScene.cast_rays / count_intersections; occupancy and the sign of a signed
 * distance are the parity of the count.  The contract (mesh_ray.h, restated in numpy by
 * tests/mesh_ray_restatement.py), all in fp64, one operation at a time: a ray is (o, d); the test is
 * the watertight test of Woop, Benthin and Wald (2013):
 *   per ray       kz = the axis of the largest |d| (the lowest wins a tie), kx = (kz+1)%3,
 *                 ky = (kx+1)%3, swapped when d[kz] < 0; Sx = d[kx]/d[kz], Sy = d[ky]/d[kz], Sz = 1/d[kz].
 *   per triangle  A = a − o (B, C alike); Ax = A[kx] − Sx*A[kz], Ay = A[ky] − Sy*A[kz];
 *                 U = Cx*By − Cy*Bx, V = Ax*Cy − Ay*Cx, W = Bx*Ay − By*Ax; miss if one of them is < 0
 *                 and one > 0; det = (U+V)+W, miss if det == 0; Az = Sz*A[kz];
 *                 t = ((U*Az + V*Bz) + W*Cz) / det; hit iff tnear <= t && t <= tfar;
 *                 (u, v) = (V/det, W/det): point ≈ (1−u−v)·a + u·b + v·c.
 * Both orientations hit; t is in units of d, which need not be normalised.  A ray with a component
 * that is not finite or with d == 0 hits nothing; unusable triangles are skipped.  An edge value that
 * is exactly zero counts for both triangles of the edge (a ray from the centre of a unit cube along
 * +x, through a face diagonal, counts 2).  The brute-force path and the grid path (a walk of the
 * triangle grid along the ray) return the same bits.
 *
 * rays [device] n×6 f64 (origin, direction).  path: 0 automatic, 1 brute force, 2 grid.
 * m3d_mesh_cast_rays: the first hit, the smallest (t, triangle index); outputs [device], each may be
 * NULL: t_out n f64 (+inf on a miss), tri_out n int32 (−1), uv_out n×2 f64 (NaN).
 * m3d_mesh_count_rays: count_out [device] n int32, the usable triangles hit.
 * M3D_ERR_INVALID: the mesh has no usable triangle, an unknown path.  n == 0 returns at once.
 * Synchronous. */
int m3d_mesh_cast_rays(m3d_ctx* ctx, m3d_mesh* mesh, const double* rays, int64_t n, double tnear, double tfar,
                       int32_t path, double* t_out, int32_t* tri_out, double* uv_out, void* stream);
int m3d_mesh_count_rays(m3d_ctx* ctx, m3d_mesh* mesh, const double* rays, int64_t n, double tnear, double tfar,
                        int32_t path, int32_t* count_out, void* stream);
/* out2 [host]: the path the last ray call of the mesh ran (1 brute force, 2 grid; 0 before the
 * first), and how many of its rays took the whole-grid fallback (an origin farther than 2^18 times
 * the mesh's largest coordinate, or outside fp32's range). */
int m3d_mesh_ray_info(const m3d_mesh* mesh, int64_t* out2);
/* the triangle count up to which path 0 of the two ray calls runs brute force */
int32_t m3d_mesh_ray_auto_brute_max(void);

/* ------------------------------------------------------------------ surface sampling (mesh_sample.hip)
 * (added within ABI 13, the version number is unchanged)  Open3D
 * TriangleMesh.sample_points_uniformly: n points drawn from the mesh's surface with probability
 * proportional to area.  The contract (mesh_sample.hip, restated in numpy by
 * tests/mesh_sample_restatement.py), all in fp64, one operation at a time:
 *   weights   len_f = sqrt((cx*cx + cy*cy) + cz*cz) of c = ab × ac for a usable triangle with a finite
 *             len_f, else 0; L = max len_f = m·2^e, m in [0.5, 1); w_f = (uint64) trunc(ldexp(len_f,
 *             32 − e)); cum_f = w_0 + … + w_f, W = cum_{F−1}.  A triangle more than about 2^32 times
 *             smaller than the largest has weight 0 and is never drawn.  Built by the first call,
 *             cached on the mesh, dropped with it.
 *   sample k  base = sample_base(seed, k), x_j = splitmix64(base + j); t = high 64 bits of x_0·W; the
 *             triangle is the smallest f with cum_f > t; u = (x_1 >> 11)·2^-53, v = (x_2 >> 11)·2^-53,
 *             both replaced by 1 − themselves when u + v > 1; point = (a + ab*u) + ac*v per
 *             coordinate; normal = c / len.
 * Outputs [device], each may be NULL: points_out n×3 f64, triangle_out n int32, uv_out n×2 f64 (m3d_mesh_closest's
 * convention: point ≈ (1−u−v)·a + u·b + v·c), normals_out n×3 f64 (the triangle's unit face
 * normal).  A sample's bits depend on (mesh, seed, k) alone.  n == 0 launches nothing.
 * M3D_ERR_INVALID: a mesh without a usable triangle, or none with a finite non-zero weight;
 * n < 0 or n >= 2^31.  Synchronous. */
int m3d_mesh_sample(m3d_ctx* ctx, m3d_mesh* mesh, int64_t n, uint64_t seed, double* points_out,
                    int32_t* triangle_out, double* uv_out, double* normals_out, void* stream);
/* out2 [host]: W and the number of triangles with a non-zero weight (0 0 before the first
 * m3d_mesh_sample of the mesh). */
int m3d_mesh_sample_info(const m3d_mesh* mesh, uint64_t* out2);

/* ------------------------------------------------------------------ minimum-distance thinning (thin.hip)
 * (added within ABI 13)  The points of a cloud kept by dart throwing in a hashed order: key_i =
 * sample_base(seed, i), points ranked by (key_i, i); point i is kept iff no kept point j of lower
 * rank has d²(i, j) < radius·radius, d² = ((dx·dx + dy·dy) + dz·dz) in fp64 on the original
 * coordinates, strictly.  The kept points are original points, no two closer than radius, and every
 * dropped point has a kept one strictly inside radius.  A point with a coordinate that is not
 * finite is never kept and blocks nobody.  The result is unique (restated in numpy by
 * tests/mesh_sample_restatement.py).
 * decided_out [device] n int32: +k kept in round k, −k dropped in round k (k >= 1; never 0 on
 * success).  *kept_count_out, *rounds_out [host], each may be NULL: the points kept and the rounds
 * (launches) the call took — deterministic as well.  An empty cloud: nothing is touched, 0 and 0.
 * M3D_ERR_INVALID: radius <= 0 or not finite.  M3D_ERR_HIP with a message: more than 256 rounds.
 * Synchronous. */
int m3d_thin_min_distance(m3d_ctx* ctx, const m3d_cloud* cloud, double radius, uint64_t seed, int32_t* decided_out,
                          int64_t* kept_count_out, int32_t* rounds_out, void* stream);

/* ------------------------------------------------------------------ ICP against a mesh (mesh_icp.hip)
 * registration_icp with the SURFACE of a triangle mesh as target (added within ABI 13, the version
 * number is unchanged): m3d_icp_run's loop — the transformed copy of the source, `init` applied
 * unless isIdentity(), fitness / inlier_rmse, the convergence rule, the LDLT solve, the slot layout
 * and the fixed summation order are its — with, for every point p of an evaluation,
 *   the winner     m3d_mesh_closest's: the smallest (d², triangle index) over every usable
 *                  triangle, q its closest point;
 *   the match      d² < max_dist·max_dist in fp64, strictly (a NaN point never matches);
 *   the row        n = the winning triangle's unit face normal (b − a) × (c − a) / |·|,
 *                  r = (p − q) · n, J = [p × n | n], weighted by `kernel` as m3d_robust_terms' rows
 *                  (NULL or kind L2: weight 1).
 * Restated in numpy by tests/mesh_icp_restatement.py.  path: 0 automatic, 1 brute force, 2 the
 * triangle grid (one box of half-width max_dist per point: a triangle outside it is farther than
 * max_dist by m3d_mesh_closest's covering argument, so no radius ladder is needed).  Both paths,
 * the seeded box on or off, and repeated calls return the same bits.  Not implemented: point-to-point
 * estimation, Generalized and Colored ICP against a mesh, sharding over devices, a step-wise driver.
 * M3D_ERR_INVALID: max_dist <= 0 or not finite, an unknown kernel kind, a k <= 0 or non-finite
 * for a kind that reads k, a mesh without a usable triangle, an unknown path.  An empty source is
 * not an error: fitness 0, T = init, no pairs.  Both calls are synchronous.
 *
 * m3d_mesh_icp_terms: ONE evaluation at T_host [host] 16 f64 (NULL = identity; applied unless
 * isIdentity()) → sums_out [host] 32 f64 in m3d_robust_terms' layout (0..20 JtJ upper triangle,
 * 21..26 Jtr, 27 sum r², 28 count, 29 sum d²).  seed_tri [device] ns int32 or NULL: per source point
 * (caller's order) a triangle to try first — the grid path then cuts the point's box with that
 * triangle's distance when it is below max_dist (−1, or an unusable triangle: no seed); it never
 * changes a bit of the result.  tri_idx [device] ns int32 or NULL: the matched triangle per source
 * point in the caller's order (−1 none); d2_out [device] ns f64 or NULL: its d² (+inf none). */
int m3d_mesh_icp_terms(m3d_ctx* ctx, m3d_mesh* mesh, const m3d_cloud* src, const double* T_host, double max_dist,
                       const m3d_robust_kernel* kernel, int32_t path, const int32_t* seed_tri, double* sums_out,
                       int32_t* tri_idx, double* d2_out, void* stream);
/* The whole registration from init [host] 16 f64 (NULL = identity).  params->estimation must be
 * M3D_EST_POINT_TO_PLANE (else M3D_ERR_INVALID); params->nn_method and flags are not read.  seed:
 * non-zero = from the second evaluation on every point's box is cut with the distance of the
 * triangle it matched last.  tri_idx as above, of the last evaluation. */
int m3d_mesh_icp_run(m3d_ctx* ctx, m3d_mesh* mesh, const m3d_cloud* src, const double* init, double max_dist,
                     const m3d_icp_params* params, const m3d_robust_kernel* kernel, int32_t path, int32_t seed,
                     m3d_icp_result* out, int32_t* tri_idx, void* stream);

/* ------------------------------------------------------------------ test hooks
 * Host-compiled copy of the device 3×3 linear algebra (same source), for CPU-side unit tests
 * of the math.  Never used by the product path. */
int m3d_debug_kabsch3_host(const double* src9, const double* tgt9, double* T16);
int m3d_debug_ldlt6_host(const double* A36, const double* b6, double* x6);  // the device solve's
                                                                       // rule: unpivoted, pivoted fallback
/* linalg.h rotation_from_cov, compiled for the host: H9 row-major (H = Σ p qᵀ, p source, q target)
 * → R9 row-major, the proper rotation mapping source to target; returns the rank it used (2 for
 * rank ≥ 2, 1, 0 for H = 0, −1 for a non-finite H: then R = I; −1 for a null pointer too) */
int m3d_debug_rotation_from_cov_host(const double* H9, double* R9);
/* linalg.h sym3_eigenvalues, compiled for the host: sym6 = (a00, a01, a02, a11, a12, a22) → lam3 ascending */
int m3d_debug_sym3_eigenvalues_host(const double* sym6, double* lam3);
/* linalg.h sym3_eigen, compiled for the host: lam3 as above, V9 row-major, column k a unit eigenvector of lam3[k] */
int m3d_debug_sym3_eigen_host(const double* sym6, double* lam3, double* V9);
/* XXH64 of [p, p + len) (the chunk hash of m3d_content_keys; known-answer tests). */
uint64_t m3d_debug_xxh64(const void* p, size_t len, uint64_t seed);
/* XXH3-128 (default secret, seed 0) of [p, p + len), len >= 241 (the long-input path the content
 * keys use; known-answer tests against the xxhash package): out2 = (low, high). */
int m3d_debug_xxh3_128(const void* p, size_t len, uint64_t* out2);
/* Failure injection for the multi-GPU failure tests: what = 1 fails this rank's next local run of
 * m3d_ransac_run_sharded, 2 its next ICP shard-loop iteration (0 clears). */
int m3d_debug_comm_inject(m3d_comm* c, int what);
/* The FPFH swap test's correctly rounded acos (ddmath.h acos_cr, host-compiled copy of the device
 * code): out[k] = acos(u[k]) rounded to nearest, for the CPU test against mpmath.  ABI 13. */
int m3d_debug_acos_cr(const double* u, int64_t n, double* out);
/* The same on the device: out[k] [device] = acos_cr(u[k]) (mode 0) or the device libm's acos
 * (mode 1) for u [device] n f64.  ABI 13. */
int m3d_debug_acos_device(m3d_ctx* ctx, const double* u, int64_t n, double* out, int mode, void* stream);
/* Fill every idle block of the block cache on the current device with `byte` (synchronous); a
 * later object that reuses one starts from those bytes.  Returns the blocks filled (>= 0).  ABI 13. */
int m3d_debug_block_cache_fill(int byte);
/* Overwrite the count of a grid loop's deferral list (synchronous on stream): a count past the
 * list makes the next scan drop its writes and m3d_icp_result_get fail with M3D_ERR_HIP until the
 * next m3d_icp_reset.  M3D_ERR_INVALID when the loop defers nothing.  ABI 13. */
int m3d_debug_icp_defer_count(m3d_icp* s, uint32_t count, void* stream);
/* The brute-force NN's slice plan, the rule on the host: counts [host] n tile
 * counts, one per query block of 512 sources -> out [host] `budget` entries x | y << 16 | S << 24
 * (slice y of the S slices of query block x; 0xFFFFFFFF = empty), S = clamp(ceil(t / tau), 1,
 * min(smax, ntiles)) for the smallest tau with sum S <= budget.  Returns tau (>= 1), or
 * M3D_ERR_INVALID (n < 1, n > budget).  Added within ABI 13, the version number is unchanged. */
int m3d_debug_nn_plan_host(const uint32_t* counts, int64_t n, int64_t budget, int64_t smax, int64_t ntiles,
                           uint32_t* out);
/* Force S[x] [host, n = the loop's query blocks] slices per query block for the following
 * evaluations of a brute-force loop, until the next m3d_icp_reset (synchronous on stream); the
 * loop's own planner leaves a forced plan alone.  M3D_ERR_INVALID for S < 1, S > the target's
 * tiles, sum S > the resident block slots, or a loop whose launch takes no plan.  Within ABI 13. */
int m3d_debug_icp_nn_plan(m3d_icp* s, const int32_t* S, int64_t n, void* stream);
/* Read a loop's plan back (synchronous): shape3 [host] = {query blocks (0: no plan), budget, flag
 * (0 none, 1 planned, 2 forced)}; counts [host, query blocks] the tile counts the planner last
 * read, table [host, budget] the entries; either may be NULL.  Within ABI 13. */
int m3d_debug_icp_nn_plan_read(m3d_icp* s, uint32_t* counts, uint32_t* table, int32_t* shape3, void* stream);
/* The seed records of a brute-force loop (synchronous): seed [host, ns x 4 f32] the
 * records in the loop's slot order (x, y, z, index bits; index -1: none), corr [host, ns i32] the
 * loop's correspondences in the same order, tgt32 [host, nt x 4 f32] the target's centred fp32
 * points on the device, whose row corr[i] record i must equal bit for bit; any of the three may be
 * NULL.  info2 [host] = {1 when the next m3d_icp_step will seed its scan from the records (the last
 * fused tail wrote them), else 0; the loop state's mfma_ok (0: the scans of the current transform
 * take the plain fallback)}.  M3D_ERR_INVALID for a loop without records (grid NN, empty target).
 * Within ABI 13. */
int m3d_debug_icp_seed_read(m3d_icp* s, float* seed, int32_t* corr, float* tgt32, int32_t* info2, void* stream);
/* The iteration whose terms pass runs inside the brute-force NN launch: on = 0
 * turns it off for this loop, anything else back on; the loop's captured step graphs are dropped.
 * Returns 1 when m3d_icp_step of this loop now runs that iteration, 0 when it runs the two
 * launches it ran before (the switch off, or a loop the iteration does not apply to).
 * m3d_debug_icp_nn_terms_read (synchronous): tickets / counts [host, query blocks; either may be
 * NULL] = the query blocks' hand-off tickets and tile counts as they are on the device; returns
 * the number of query blocks (0: the loop has neither).
 * m3d_debug_nn_terms_select (host only): the selection rule itself on nine conditions, bit 0 the
 * NN launch is the planned one, 1 the tail is the fused one, 2 it hands the keys back, 3
 * point-to-plane, 4 target records, 5 seed records, 6 a claim, 7 one device, 8 switched on;
 * returns 1 when the iteration is selected.  Within ABI 13. */
int m3d_debug_icp_nn_terms(m3d_icp* s, int on);
int m3d_debug_icp_nn_terms_read(m3d_icp* s, uint32_t* tickets, uint32_t* counts, void* stream);
int m3d_debug_nn_terms_select(uint32_t bits);

/* ------------------------------------------------------------------ host text I/O (§8(f) rank 4) */

/* ASCII number blocks of PLY files (m3d.plyio; replaces the C++ readers/writers the reference
 * calls: o3d.io.read_point_cloud, src/ply/ply.py:80, and trimesh's ASCII PLY export,
 * convert_stl-ply.py:1-11).  Host only, no device needed.
 * m3d_parse_ascii_rows: `rows` non-blank lines of exactly `cols` numbers from buf[0, len) →
 * out [host] rows×cols f64 (correctly rounded, as numpy's parser); *consumed = bytes used.
 * M3D_ERR_INVALID on anything else (short file, extra or non-numeric tokens).
 * m3d_format_ascii_rows: rows×cols f64 → text, one row per line, each number the shortest
 * representation that reads back to the same double; cap ≥ 32·rows·cols. */
int m3d_parse_ascii_rows(const char* buf, size_t len, int64_t rows, int32_t cols, double* out,
                         size_t* consumed);
int m3d_format_ascii_rows(const double* data, int64_t rows, int32_t cols, char* out, size_t cap,
                          size_t* written);
/* STL corner merge (convert_stl-ply.py:3-6, trimesh.load_mesh): xyz [host] n×3 f64 corners →
 * uniq [host] (≤ n)×3 f64 unique vertices in first-occurrence order (exact equality, -0.0 ≡ +0.0),
 * inverse [host] n int32 (corner → vertex id), *n_unique. */
int m3d_merge_vertices(const double* xyz, int64_t n, double* uniq, int32_t* inverse,
                       int64_t* n_unique);
/* Content keys of the drop-in's cache (m3d.cache): keys [host] 2·n uint64 (low, high), the
 * 128-bit key of each buffer [host] bufs[i], lens[i] bytes — its 64 KB chunks hashed with
 * XXH3-128 by a persistent host thread pool (a tail under 241 bytes joins the previous chunk),
 * then XXH3-128 of (chunk digests ‖ length ‖ chunk count) (ABI 10; ABI ≤ 9 chained 64-bit XXH64
 * chunk digests).  Non-cryptographic: unrelated contents collide with probability ≈ 2⁻¹²⁸.  The
 * same bytes give the same key whatever the thread count. */
int m3d_content_keys(const void* const* bufs, const size_t* lens, int32_t n, uint64_t* keys);

#ifdef __cplusplus
}
#endif
#endif /* M3D_H_ */
