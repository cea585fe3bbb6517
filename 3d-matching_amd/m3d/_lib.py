"""ctypes binding of libm3d.so (include/m3d.h).

The library is built in-tree (``make -C 3d-matching_amd/csrc`` or ``__graft_entry__.build()``)
and loaded from this directory.  There is no fallback: if the shared object or a gfx950 device
is missing, the product path raises.
"""

from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

LIB_PATH = Path(__file__).resolve().parent / "libm3d.so"

M3D_OK = 0
M3D_ERR_INVALID = -1
M3D_ERR_HIP = -2
M3D_ERR_OOM = -3
M3D_ERR_NODEVICE = -4
M3D_ERR_COMM = -5

HYP_OK, HYP_DEGENERATE, HYP_NONFINITE = 0, 1, 2
SCORE_SQUARED, SCORE_NORM = 0, 1
EST_POINT_TO_POINT, EST_POINT_TO_PLANE = 0, 1
KERNEL_NN, KERNEL_SCORE, KERNEL_KABSCH, KERNEL_TERMS, KERNEL_LOOP, KERNEL_COMM = 0, 1, 2, 3, 4, 5
ICP_NO_SPLIT = 2
NN_BRUTE, NN_GRID = 0, 1
EVAL_INFORMATION = 1
ROBUST_L2, ROBUST_L1, ROBUST_HUBER, ROBUST_CAUCHY, ROBUST_GM, ROBUST_TUKEY = 0, 1, 2, 3, 4, 5  # M3D_KERNEL_L2 ..
COMM_ID_BYTES = 128
DT_I32, DT_I64, DT_F64 = 0, 1, 2
OP_SUM, OP_MIN, OP_MAX = 0, 1, 2
NN_METHODS = {"brute": NN_BRUTE, "grid": NN_GRID}
ABI_VERSION = 13
PLANE_CHUNK = 512  # plane.hip kPlaneChunk (m3d_plane_chunk): points per chunk of the score kernel's partial sums
FGR_TRIAL_BATCH = 16384  # fgr.hip kFgrTrialBatch (m3d_fgr_trial_batch): trials per batch of the tuple test
FGR_ONE_WG_ROWS = 3072   # fgr.hip kFgrOneWgRows (m3d_fgr_one_wg_rows): rows the one-workgroup loop holds
MESH_AUTO, MESH_BRUTE, MESH_GRID = 0, 1, 2  # m3d_mesh_closest path
MESH_BRUTE_TILE = 256  # mesh.hip kMeshBruteTile (m3d_mesh_brute_tile): triangles per LDS tile of the brute kernel

vp = C.c_void_p
i64 = C.c_int64
u64 = C.c_uint64
i32 = C.c_int32
dbl = C.c_double


class RansacParams(C.Structure):
    _fields_ = [("max_iter", i64), ("seed", u64), ("thr", dbl), ("mode", i32),
                ("early_stop", i32), ("es_threshold", dbl), ("es_confidence", dbl),
                ("batch", i64), ("hyp0", i64)]


class RansacResult(C.Structure):
    _fields_ = [("T", dbl * 16), ("fitness", dbl), ("best_index", i64), ("iterations", i64),
                ("best_count", i64), ("rechecked", i64)]


class IcpParams(C.Structure):
    _fields_ = [("relative_fitness", dbl), ("relative_rmse", dbl), ("max_iteration", i32),
                ("estimation", i32), ("nn_method", i32), ("flags", i32)]


class FeatureRansacParams(C.Structure):
    _fields_ = [("max_correspondence_distance", dbl), ("confidence", dbl), ("edge_length", dbl),
                ("distance", dbl), ("seed", u64), ("max_iteration", i32), ("ransac_n", i32)]


class FeatureRansacResult(C.Structure):
    _fields_ = [("T", dbl * 16), ("fitness", dbl), ("inlier_rmse", dbl), ("best_index", i64),
                ("validations", i64), ("corres_ratio", dbl)]


class IcpResult(C.Structure):
    _fields_ = [("T", dbl * 16), ("fitness", dbl), ("inlier_rmse", dbl),
                ("num_correspondences", i64), ("iterations", i32), ("converged", i32),
                ("update", dbl * 16)]


class EvalResult(C.Structure):
    _fields_ = [("fitness", dbl), ("inlier_rmse", dbl), ("num_correspondences", i64),
                ("information", dbl * 36)]


class GicpParams(C.Structure):
    _fields_ = [("relative_fitness", dbl), ("relative_rmse", dbl), ("max_iteration", i32),
                ("nn_method", i32), ("epsilon", dbl)]


class RobustKernel(C.Structure):
    _fields_ = [("kind", i32), ("k", dbl)]


class ColoredParams(C.Structure):
    _fields_ = [("lambda_geometric", dbl), ("relative_fitness", dbl), ("relative_rmse", dbl),
                ("max_iteration", i32), ("nn_method", i32)]


class OutlierStats(C.Structure):
    _fields_ = [("kept", i64), ("valid", i64), ("mean", dbl), ("std_dev", dbl), ("threshold", dbl)]


class PlaneParams(C.Structure):
    _fields_ = [("distance_threshold", dbl), ("probability", dbl), ("seed", u64), ("ransac_n", i32),
                ("num_iterations", i32), ("batch", i32), ("reserved", i32)]


class PlaneResult(C.Structure):
    _fields_ = [("plane", dbl * 4), ("ransac_plane", dbl * 4), ("num_inliers", i64), ("best_index", i64),
                ("best_count", i64), ("evaluated", i64), ("iterations", i64), ("best_rmse", dbl)]


class FgrParams(C.Structure):
    _fields_ = [("division_factor", dbl), ("maximum_correspondence_distance", dbl), ("tuple_scale", dbl),
                ("seed", u64), ("iteration_number", i32), ("maximum_tuple_count", i32),
                ("use_absolute_scale", i32), ("decrease_mu", i32), ("tuple_test", i32), ("path", i32)]


class FgrResult(C.Structure):
    _fields_ = [("T", dbl * 16), ("fitness", dbl), ("inlier_rmse", dbl), ("n_input", i64), ("n_rows", i64),
                ("tuples", i64), ("trials", i64), ("par_final", dbl), ("scale_global", dbl),
                ("mean_src", dbl * 3), ("mean_tgt", dbl * 3), ("T_norm", dbl * 16)]


class DbscanResult(C.Structure):
    _fields_ = [("num_clusters", i64), ("num_core", i64), ("num_noise", i64), ("largest_label", i64),
                ("largest_size", i64)]


class IssParams(C.Structure):
    _fields_ = [("salient_radius", dbl), ("non_max_radius", dbl), ("gamma_21", dbl), ("gamma_32", dbl),
                ("min_neighbors", i32)]


class IssResult(C.Structure):
    _fields_ = [("num_keypoints", i64), ("num_salient", i64), ("num_counted", i64), ("salient_radius", dbl),
                ("non_max_radius", dbl), ("resolution", dbl)]


# name -> (restype, argtypes)
SIGNATURES = {
    "m3d_abi_version": (C.c_int, []),
    "m3d_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "m3d_create": (C.c_int, [C.c_int, C.POINTER(vp)]),
    "m3d_destroy": (None, [vp]),
    "m3d_last_error": (C.c_char_p, [vp]),
    "m3d_get_stats": (C.c_int, [vp, C.POINTER(i64)]),
    "m3d_trim_block_cache": (C.c_int, [vp, C.POINTER(i64)]),
    "m3d_profile_enable": (C.c_int, [vp, C.c_int]),
    "m3d_profile_read": (C.c_int, [vp, C.c_int, C.POINTER(dbl), C.POINTER(i64)]),
    "m3d_corrset_create": (C.c_int, [vp, vp, i64, vp, i64, vp, i64, vp, C.POINTER(vp)]),
    "m3d_corrset_create_gathered": (C.c_int, [vp, vp, vp, i64, vp, C.POINTER(vp)]),
    "m3d_corrset_destroy": (None, [vp]),
    "m3d_corrset_size": (i64, [vp]),
    "m3d_kabsch3_batch": (C.c_int, [vp, vp, vp, u64, i64, i64, vp, vp, vp]),
    "m3d_ransac_score": (C.c_int, [vp, vp, vp, i64, dbl, C.c_int, vp, vp]),
    "m3d_kabsch3_one": (C.c_int, [vp, vp, C.POINTER(i32), C.POINTER(dbl), C.POINTER(i32), vp]),
    "m3d_ransac_score_one": (C.c_int, [vp, vp, C.POINTER(dbl), dbl, C.c_int, C.POINTER(i64), vp]),
    "m3d_ransac_run": (C.c_int, [vp, vp, C.POINTER(RansacParams), vp, C.POINTER(RansacResult), vp]),
    "m3d_ransac_run_async": (C.c_int, [vp, vp, C.POINTER(RansacParams), vp, vp, vp, vp]),
    "m3d_replay_triples": (C.c_int, [C.POINTER(C.c_uint32), C.POINTER(i32), i64, i64,
                                     C.POINTER(i32)]),
    "m3d_cloud_create": (C.c_int, [vp, vp, vp, i64, vp, C.POINTER(vp)]),
    "m3d_cloud_create_framed": (C.c_int, [vp, vp, vp, i64, C.POINTER(C.c_double), vp, C.POINTER(vp)]),
    "m3d_cloud_create_host": (C.c_int, [vp, vp, vp, i64, C.POINTER(C.c_double), vp, C.POINTER(vp)]),
    "m3d_cloud_destroy": (None, [vp]),
    "m3d_cloud_size": (i64, [vp]),
    "m3d_nn1": (C.c_int, [vp, vp, vp, C.POINTER(dbl), dbl, i32, vp, vp, vp]),
    "m3d_evaluate_registration": (C.c_int, [vp, vp, vp, C.POINTER(dbl), dbl, i32, i32,
                                            C.POINTER(EvalResult), vp, vp, vp]),
    "m3d_covariances_from_normals": (C.c_int, [vp, vp, i64, dbl, vp, vp]),
    "m3d_gicp_terms": (C.c_int, [vp, vp, vp, vp, vp, C.POINTER(dbl), dbl, i32, dbl, C.POINTER(dbl), vp, vp]),
    "m3d_gicp_run": (C.c_int, [vp, vp, vp, vp, vp, C.POINTER(dbl), dbl, C.POINTER(GicpParams),
                               C.POINTER(IcpResult), vp, vp]),
    "m3d_robust_terms": (C.c_int, [vp, vp, vp, C.POINTER(dbl), dbl, i32, C.POINTER(RobustKernel), C.POINTER(dbl),
                                   vp, vp]),
    "m3d_robust_icp_run": (C.c_int, [vp, vp, vp, C.POINTER(dbl), dbl, C.POINTER(IcpParams),
                                     C.POINTER(RobustKernel), C.POINTER(IcpResult), vp, vp]),
    "m3d_gicp_terms_robust": (C.c_int, [vp, vp, vp, vp, vp, C.POINTER(dbl), dbl, i32, dbl, C.POINTER(RobustKernel),
                                        C.POINTER(dbl), vp, vp]),
    "m3d_gicp_run_robust": (C.c_int, [vp, vp, vp, vp, vp, C.POINTER(dbl), dbl, C.POINTER(GicpParams),
                                      C.POINTER(RobustKernel), C.POINTER(IcpResult), vp, vp]),
    "m3d_color_gradients": (C.c_int, [vp, vp, vp, dbl, i32, vp, vp]),
    "m3d_colored_terms": (C.c_int, [vp, vp, vp, vp, vp, vp, C.POINTER(dbl), dbl, i32, dbl, C.POINTER(RobustKernel),
                                    C.POINTER(dbl), vp, vp]),
    "m3d_colored_icp_run": (C.c_int, [vp, vp, vp, vp, vp, vp, C.POINTER(dbl), dbl, C.POINTER(ColoredParams),
                                      C.POINTER(RobustKernel), C.POINTER(IcpResult), vp, vp]),
    "m3d_icp_run": (C.c_int, [vp, vp, vp, C.POINTER(dbl), dbl, C.POINTER(IcpParams),
                              C.POINTER(IcpResult), vp, vp]),
    "m3d_icp_create": (C.c_int, [vp, vp, vp, dbl, C.POINTER(IcpParams), C.POINTER(vp)]),
    "m3d_icp_destroy": (None, [vp]),
    "m3d_icp_reset": (C.c_int, [vp, C.POINTER(dbl), vp]),
    "m3d_icp_step": (C.c_int, [vp, vp]),
    "m3d_icp_steps": (C.c_int, [vp, C.c_int32, vp]),
    "m3d_icp_prepare_steps": (C.c_int, [vp, C.c_int32]),
    "m3d_icp_shard_nn": (C.c_int, [vp, i64, vp, vp]),
    "m3d_icp_shard_nn_range": (C.c_int, [vp, i64, i64, i64, vp, vp]),
    "m3d_icp_shard_claim": (C.c_int, [vp, vp, vp, vp]),
    "m3d_icp_shard_terms": (C.c_int, [vp, i64, vp, vp, vp, vp]),
    "m3d_icp_solve": (C.c_int, [vp, vp, vp]),
    "m3d_icp_result_get": (C.c_int, [vp, C.POINTER(IcpResult), vp]),
    "m3d_icp_set_source_total": (C.c_int, [vp, i64]),
    "m3d_icp_corr": (vp, [vp]),
    "m3d_icp_copy_corr": (C.c_int, [vp, vp, vp]),
    "m3d_corr_pairs": (C.c_int, [vp, vp, i64, vp, C.POINTER(i64), vp]),
    "m3d_icp_copy_slots": (C.c_int, [vp, vp, vp]),
    "m3d_icp_copy_points": (C.c_int, [vp, vp, vp]),
    "m3d_voxel_down_sample": (C.c_int, [vp, vp, vp, i64, dbl, vp, vp, C.POINTER(i64), vp]),
    "m3d_hybrid_search": (C.c_int, [vp, vp, dbl, i32, vp, vp, vp, vp]),
    "m3d_estimate_normals": (C.c_int, [vp, vp, dbl, i32, vp, vp]),
    "m3d_compute_fpfh": (C.c_int, [vp, vp, vp, dbl, i32, vp, vp]),
    "m3d_knn_search": (C.c_int, [vp, vp, i32, vp, vp, vp, vp]),
    "m3d_estimate_normals_knn": (C.c_int, [vp, vp, i32, vp, vp]),
    "m3d_remove_statistical_outlier": (C.c_int, [vp, vp, i32, dbl, vp, C.POINTER(i64),
                                                 C.POINTER(OutlierStats), vp, vp]),
    "m3d_remove_radius_outlier": (C.c_int, [vp, vp, i32, dbl, vp, C.POINTER(i64), vp, vp]),
    "m3d_segment_plane": (C.c_int, [vp, vp, C.POINTER(PlaneParams), vp, C.POINTER(PlaneResult), vp, vp, vp, vp]),
    "m3d_plane_score": (C.c_int, [vp, vp, vp, i64, dbl, vp, vp, vp]),
    "m3d_plane_chunk": (i32, []),
    "m3d_cluster_dbscan": (C.c_int, [vp, vp, dbl, i32, vp, C.POINTER(DbscanResult), vp, vp, vp]),
    "m3d_model_resolution": (C.c_int, [vp, vp, C.POINTER(dbl), vp]),
    "m3d_compute_iss_keypoints": (C.c_int, [vp, vp, C.POINTER(IssParams), C.POINTER(IssResult), vp, vp, vp, vp]),
    "m3d_feature_correspondences": (C.c_int, [vp, vp, i64, vp, i64, i32, i32, dbl, vp,
                                              C.POINTER(i64), vp]),
    "m3d_ransac_on_correspondences": (C.c_int, [vp, vp, vp, vp, i64, C.POINTER(FeatureRansacParams),
                                                C.POINTER(FeatureRansacResult), vp, vp]),
    "m3d_fgr_on_correspondences": (C.c_int, [vp, vp, vp, vp, i64, C.POINTER(FgrParams), C.POINTER(FgrResult),
                                             vp, vp, vp]),
    "m3d_fgr_tuple_test": (C.c_int, [vp, vp, vp, vp, i64, C.POINTER(FgrParams), vp, C.POINTER(i64),
                                     C.POINTER(i64), vp]),
    "m3d_fgr_terms": (C.c_int, [vp, vp, vp, i64, dbl, C.POINTER(dbl), vp]),
    "m3d_fgr_trial_batch": (i32, []),
    "m3d_fgr_one_wg_rows": (i32, []),
    "m3d_mesh_create": (C.c_int, [vp, vp, i64, vp, i64, C.POINTER(vp)]),
    "m3d_mesh_destroy": (None, [vp]),
    "m3d_mesh_size": (i64, [vp]),
    "m3d_mesh_closest": (C.c_int, [vp, vp, vp, i64, C.POINTER(dbl), i32, dbl, vp, vp, vp, vp, vp, vp]),
    "m3d_mesh_icp_terms": (C.c_int, [vp, vp, vp, C.POINTER(dbl), dbl, C.POINTER(RobustKernel), i32, vp,
                                     C.POINTER(dbl), vp, vp, vp]),
    "m3d_mesh_icp_run": (C.c_int, [vp, vp, vp, C.POINTER(dbl), dbl, C.POINTER(IcpParams), C.POINTER(RobustKernel),
                                   i32, i32, C.POINTER(IcpResult), vp, vp]),
    "m3d_mesh_grid_info": (C.c_int, [vp, C.POINTER(i64)]),
    "m3d_mesh_sample": (C.c_int, [vp, vp, i64, u64, vp, vp, vp, vp, vp]),
    "m3d_mesh_sample_info": (C.c_int, [vp, C.POINTER(u64)]),
    "m3d_thin_min_distance": (C.c_int, [vp, vp, dbl, u64, vp, C.POINTER(i64), C.POINTER(i32), vp]),
    "m3d_mesh_brute_tile": (i32, []),
    "m3d_mesh_auto_brute_max": (i32, []),
    "m3d_mesh_cast_rays": (C.c_int, [vp, vp, vp, i64, dbl, dbl, i32, vp, vp, vp, vp]),
    "m3d_mesh_count_rays": (C.c_int, [vp, vp, vp, i64, dbl, dbl, i32, vp, vp]),
    "m3d_mesh_ray_info": (C.c_int, [vp, C.POINTER(i64)]),
    "m3d_mesh_ray_auto_brute_max": (i32, []),
    "m3d_comm_unique_id": (C.c_int, [C.POINTER(C.c_uint8)]),
    "m3d_comm_init": (C.c_int, [vp, C.POINTER(C.c_uint8), C.c_int, C.c_int, C.POINTER(vp)]),
    "m3d_comm_destroy": (None, [vp]),
    "m3d_comm_allreduce": (C.c_int, [vp, vp, i64, C.c_int, C.c_int, vp]),
    "m3d_icp_shard_steps": (C.c_int, [vp, vp, i64, i32, vp]),
    "m3d_icp_source_shard_steps": (C.c_int, [vp, vp, i32, vp]),
    "m3d_ransac_best_allreduce": (C.c_int, [vp, vp, i64, vp, vp]),
    "m3d_ransac_run_sharded": (C.c_int, [vp, vp, vp, C.POINTER(RansacParams), C.POINTER(RansacResult), vp]),
    "m3d_comm_poisoned": (C.c_int, [vp]),
    "m3d_debug_comm_inject": (C.c_int, [vp, C.c_int]),
    "m3d_debug_acos_cr": (C.c_int, [vp, C.c_int64, vp]),
    "m3d_debug_acos_device": (C.c_int, [vp, vp, C.c_int64, vp, C.c_int, vp]),
    "m3d_debug_block_cache_fill": (C.c_int, [C.c_int]),
    "m3d_debug_icp_defer_count": (C.c_int, [vp, C.c_uint32, vp]),
    "m3d_debug_nn_plan_host": (C.c_int, [vp, C.c_int64, C.c_int64, C.c_int64, C.c_int64, vp]),
    "m3d_debug_icp_nn_plan": (C.c_int, [vp, vp, C.c_int64, vp]),
    "m3d_debug_icp_nn_plan_read": (C.c_int, [vp, vp, vp, vp, vp]),
    "m3d_debug_icp_seed_read": (C.c_int, [vp, vp, vp, vp, vp, vp]),
    "m3d_debug_icp_nn_terms": (C.c_int, [vp, C.c_int]),
    "m3d_debug_icp_nn_terms_read": (C.c_int, [vp, vp, vp, vp]),
    "m3d_debug_nn_terms_select": (C.c_int, [C.c_uint32]),
    "m3d_parse_ascii_rows": (C.c_int, [C.c_char_p, C.c_size_t, i64, i32, C.POINTER(dbl),
                                       C.POINTER(C.c_size_t)]),
    "m3d_format_ascii_rows": (C.c_int, [C.POINTER(dbl), i64, i32, vp, C.c_size_t, C.POINTER(C.c_size_t)]),
    "m3d_merge_vertices": (C.c_int, [C.POINTER(dbl), i64, C.POINTER(dbl), C.POINTER(i32), C.POINTER(i64)]),
    "m3d_content_keys": (C.c_int, [C.POINTER(vp), C.POINTER(C.c_size_t), i32, C.POINTER(u64)]),
    "m3d_debug_xxh64": (u64, [vp, C.c_size_t, u64]),
    "m3d_debug_xxh3_128": (C.c_int, [vp, C.c_size_t, C.POINTER(u64)]),
    "m3d_debug_kabsch3_host":(C.c_int, [C.POINTER(dbl), C.POINTER(dbl), C.POINTER(dbl)]),
    "m3d_debug_ldlt6_host": (C.c_int, [C.POINTER(dbl), C.POINTER(dbl), C.POINTER(dbl)]),
    "m3d_debug_rotation_from_cov_host": (C.c_int, [C.POINTER(dbl), C.POINTER(dbl)]),
    "m3d_debug_sym3_eigenvalues_host": (C.c_int, [C.POINTER(dbl), C.POINTER(dbl)]),
    "m3d_debug_sym3_eigen_host": (C.c_int, [C.POINTER(dbl), C.POINTER(dbl), C.POINTER(dbl)]),
}

_lib = None


class M3DError(RuntimeError):
    pass


class M3DCommError(M3DError):
    """A peer rank failed, or the communicator was aborted after a failure (M3D_ERR_COMM)."""


def load() -> C.CDLL:
    """Load libm3d.so (once).  Raises ImportError if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise ImportError(f"{LIB_PATH} not built: run `make -C {LIB_PATH.parent.parent / 'csrc'}` "
                          "(hipcc --offload-arch=gfx950)")
    # torch first: PyTorch-ROCm ships its own HIP/HSA runtime libraries.  Imported first, they
    # are the copies libm3d.so binds to (same sonames) and the process has ONE runtime; loaded
    # after libm3d.so (e.g. plyio's host text helpers before any device call), torch brings up a
    # second runtime and libm3d's then reports no device (measured on the MI355X box).
    try:
        import torch  # noqa: F401
    except ImportError:  # pragma: no cover - host-only use without torch
        pass
    lib = C.CDLL(os.fspath(LIB_PATH))
    lib.m3d_abi_version.restype = C.c_int
    if lib.m3d_abi_version() != ABI_VERSION:
        raise ImportError(f"{LIB_PATH}: ABI {lib.m3d_abi_version()} != {ABI_VERSION}; rebuild it")
    for name, (res, args) in SIGNATURES.items():
        f = getattr(lib, name, None)
        if f is None and name.startswith("m3d_debug_") and os.environ.get("AB_LIB"):
            continue  # A/B runs (AB_LIB: another build of this ABI) may lack a later diagnostic entry
        if f is None:
            raise ImportError(f"{LIB_PATH}: no symbol {name}; rebuild it")
        f.restype = res
        f.argtypes = args
    _lib = lib
    return lib


def check(rc: int, ctx=None, what: str = "") -> None:
    if rc == M3D_OK:
        return
    msg = ""
    if ctx is not None:
        raw = load().m3d_last_error(ctx)
        msg = raw.decode() if raw else ""
    if rc == M3D_ERR_INVALID:
        raise ValueError(f"{what}: {msg}" if msg else what)
    if rc == M3D_ERR_COMM:
        raise M3DCommError(f"{what} failed (code {rc}): {msg}")
    raise M3DError(f"{what} failed (code {rc}): {msg}")
