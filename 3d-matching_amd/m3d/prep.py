"""Device preprocessing and feature matching (prep.hip / feat.hip through the C ABI).

Open3D 0.19 calls of the reference path and their replacements (semantics restated in
oracle/prep_oracle.py; parity against Open3D itself unpinned — SURVEY.md §8(c)):

| reference (file:line)                                   | here                              |
|---------------------------------------------------------|-----------------------------------|
| ``pcd.voxel_down_sample(v)`` (src/ply/ply.py:106)        | ``voxel_down_sample``             |
| ``estimate_normals(Hybrid(2v, 30))`` (ply.py:110,133)    | ``estimate_normals``              |
| ``compute_fpfh_feature(pcd, Hybrid(5v, 100))`` (:117)    | ``compute_fpfh`` (N×33)           |
| ``correspondences_from_features`` (ransac.py:85)         | ``feature_correspondences``       |
| ``RegistrationRANSACBasedOnCorrespondence`` (a6)         | ``ransac_on_correspondences``     |
| ``KDTreeFlann.search_knn_vector_3d`` (not in the path)   | ``knn_search`` (every point)      |
| ``pcd.remove_statistical_outlier(nb, ratio)`` (users)    | ``remove_statistical_outlier``    |
| ``pcd.remove_radius_outlier(nb, r)`` (users)             | ``remove_radius_outlier``         |
| ``pcd.segment_plane(thr, ransac_n, iterations)`` (users) | ``segment_plane``, ``plane_score`` |
| ``pcd.cluster_dbscan(eps, min_points)`` (users)          | ``cluster_dbscan``                |
| ``keypoint.compute_iss_keypoints(pcd, ...)`` (users)     | ``compute_iss_keypoints``, ``model_resolution`` |
| ``registration_fgr_based_on_correspondence`` (users)     | ``fgr_on_correspondences``, ``fgr_tuple_test``, ``fgr_terms`` |
| (none: a minimum point distance, keeping original points) | ``thin_min_distance``             |

All entry points take host or device arrays and return numpy arrays (the reference works in
numpy / Open3D host containers); the arithmetic runs on the GPU.
"""

from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib
from .core import Cloud, _torch, context, corr_pairs, device_empty, ptr, stream_handle, to_device


def voxel_down_sample(points, voxel_size: float, normals=None):
    """→ (points M×3, normals M×3 or None), voxels in ascending (ix, iy, iz) order."""
    torch = _torch()
    ctx = context()
    p = to_device(points)
    nrm = None if normals is None else to_device(normals)
    n = p.shape[0]
    out = device_empty((max(n, 1), 3), torch.float64)
    out_n = device_empty((max(n, 1), 3), torch.float64) if nrm is not None else None
    m = C.c_int64()
    ctx.check(ctx.lib.m3d_voxel_down_sample(ctx.h, ptr(p), ptr(nrm), n, float(voxel_size), ptr(out),
                                            ptr(out_n), C.byref(m), stream_handle()), "voxel_down_sample")
    k = m.value
    return out[:k].cpu().numpy(), (None if out_n is None else out_n[:k].cpu().numpy())


def _cloud(points, normals=None):
    return points if isinstance(points, Cloud) else Cloud(points, normals)


def hybrid_search(points, radius: float, max_nn: int):
    """KDTreeFlann::SearchHybrid for every point → (idx N×k int32 (−1 pad), d2 N×k, count N)."""
    torch = _torch()
    c = _cloud(points)
    ctx = c.ctx
    n = max(c.n, 1)
    idx = device_empty((n, max_nn), torch.int32)
    d2 = device_empty((n, max_nn), torch.float64)
    cnt = device_empty((n,), torch.int32)
    ctx.check(ctx.lib.m3d_hybrid_search(ctx.h, c.h, float(radius), int(max_nn), ptr(idx), ptr(d2),
                                        ptr(cnt), stream_handle()), "hybrid_search")
    return idx[: c.n].cpu().numpy(), d2[: c.n].cpu().numpy(), cnt[: c.n].cpu().numpy()


def _empty(points) -> bool:
    return (points.n if isinstance(points, Cloud) else len(points)) == 0


def knn_search(points, k: int):
    """KDTreeFlann::SearchKNN(p_i, k) for every point, the point itself included: the min(k, N)
    smallest (d², index) pairs over the whole cloud → (idx N×k int32 (−1 pad), d2 N×k (inf pad),
    count N)."""
    if not 1 <= int(k) <= 256:
        raise ValueError("knn_search: 1 <= k <= 256")
    torch = _torch()
    c = _cloud(points)
    ctx = c.ctx
    n = max(c.n, 1)
    idx = device_empty((n, k), torch.int32)
    d2 = device_empty((n, k), torch.float64)
    cnt = device_empty((n,), torch.int32)
    ctx.check(ctx.lib.m3d_knn_search(ctx.h, c.h, int(k), ptr(idx), ptr(d2), ptr(cnt), stream_handle()),
              "knn_search")
    return idx[: c.n].cpu().numpy(), d2[: c.n].cpu().numpy(), cnt[: c.n].cpu().numpy()


@dataclass
class OutlierStats:
    """What RemoveStatisticalOutliers derives from the mean neighbour distances."""
    kept: int
    valid: int
    mean: float
    std_dev: float
    threshold: float
    mean_distance: np.ndarray | None = None  # per point, with ``with_mean_distance=True``


def remove_statistical_outlier(points, nb_neighbors: int, std_ratio: float, with_mean_distance: bool = False):
    """PointCloud::RemoveStatisticalOutliers → (kept indices int32 ascending, OutlierStats)."""
    if int(nb_neighbors) < 1 or not float(std_ratio) > 0.0:
        raise ValueError("Illegal input parameters, the number of neighbors and standard deviation ratio "
                         "must be positive.")
    if int(nb_neighbors) > 256:
        raise ValueError("remove_statistical_outlier: nb_neighbors <= 256")
    if _empty(points):  # an empty cloud gives an empty result, no device involved
        return np.zeros(0, np.int32), OutlierStats(0, 0, 0.0, 0.0, 0.0,
                                                   np.zeros(0) if with_mean_distance else None)
    torch = _torch()
    c = _cloud(points)
    ctx = c.ctx
    n = max(c.n, 1)
    ind = device_empty((n,), torch.int32)
    avg = device_empty((n,), torch.float64) if with_mean_distance else None
    m = C.c_int64()
    st = _lib.OutlierStats()
    ctx.check(ctx.lib.m3d_remove_statistical_outlier(ctx.h, c.h, int(nb_neighbors), float(std_ratio), ptr(ind),
                                                     C.byref(m), C.byref(st), ptr(avg), stream_handle()),
              "remove_statistical_outlier")
    return ind[: m.value].cpu().numpy(), OutlierStats(int(st.kept), int(st.valid), float(st.mean),
                                                      float(st.std_dev), float(st.threshold),
                                                      None if avg is None else avg[: c.n].cpu().numpy())


def remove_radius_outlier(points, nb_points: int, radius: float, with_counts: bool = False):
    """PointCloud::RemoveRadiusOutliers → kept indices int32 ascending (a point is kept iff more
    than ``nb_points`` points, itself included, lie strictly within ``radius``);
    ``with_counts=True`` → (indices, every point's full count)."""
    if int(nb_points) < 1 or not float(radius) > 0.0:
        raise ValueError("Illegal input parameters, the number of points and radius must be positive.")
    if _empty(points):
        return (np.zeros(0, np.int32), np.zeros(0, np.int32)) if with_counts else np.zeros(0, np.int32)
    torch = _torch()
    c = _cloud(points)
    ctx = c.ctx
    n = max(c.n, 1)
    ind = device_empty((n,), torch.int32)
    cnt = device_empty((n,), torch.int32) if with_counts else None
    m = C.c_int64()
    ctx.check(ctx.lib.m3d_remove_radius_outlier(ctx.h, c.h, int(nb_points), float(radius), ptr(ind), C.byref(m),
                                                ptr(cnt), stream_handle()), "remove_radius_outlier")
    kept = ind[: m.value].cpu().numpy()
    return (kept, cnt[: c.n].cpu().numpy()) if with_counts else kept


PLANE_CHUNK = _lib.PLANE_CHUNK  # points per chunk of the plane score kernel's partial sums


@dataclass
class PlaneOutcome:
    """What ``segment_plane`` found besides the refitted plane and the inliers."""
    ransac_plane: np.ndarray  # the best hypothesis's own plane: the inliers are tested against it
    best_index: int           # its hypothesis number (−1: none)
    best_count: int
    best_rmse: float
    evaluated: int            # non-degenerate hypotheses evaluated
    iterations: int           # the hypothesis number at which the loop left
    counts: np.ndarray        # per hypothesis, −1 = degenerate or not reached
    err: np.ndarray           # Σ dist² over its inliers (−1 on the same rows)


def _check_plane_args(distance_threshold, ransac_n, num_iterations, probability):
    if not (0.0 < float(probability) <= 1.0):
        raise ValueError("Probability must be > 0 and <= 1.0")
    if int(ransac_n) < 3:
        raise ValueError("ransac_n should be set to higher than or equal to 3.")
    if int(ransac_n) > 32:
        raise ValueError("segment_plane: ransac_n <= 32")
    if int(num_iterations) < 0:
        raise ValueError("segment_plane: num_iterations >= 0")
    if not (np.isfinite(float(distance_threshold)) and float(distance_threshold) >= 0.0):
        raise ValueError("segment_plane: distance_threshold must be finite and >= 0")


def segment_plane(points, distance_threshold: float = 0.01, ransac_n: int = 3, num_iterations: int = 100,
                  probability: float = 0.99999999, *, seed: int = 0, samples=None, batch: int = 0,
                  with_details: bool = False):
    """PointCloud::SegmentPlane on the device (m3d_segment_plane; the contract is in include/m3d.h)
    → (plane_model (4,) float64, inliers int64 ascending); ``with_details=True`` adds a
    ``PlaneOutcome``.  ``samples`` (num_iterations × ransac_n indices) replaces the native counter
    sampler (``seed``); ``batch`` (hypotheses per device batch, 0 = automatic) changes no result."""
    _check_plane_args(distance_threshold, ransac_n, num_iterations, probability)
    n_pts = points.n if isinstance(points, Cloud) else len(points)
    if n_pts < int(ransac_n):
        raise ValueError("There must be at least 'ransac_n' points.")
    smp = None
    if samples is not None:
        smp = np.ascontiguousarray(np.asarray(samples, np.int64).reshape(-1, int(ransac_n)))
        if smp.shape[0] != int(num_iterations):
            raise ValueError("segment_plane: samples must be num_iterations × ransac_n")
        if smp.size and (smp.min() < -(1 << 31) or smp.max() >= (1 << 31)):
            raise ValueError("segment_plane: a sample index is outside [0, n)")
    torch = _torch()
    c = _cloud(points)
    ctx = c.ctx
    H = int(num_iterations)
    p = _lib.PlaneParams(float(distance_threshold), float(probability), int(seed) & ((1 << 64) - 1),
                         int(ransac_n), H, int(batch), 0)
    r = _lib.PlaneResult()
    smp_dev = None if smp is None else to_device(smp.astype(np.int32), dtype="int32", shape_tail=(int(ransac_n),))
    inl = device_empty((max(c.n, 1),), torch.int32)
    cnt = device_empty((max(H, 1),), torch.int32) if with_details else None
    err = device_empty((max(H, 1),), torch.float64) if with_details else None
    ctx.check(ctx.lib.m3d_segment_plane(ctx.h, c.h, C.byref(p), ptr(smp_dev), C.byref(r), ptr(inl), ptr(cnt),
                                        ptr(err), stream_handle()), "segment_plane")
    plane = np.array(r.plane[:], np.float64)
    inliers = inl[: int(r.num_inliers)].cpu().numpy().astype(np.int64)
    if not with_details:
        return plane, inliers
    return plane, inliers, PlaneOutcome(np.array(r.ransac_plane[:], np.float64), int(r.best_index),
                                        int(r.best_count), float(r.best_rmse), int(r.evaluated),
                                        int(r.iterations), cnt[:H].cpu().numpy(), err[:H].cpu().numpy())


def plane_score(points, planes, distance_threshold: float):
    """For each of the H planes (H×4: a, b, c, d) the number of points with
    |((a·x + b·y) + c·z) + d| < distance_threshold and the sum of their squared distances
    (m3d_plane_score) → (counts int32 H, err float64 H); an empty cloud gives zeros."""
    torch = _torch()
    c = _cloud(points)
    ctx = c.ctx
    pl = to_device(np.asarray(planes, np.float64).reshape(-1, 4), shape_tail=(4,))
    H = pl.shape[0]
    cnt = torch.zeros((max(H, 1),), dtype=torch.int32, device=pl.device)
    err = torch.zeros((max(H, 1),), dtype=torch.float64, device=pl.device)
    ctx.check(ctx.lib.m3d_plane_score(ctx.h, c.h, ptr(pl), H, float(distance_threshold), ptr(cnt), ptr(err),
                                      stream_handle()), "plane_score")
    return cnt[:H].cpu().numpy(), err[:H].cpu().numpy()


@dataclass
class DbscanOutcome:
    """What ``cluster_dbscan`` found besides the labels."""
    num_clusters: int
    num_core: int
    num_noise: int
    largest_label: int   # the biggest cluster, the lowest label on ties; −1 without a cluster
    largest_size: int
    sizes: np.ndarray    # int32 (num_clusters,): members per label
    counts: np.ndarray   # int32 (n,): every point's full neighbour count, itself included


def cluster_dbscan(points, eps: float, min_points: int, *, with_details: bool = False):
    """PointCloud::ClusterDBSCAN on the device (m3d_cluster_dbscan; the contract is in include/m3d.h)
    → labels int32 (n,), −1 = noise; ``with_details=True`` → (labels, ``DbscanOutcome``)."""
    if not (np.isfinite(float(eps)) and float(eps) > 0.0):
        raise ValueError("cluster_dbscan: eps must be finite and > 0")
    if int(min_points) < 1:
        raise ValueError("cluster_dbscan: min_points >= 1")
    if _empty(points):  # an empty cloud gives an empty result, no device involved
        labels = np.zeros(0, np.int32)
        return (labels, DbscanOutcome(0, 0, 0, -1, 0, np.zeros(0, np.int32), np.zeros(0, np.int32))) \
            if with_details else labels
    torch = _torch()
    c = _cloud(points)
    ctx = c.ctx
    lab = device_empty((c.n,), torch.int32)
    sizes = device_empty((c.n,), torch.int32) if with_details else None
    cnt = device_empty((c.n,), torch.int32) if with_details else None
    r = _lib.DbscanResult()
    ctx.check(ctx.lib.m3d_cluster_dbscan(ctx.h, c.h, float(eps), int(min_points), ptr(lab), C.byref(r), ptr(sizes),
                                         ptr(cnt), stream_handle()), "cluster_dbscan")
    labels = lab.cpu().numpy()
    if not with_details:
        return labels
    return labels, DbscanOutcome(int(r.num_clusters), int(r.num_core), int(r.num_noise), int(r.largest_label),
                                 int(r.largest_size), sizes[: int(r.num_clusters)].cpu().numpy(), cnt.cpu().numpy())


@dataclass
class ThinOutcome:
    """What ``thin_min_distance`` found besides the kept indices."""
    decided: np.ndarray  # (n,) int32: +k kept in round k, −k dropped in round k
    rounds: int          # launches of the device loop
    kept: int


def thin_min_distance(points, radius: float, seed: int = 0, with_details: bool = False):
    """Thin a cloud to a minimum point distance on the device (m3d_thin_min_distance; the contract
    is in include/m3d.h): dart throwing in the order of the hashed keys ``sample_base(seed, i)`` —
    a point is kept unless a kept point of lower rank lies strictly inside ``radius``.  The kept
    points are original points (a voxel mean is not), no two closer than ``radius``, and every
    dropped point has a kept one inside it.  → ascending int64 indices of the kept points;
    ``with_details=True`` → (indices, ``ThinOutcome``).  A host point with a coordinate that is
    not finite is never kept and blocks nobody; a ``Cloud`` must be finite."""
    if not (np.isfinite(float(radius)) and float(radius) > 0.0):
        raise ValueError("thin_min_distance: radius must be finite and > 0")
    if _empty(points):
        idx = np.zeros(0, np.int64)
        return (idx, ThinOutcome(np.zeros(0, np.int32), 0, 0)) if with_details else idx
    torch = _torch()
    if not isinstance(points, Cloud) and not isinstance(points, torch.Tensor):
        p = np.asarray(points, np.float64).reshape(-1, 3)
        ok = np.isfinite(p).all(axis=1)
        if not ok.all():
            finite = np.flatnonzero(ok)
            if len(finite) == 0:
                idx = np.zeros(0, np.int64)
                return (idx, ThinOutcome(np.full(len(p), -1, np.int32), 1, 0)) if with_details else idx
            return _thin_subset(p, finite, radius, seed, with_details)
        points = p
    c = _cloud(points)
    ctx = c.ctx
    dec = device_empty((c.n,), torch.int32)
    kept, rounds = C.c_int64(0), C.c_int32(0)
    ctx.check(ctx.lib.m3d_thin_min_distance(ctx.h, c.h, float(radius), int(seed) & 0xFFFFFFFFFFFFFFFF, ptr(dec),
                                            C.byref(kept), C.byref(rounds), stream_handle()), "thin_min_distance")
    decided = dec.cpu().numpy()
    idx = np.flatnonzero(decided > 0).astype(np.int64)
    return (idx, ThinOutcome(decided, int(rounds.value), int(kept.value))) if with_details else idx


def _thin_subset(p: np.ndarray, finite: np.ndarray, radius: float, seed: int, with_details: bool):
    """``thin_min_distance`` of a host cloud with rows that are not finite.  A device cloud's frame
    (its mean) does not survive such a row, and the ranks are those of the ORIGINAL indices, so the
    rows cannot simply be left out: they are parked together at one point more than two radii
    outside the finite rows' box — where they meet only each other — and reported as dropped in
    round 1 whatever happened to them there.  (``rounds`` counts the parked rows' rounds too: two.)"""
    q = p.copy()
    bad = np.setdiff1d(np.arange(len(p)), finite)
    far = float(np.abs(p[finite]).max()) + 2.5 * float(radius)
    q[bad] = [far, far, far]
    _, out = thin_min_distance(q, radius, seed, with_details=True)
    decided = out.decided.copy()
    decided[bad] = -1
    idx = np.flatnonzero(decided > 0).astype(np.int64)
    return (idx, ThinOutcome(decided, out.rounds, len(idx))) if with_details else idx


def model_resolution(points) -> float:
    """Open3D ``ComputeModelResolution`` on the device (m3d_model_resolution): the mean distance to
    the nearest other point; 0.0 for an empty cloud or a single point."""
    if not isinstance(points, Cloud):
        shape = tuple(points.shape) if hasattr(points, "shape") else np.shape(points)
        if len(shape) != 2 or shape[1] != 3:
            raise ValueError("model_resolution: points must be (n, 3)")
    if _empty(points):
        return 0.0
    c = _cloud(points)
    ctx = c.ctx
    res = C.c_double(0.0)
    ctx.check(ctx.lib.m3d_model_resolution(ctx.h, c.h, C.byref(res), stream_handle()), "model_resolution")
    return float(res.value)


@dataclass
class IssOutcome:
    """What ``compute_iss_keypoints`` found besides the keypoint indices."""
    num_keypoints: int
    num_salient: int       # points with third_eigen_values > 0: the candidates of the non-maximum pass
    num_counted: int       # points with count >= min_neighbors
    salient_radius: float  # as used
    non_max_radius: float
    resolution: float      # 0.0 when both radii were given
    third_eigen_values: np.ndarray  # float64 (n,): the smallest eigenvalue of a salient point, else 0
    counts: np.ndarray     # int32 (n,): points strictly within salient_radius, the point itself included


def compute_iss_keypoints(points, salient_radius: float = 0.0, non_max_radius: float = 0.0, gamma_21: float = 0.975,
                          gamma_32: float = 0.975, min_neighbors: int = 5, *, with_details: bool = False):
    """keypoint::ComputeISSKeypoints on the device (m3d_compute_iss_keypoints; the contract is in
    include/m3d.h) → keypoint indices int64, ascending; ``with_details=True`` → (indices, ``IssOutcome``)."""
    rs, rn, g21, g32 = float(salient_radius), float(non_max_radius), float(gamma_21), float(gamma_32)
    if not (np.isfinite(rs) and rs >= 0.0 and np.isfinite(rn) and rn >= 0.0):
        raise ValueError("compute_iss_keypoints: the radii must be finite and >= 0")
    if not (np.isfinite(g21) and np.isfinite(g32)):
        raise ValueError("compute_iss_keypoints: the gammas must be finite")
    if int(min_neighbors) < 0:
        raise ValueError("compute_iss_keypoints: min_neighbors >= 0")
    if _empty(points):  # an empty cloud gives an empty result, no device involved
        idx = np.zeros(0, np.int64)
        return (idx, IssOutcome(0, 0, 0, rs, rn, 0.0, np.zeros(0), np.zeros(0, np.int32))) if with_details else idx
    torch = _torch()
    c = _cloud(points)
    ctx = c.ctx
    ind = device_empty((c.n,), torch.int32)
    third = device_empty((c.n,), torch.float64) if with_details else None
    cnt = device_empty((c.n,), torch.int32) if with_details else None
    p = _lib.IssParams(rs, rn, g21, g32, int(min_neighbors))
    r = _lib.IssResult()
    ctx.check(ctx.lib.m3d_compute_iss_keypoints(ctx.h, c.h, C.byref(p), C.byref(r), ptr(ind), ptr(third), ptr(cnt),
                                                stream_handle()), "compute_iss_keypoints")
    idx = ind[: int(r.num_keypoints)].cpu().numpy().astype(np.int64)
    if not with_details:
        return idx
    return idx, IssOutcome(int(r.num_keypoints), int(r.num_salient), int(r.num_counted), float(r.salient_radius),
                           float(r.non_max_radius), float(r.resolution), third.cpu().numpy(), cnt.cpu().numpy())


def estimate_normals(points, radius: float, max_nn: int = 30, normals=None):
    """PointCloud::EstimateNormals(KDTreeSearchParamHybrid(radius, max_nn)); existing
    ``normals`` orient the result like Open3D."""
    torch = _torch()
    c = _cloud(points, normals)
    ctx = c.ctx
    out = device_empty((max(c.n, 1), 3), torch.float64)
    ctx.check(ctx.lib.m3d_estimate_normals(ctx.h, c.h, float(radius), int(max_nn), ptr(out),
                                           stream_handle()), "estimate_normals")
    return out[: c.n].cpu().numpy()


def estimate_normals_knn(points, knn: int = 20, normals=None):
    """PointCloud::EstimateNormals(KDTreeSearchParamKNN(knn)) (m3d_estimate_normals_knn): the
    covariance of each point's exact ``knn`` nearest points, itself included → N×3; fewer than
    three neighbours give (0, 0, 1); existing ``normals`` orient the result like Open3D."""
    if not 1 <= int(knn) <= 256:
        raise ValueError("estimate_normals_knn: 1 <= knn <= 256")
    torch = _torch()
    c = _cloud(points, normals)
    ctx = c.ctx
    out = device_empty((max(c.n, 1), 3), torch.float64)
    ctx.check(ctx.lib.m3d_estimate_normals_knn(ctx.h, c.h, int(knn), ptr(out), stream_handle()),
              "estimate_normals_knn")
    return out[: c.n].cpu().numpy()


def covariances_from_normals(normals, epsilon: float = 1e-3):
    """Generalized ICP's per-point covariances (InitializePointCloudForGeneralizedICP):
    C = Rx·diag(ε, 1, 1)·Rxᵀ with Rx the rotation of e1 onto the normal → N×3×3, exactly
    symmetric (m3d_covariances_from_normals)."""
    if not float(epsilon) > 0.0:
        raise ValueError("epsilon must be > 0")
    torch = _torch()
    ctx = context()
    nrm = to_device(normals)
    n = nrm.shape[0]
    out = device_empty((max(n, 1), 9), torch.float64)
    ctx.check(ctx.lib.m3d_covariances_from_normals(ctx.h, ptr(nrm), n, float(epsilon), ptr(out),
                                                   stream_handle()), "covariances_from_normals")
    return out[:n].cpu().numpy().reshape(n, 3, 3)


def compute_fpfh(points, normals, radius: float, max_nn: int = 100):
    """ComputeFPFHFeature → N×33 (Open3D's Feature.data is the 33×N transpose)."""
    torch = _torch()
    c = _cloud(points)
    ctx = c.ctx
    nrm = to_device(normals)
    if nrm.shape != (c.n, 3):
        raise ValueError("normals must be N×3")
    out = device_empty((max(c.n, 1), 33), torch.float64)
    ctx.check(ctx.lib.m3d_compute_fpfh(ctx.h, c.h, ptr(nrm), float(radius), int(max_nn), ptr(out),
                                       stream_handle()), "compute_fpfh")
    return out[: c.n].cpu().numpy()


def _feature_rows(f):
    """N×33 feature rows from an Open3D-style Feature (``.data`` is 33×N) or an array."""
    if not isinstance(f, np.ndarray) and hasattr(f, "data"):
        return np.ascontiguousarray(np.asarray(f.data, np.float64).T)
    return f


def feature_correspondences(f_src, f_tgt, mutual_filter: bool = False,
                            mutual_consistent_ratio: float = 0.1) -> np.ndarray:
    """CorrespondencesFromFeatures (ransac.py:85) on N×33 feature rows, or on Open3D-style
    Features (33×N ``.data``) → (M, 2) int32 (source, target)."""
    torch = _torch()
    ctx = context()
    f_src, f_tgt = _feature_rows(f_src), _feature_rows(f_tgt)
    fs = to_device(f_src, shape_tail=None)
    ft = to_device(f_tgt, shape_tail=None)
    if fs.ndim != 2 or ft.ndim != 2 or fs.shape[1] != ft.shape[1]:
        raise ValueError("features must be N×33 arrays")
    ns, nt = fs.shape[0], ft.shape[0]
    out = device_empty((max(ns, 1), 2), torch.int32)
    m = C.c_int64()
    ctx.check(ctx.lib.m3d_feature_correspondences(ctx.h, ptr(fs), ns, ptr(ft), nt, fs.shape[1],
                                                  int(bool(mutual_filter)), float(mutual_consistent_ratio),
                                                  ptr(out), C.byref(m), stream_handle()),
              "feature_correspondences")
    return out[: m.value].cpu().numpy()


@dataclass
class FeatureRansacOutcome:
    transformation: np.ndarray
    fitness: float
    inlier_rmse: float
    best_index: int
    validations: int
    correspondence_set: np.ndarray
    corres_ratio: float = 0.0  # the best's correspondence inlier ratio (Open3D's exit input)


def ransac_on_correspondences(src, tgt, corres, max_correspondence_distance: float, *,
                              ransac_n: int = 3, edge_length: float | None = 0.9,
                              distance: float | None = None, max_iteration: int = 100000,
                              confidence: float = 0.999, seed: int = 0) -> FeatureRansacOutcome:
    """RegistrationRANSACBasedOnCorrespondence (PointToPoint, no scaling) with the EdgeLength /
    Distance checkers (None disables a checker)."""
    torch = _torch()
    sc, tc = _cloud(src), _cloud(tgt)
    ctx = sc.ctx
    corr = to_device(np.asarray(corres).reshape(-1, 2), dtype="int32", shape_tail=(2,))
    p = _lib.FeatureRansacParams(float(max_correspondence_distance), float(confidence),
                                 float(edge_length) if edge_length is not None else 0.0,
                                 float(distance) if distance is not None else 0.0,
                                 int(seed) & ((1 << 64) - 1), int(max_iteration), int(ransac_n))
    r = _lib.FeatureRansacResult()
    cs = device_empty((max(sc.n, 1),), torch.int32)
    ctx.check(ctx.lib.m3d_ransac_on_correspondences(ctx.h, sc.h, tc.h, ptr(corr), corr.shape[0], C.byref(p),
                                                    C.byref(r), ptr(cs), stream_handle()),
              "ransac_on_correspondences")
    return FeatureRansacOutcome(np.array(r.T[:]).reshape(4, 4), r.fitness, r.inlier_rmse,
                                int(r.best_index), int(r.validations), corr_pairs(ctx, cs, sc.n),
                                float(r.corres_ratio))


FGR_TRIAL_BATCH = _lib.FGR_TRIAL_BATCH  # trials per batch of the tuple test
FGR_ONE_WG_ROWS = _lib.FGR_ONE_WG_ROWS  # rows the one-workgroup loop holds


@dataclass
class FgrOutcome:
    transformation: np.ndarray   # source → target, original scale
    fitness: float
    inlier_rmse: float
    correspondence_set: np.ndarray
    rows: np.ndarray             # (n_rows, 2) the row set the loop optimised over
    n_input: int
    tuples: int                  # accepted trials kept by the tuple test (0 without it)
    trials: int                  # trials the sequential tuple loop ran
    par_final: float
    scale_global: float
    mean_src: np.ndarray
    mean_tgt: np.ndarray
    T_norm: np.ndarray           # the loop's T: normalised target → normalised source


def _check_fgr_option(o):
    if not (0.0 < float(o.tuple_scale) <= 1.0):
        raise ValueError("fgr: tuple_scale must be in (0, 1]")
    if not float(o.division_factor) > 0.0:
        raise ValueError("fgr: division_factor must be > 0")
    if int(o.iteration_number) < 0 or int(o.maximum_tuple_count) < 0:
        raise ValueError("fgr: iteration_number and maximum_tuple_count must be >= 0")
    if not np.isfinite(float(o.maximum_correspondence_distance)):
        raise ValueError("fgr: maximum_correspondence_distance must be finite")


def _fgr_params(option, path: int = 0):
    from .types import FastGlobalRegistrationOption

    o = option if option is not None else FastGlobalRegistrationOption()
    _check_fgr_option(o)
    if path not in (0, 1, 2):
        raise ValueError("fgr: path is 0, 1 or 2")
    seed = 0 if o.seed is None else int(o.seed)
    return _lib.FgrParams(float(o.division_factor), float(o.maximum_correspondence_distance), float(o.tuple_scale),
                          seed & ((1 << 64) - 1), int(o.iteration_number), int(o.maximum_tuple_count),
                          int(bool(o.use_absolute_scale)), int(bool(o.decrease_mu)), int(bool(o.tuple_test)), int(path))


def _fgr_rows(corres, ns: int, nt: int):
    c = np.asarray(corres)
    c = np.zeros((0, 2), np.int64) if c.size == 0 else c.reshape(-1, 2).astype(np.int64)
    if len(c) and (c.min() < 0 or c[:, 0].max() >= ns or c[:, 1].max() >= nt):
        raise ValueError("fgr: a correspondence index is outside its cloud")
    return c.astype(np.int32)


def _fgr_rows_room(p, nc: int) -> int:
    cap = min(max(int(p.maximum_tuple_count), 1), max(100 * nc, 1))
    return max(3 * cap if p.tuple_test else nc, 1)


def fgr_on_correspondences(src_points, tgt_points, corres, option=None, with_details: bool = False, *, path: int = 0):
    """Fast Global Registration over given (source, target) rows on the device
    (m3d_fgr_on_correspondences; the contract is in include/m3d.h) → ``FgrOutcome``
    (``with_details``: with the row set; otherwise ``rows`` is empty).  ``path`` forces the loop's
    launch shape (1 one workgroup, 2 one launch per iteration) and changes no bit of the result."""
    p = _fgr_params(option, path)
    torch = _torch()
    sc, tc = _cloud(src_points), _cloud(tgt_points)
    ctx = sc.ctx
    rows = _fgr_rows(corres, sc.n, tc.n)
    nc = len(rows)
    corr = to_device(rows, dtype="int32", shape_tail=(2,)) if nc else None
    r = _lib.FgrResult()
    rows_out = device_empty((_fgr_rows_room(p, nc), 2), torch.int32) if with_details else None
    cs = device_empty((max(sc.n, 1),), torch.int32)
    ctx.check(ctx.lib.m3d_fgr_on_correspondences(ctx.h, sc.h, tc.h, ptr(corr), nc, C.byref(p), C.byref(r),
                                                 ptr(rows_out), ptr(cs), stream_handle()), "fgr_on_correspondences")
    have = sc.n > 0 and tc.n > 0
    kept = rows_out[: int(r.n_rows)].cpu().numpy() if with_details and have else np.zeros((0, 2), np.int32)
    return FgrOutcome(np.array(r.T[:]).reshape(4, 4), r.fitness, r.inlier_rmse, corr_pairs(ctx, cs, sc.n), kept,
                      int(r.n_input), int(r.tuples), int(r.trials), float(r.par_final), float(r.scale_global),
                      np.array(r.mean_src[:]), np.array(r.mean_tgt[:]), np.array(r.T_norm[:]).reshape(4, 4))


def fgr_tuple_test(src_points, tgt_points, corres, option=None):
    """Normalisation and tuple test alone (m3d_fgr_tuple_test) → (rows (n_rows, 2) int32, trials)."""
    p = _fgr_params(option)
    torch = _torch()
    sc, tc = _cloud(src_points), _cloud(tgt_points)
    ctx = sc.ctx
    rows = _fgr_rows(corres, sc.n, tc.n)
    nc = len(rows)
    corr = to_device(rows, dtype="int32", shape_tail=(2,)) if nc else None
    out = device_empty((_fgr_rows_room(p, nc), 2), torch.int32)
    n_rows, trials = C.c_int64(), C.c_int64()
    ctx.check(ctx.lib.m3d_fgr_tuple_test(ctx.h, sc.h, tc.h, ptr(corr), nc, C.byref(p), ptr(out), C.byref(n_rows),
                                         C.byref(trials), stream_handle()), "fgr_tuple_test")
    return out[: n_rows.value].cpu().numpy(), int(trials.value)


def fgr_terms(p_rows, q_rows, par: float) -> np.ndarray:
    """One iteration's sums over given rows (m3d_fgr_terms): the 21 upper-triangle entries of JᵀJ
    and the 6 of Jᵀr, (27,) float64."""
    ctx = context()
    p, q = to_device(p_rows), to_device(q_rows)
    if p.shape != q.shape:
        raise ValueError("fgr_terms: p and q must have the same shape")
    out = (C.c_double * 27)()
    ctx.check(ctx.lib.m3d_fgr_terms(ctx.h, ptr(p), ptr(q), p.shape[0], float(par), out, stream_handle()), "fgr_terms")
    return np.array(out[:], np.float64)
