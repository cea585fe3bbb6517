"""Host-side result/data types mirroring the reference's Open3D-facing types.

* ``RegistrationResult`` — Open3D ``pipelines.registration.RegistrationResult`` as the reference
  uses it (`ransac.py:134-136`, `icp.py:42`): ``transformation`` (4×4 f64), ``fitness``,
  ``inlier_rmse``, ``correspondence_set`` (M×2 int32).
* ``FastGlobalRegistrationOption`` — Open3D ``pipelines.registration.FastGlobalRegistrationOption``:
  the same names and defaults.
* ``PointCloud`` — the two attributes the path reads from ``o3d.geometry.PointCloud``:
  ``points`` (N×3 f64) and ``normals`` (N×3 f64 or empty), ``covariances`` (N×3×3 f64 or
  empty) for Generalized ICP and ``colors`` (N×3 f64 in [0, 1] or empty) for Colored ICP.
"""

from __future__ import annotations

import numpy as np


class RegistrationResult:
    def __init__(self, transformation=None, fitness=0.0, inlier_rmse=0.0, correspondence_set=None):
        self.transformation = np.eye(4) if transformation is None else np.asarray(transformation, np.float64)
        self.fitness = float(fitness)
        self.inlier_rmse = float(inlier_rmse)
        self.correspondence_set = (np.zeros((0, 2), np.int32) if correspondence_set is None
                                   else np.asarray(correspondence_set, np.int32).reshape(-1, 2))

    def __repr__(self):
        return (f"RegistrationResult with fitness={self.fitness:e}, inlier_rmse={self.inlier_rmse:e}, "
                f"and correspondence_set size of {len(self.correspondence_set)}")


class FastGlobalRegistrationOption:
    """Open3D ``FastGlobalRegistrationOption`` (0.19): names and defaults as upstream.  ``seed``
    keys the counter sampler of the tuple test (``None``: 0)."""

    def __init__(self, division_factor: float = 1.4, use_absolute_scale: bool = False, decrease_mu: bool = False,
                 maximum_correspondence_distance: float = 0.025, iteration_number: int = 64,
                 tuple_scale: float = 0.95, maximum_tuple_count: int = 1000, tuple_test: bool = True, seed=None):
        self.division_factor = float(division_factor)
        self.use_absolute_scale = bool(use_absolute_scale)
        self.decrease_mu = bool(decrease_mu)
        self.maximum_correspondence_distance = float(maximum_correspondence_distance)
        self.iteration_number = int(iteration_number)
        self.tuple_scale = float(tuple_scale)
        self.maximum_tuple_count = int(maximum_tuple_count)
        self.tuple_test = bool(tuple_test)
        self.seed = seed

    def __repr__(self):
        return ("FastGlobalRegistrationOption(" + ", ".join(f"{k}={v!r}" for k, v in vars(self).items()) + ")")


class Feature:
    """Open3D ``pipelines.registration.Feature``: ``data`` is dimension × N (33×N for FPFH)."""

    def __init__(self, data=None):
        self.data = np.zeros((33, 0)) if data is None else np.asarray(data, np.float64)

    def dimension(self) -> int:
        return self.data.shape[0]

    def num(self) -> int:
        return self.data.shape[1]


class PointCloud:
    def __init__(self, points=None, normals=None, covariances=None, colors=None):
        self.points = np.zeros((0, 3)) if points is None else np.asarray(points, np.float64).reshape(-1, 3)
        self.normals = np.zeros((0, 3)) if normals is None else np.asarray(normals, np.float64).reshape(-1, 3)
        # per-point 3×3 covariances (Open3D ``PointCloud.covariances``, Generalized ICP), or none
        self.covariances = (np.zeros((0, 3, 3)) if covariances is None
                            else np.asarray(covariances, np.float64).reshape(-1, 3, 3))
        # per-point RGB in [0, 1] (Open3D ``PointCloud.colors``, Colored ICP), or none
        self.colors = np.zeros((0, 3)) if colors is None else np.asarray(colors, np.float64).reshape(-1, 3)

    def has_points(self) -> bool:
        return len(self.points) > 0

    def has_normals(self) -> bool:
        return len(self.normals) == len(self.points) and len(self.points) > 0

    def has_covariances(self) -> bool:
        return len(self.covariances) == len(self.points) and len(self.points) > 0

    def has_colors(self) -> bool:
        return len(self.colors) == len(self.points) and len(self.points) > 0

    def compute_point_cloud_distance(self, target) -> np.ndarray:
        """Open3D ``PointCloud.compute_point_cloud_distance``: for each point the distance to its
        nearest point of ``target``, on the device (matcher.evaluate)."""
        from matcher.evaluate import compute_point_cloud_distance

        return compute_point_cloud_distance(self, target)

    def select_by_index(self, indices, invert: bool = False) -> "PointCloud":
        """Open3D ``PointCloud.select_by_index``: the points (and normals, covariances, colours) at
        ``indices`` in index order; ``invert`` selects every other point."""
        n = len(self.points)
        mask = np.zeros(n, bool)
        mask[np.asarray(indices, np.int64).reshape(-1)] = True
        if invert:
            mask = ~mask
        return PointCloud(self.points[mask], self.normals[mask] if self.has_normals() else None,
                          self.covariances[mask] if self.has_covariances() else None,
                          self.colors[mask] if self.has_colors() else None)

    def voxel_down_sample(self, voxel_size: float) -> "PointCloud":
        """Open3D ``PointCloud.voxel_down_sample`` on the device (m3d.prep): points, normals and
        colours are each the plain per-voxel mean, voxels in ascending (ix, iy, iz) order.  The
        colours go through the same mean kernel in a second pass over the same voxels."""
        from .prep import voxel_down_sample

        pts, nrm = voxel_down_sample(self.points, voxel_size, normals=self.normals if self.has_normals() else None)
        col = voxel_down_sample(self.points, voxel_size, normals=self.colors)[1] if self.has_colors() else None
        return PointCloud(pts, nrm, colors=col)

    def remove_statistical_outlier(self, nb_neighbors: int, std_ratio: float):
        """Open3D ``PointCloud.remove_statistical_outlier`` on the device (m3d.prep) →
        (filtered cloud, kept indices)."""
        from .prep import remove_statistical_outlier

        ind, _ = remove_statistical_outlier(self.points, nb_neighbors, std_ratio)
        return self.select_by_index(ind), ind

    def remove_radius_outlier(self, nb_points: int, radius: float):
        """Open3D ``PointCloud.remove_radius_outlier`` on the device (m3d.prep) →
        (filtered cloud, kept indices)."""
        from .prep import remove_radius_outlier

        ind = remove_radius_outlier(self.points, nb_points, radius)
        return self.select_by_index(ind), ind

    def segment_plane(self, distance_threshold: float = 0.01, ransac_n: int = 3, num_iterations: int = 100,
                      probability: float = 0.99999999):
        """Open3D ``PointCloud.segment_plane`` on the device (m3d.prep) → (plane_model (4,),
        inlier indices ascending); ``select_by_index(inliers, invert=True)`` drops the plane."""
        from .prep import segment_plane

        return segment_plane(self.points, distance_threshold, ransac_n, num_iterations, probability)

    def cluster_dbscan(self, eps: float, min_points: int, print_progress: bool = False):
        """Open3D ``PointCloud.cluster_dbscan`` on the device (m3d.prep) → labels int32 (n,), −1 =
        noise (``print_progress`` is accepted and ignored)."""
        from .prep import cluster_dbscan

        return cluster_dbscan(self.points, eps, min_points)

    def thin_min_distance(self, radius: float, seed: int = 0):
        """The cloud thinned to a minimum point distance on the device (m3d.prep
        ``thin_min_distance``: original points, no two closer than ``radius``) →
        (thinned cloud, kept indices)."""
        from .prep import thin_min_distance

        ind = thin_min_distance(self.points, radius, seed=seed)
        return self.select_by_index(ind), ind

    def transform(self, T):
        T = np.asarray(T, np.float64)
        self.points = self.points @ T[:3, :3].T + T[:3, 3]
        if len(self.normals):
            self.normals = self.normals @ T[:3, :3].T
        if len(self.covariances):  # C ← R·C·Rᵀ, as Open3D's PointCloud::Transform
            R = T[:3, :3]
            self.covariances = R @ self.covariances @ R.T
        return self
