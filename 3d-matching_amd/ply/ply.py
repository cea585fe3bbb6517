"""Point-cloud data holder mirroring the reference's ``src/ply/ply.py``.

``Ply(path, voxel_size)`` follows ply.py:32-135 step by step, with every Open3D call replaced
by the device path of ``m3d.prep``:

1. read the PLY (``m3d.plyio``; Open3D ``read_point_cloud``)                       ply.py:80
1a. optional, not in the reference: ``remove_outliers`` = ``{"nb_neighbors", "std_ratio"}`` or
   ``{"nb_points", "radius"}`` filters ``pcd`` (points and file normals) on the device like
   Open3D's ``remove_statistical_outlier`` / ``remove_radius_outlier`` before step 2; the
   default ``None`` leaves every result as it is without it
1b. optional, not in the reference: ``remove_plane`` = ``{"distance_threshold"}`` plus optional
   ``ransac_n``, ``num_iterations``, ``probability``, ``seed`` drops the inliers of Open3D's
   ``segment_plane`` (the table or floor a scanned part stands on) from ``pcd`` after 1a;
   ``plane_model`` and ``plane_removed`` keep the plane and the number of points dropped
1c. optional, not in the reference: ``keep_cluster`` = ``{"eps", "min_points"}`` keeps the largest
   cluster of Open3D's ``cluster_dbscan`` (the object, without the clamp, the hand and the plane's
   leftover rim) after 1b; ``cluster_label``, ``cluster_size`` and ``num_clusters`` keep what was
   found; no cluster at all is a ``ValueError``
2. ``pcd_down`` = voxel down-sample (voxel_size); file normals and colours (``red green blue``,
   kept in ``pcd.colors``), when present, are averaged per voxel like Open3D's VoxelDownSample
                                                                                     ply.py:106
3. ``pcd_down`` normals: hybrid search (2·v, 30), oriented by those averaged normals ply.py:110-112
4. ``pcd_fpfh`` = FPFH on ``pcd_down`` (hybrid 5·v, 100) — an Open3D-style ``Feature``
   (``.data`` 33×N)                                                                  ply.py:117-120
4a. optional, not in the reference: ``keypoints`` = any subset of ``{"salient_radius",
   "non_max_radius", "gamma_21", "gamma_32", "min_neighbors"}`` (``{}``: Open3D's defaults) keeps
   only the ISS keypoints of ``pcd_down`` (Open3D's ``compute_iss_keypoints``) in ``pcd_down`` and
   ``pcd_fpfh``; the FPFH rows are still computed on the whole down-sampled cloud, as users do.
   ``keypoint_indices`` (into the down-sampled cloud) and ``keypoint_radii`` (salient, non-max, as
   used) record what was kept
5. Gaussian noise N(0, 0.05²) on ``pcd_down`` points from the GLOBAL numpy RNG, after the
   features (the reference's robustness test)                                        ply.py:61-62
6. ``pcd`` normals: hybrid search (2·v, 30), oriented by normals read from the file  ply.py:65,133

``Ply.from_arrays`` builds one from arrays (synthetic clouds, tests, benchmarks) without any
preprocessing unless ``preprocess=True``.

``Ply.from_mesh`` builds one from a triangle mesh (a CAD model, an STL file): ``pcd`` is points drawn
uniformly from the model's SURFACE with their face normals (``TriangleMesh.sample_points_uniformly``)
and goes through the same steps 1a–6.  The reference's way from an STL to a ``Ply`` keeps the STL's
vertices and drops its faces (``convert_stl-ply.py``); ``Ply(path)`` itself keeps refusing anything
but a ``.ply``.
"""

from __future__ import annotations

import time
from pathlib import Path

import numpy as np

from m3d.types import Feature, PointCloud

# Ply.from_mesh's default sample count: 16 samples per voxel-sized square of surface, so that a
# voxel of the down-sampled cloud averages about that many; clamped to [MIN, MAX].  A stated
# default, not a tuned one.
MESH_SAMPLES_PER_VOXEL_AREA = 16
MESH_SAMPLES_MIN = 10_000
MESH_SAMPLES_MAX = 5_000_000


def _mesh_of(mesh):
    """A ``TriangleMesh``, a ``(vertices, triangles)`` pair, or the path of an STL file."""
    from m3d import mesh as M

    if isinstance(mesh, M.TriangleMesh):
        return mesh
    if isinstance(mesh, (str, Path)):
        return M.read_triangle_mesh(mesh)
    vertices, triangles = mesh
    return M.TriangleMesh(vertices, triangles)


def mesh_sample_count(area: float, voxel_size: float) -> int:
    """``Ply.from_mesh``'s default ``number_of_points``: ceil(16·area / voxel²) in [10,000, 5,000,000]."""
    want = np.ceil(MESH_SAMPLES_PER_VOXEL_AREA * float(area) / (float(voxel_size) * float(voxel_size)))
    return int(min(max(want, MESH_SAMPLES_MIN), MESH_SAMPLES_MAX)) if np.isfinite(want) else MESH_SAMPLES_MAX


class Ply:
    def __init__(self, path, voxel_size: float = 0.3, remove_outliers: dict | None = None,
                 remove_plane: dict | None = None, keep_cluster: dict | None = None,
                 keypoints: dict | None = None) -> None:
        self.path = Path(path)
        self.voxel_size = voxel_size
        if not self.path.exists():
            raise FileNotFoundError(f"Ply file not found: {self.path}")     # ply.py:46-48
        if self.path.suffix.lower() != ".ply":
            raise TypeError(f"File is not a ply file: {self.path}")         # ply.py:49-51
        from m3d import plyio

        t0 = time.perf_counter()
        pcd = plyio.read_point_cloud(self.path)  # points, normals and colours where the file has them
        self.stage_ms = {"read": (time.perf_counter() - t0) * 1e3}
        if len(pcd.points) == 0:
            raise ValueError(f"Point cloud is empty: {self.path}")          # ply.py:81-84
        self.pcd = pcd
        self._preprocess(voxel_size, remove_outliers, remove_plane, keep_cluster, keypoints)

    def _remove_outliers(self, params: dict) -> None:
        """``pcd`` ← the points (and file normals) one of Open3D's two outlier filters keeps."""
        keys = set(params)
        if keys == {"nb_neighbors", "std_ratio"}:
            self.pcd, _ = self.pcd.remove_statistical_outlier(params["nb_neighbors"], params["std_ratio"])
        elif keys == {"nb_points", "radius"}:
            self.pcd, _ = self.pcd.remove_radius_outlier(params["nb_points"], params["radius"])
        else:
            raise ValueError("remove_outliers: {'nb_neighbors', 'std_ratio'} or {'nb_points', 'radius'}")

    _PLANE_KEYS = {"distance_threshold", "ransac_n", "num_iterations", "probability", "seed"}

    def _remove_plane(self, params: dict) -> None:
        """``pcd`` ← the points (and file normals) outside the segmented plane's inliers."""
        from m3d import prep

        keys = set(params)
        if "distance_threshold" not in keys or not keys <= self._PLANE_KEYS:
            raise ValueError("remove_plane: {'distance_threshold'} plus optional 'ransac_n', 'num_iterations', "
                             "'probability', 'seed'")
        plane, inliers, out = prep.segment_plane(self.pcd.points, params["distance_threshold"],
                                                 params.get("ransac_n", 3), params.get("num_iterations", 100),
                                                 params.get("probability", 0.99999999),
                                                 seed=params.get("seed", 0), with_details=True)
        self.plane_model = plane
        self.plane_ransac = out.ransac_plane  # the plane the removed points were tested against
        self.plane_removed = len(inliers)
        self.pcd = self.pcd.select_by_index(inliers, invert=True)

    def _keep_cluster(self, params: dict) -> None:
        """``pcd`` ← the points (and file normals) of the largest DBSCAN cluster."""
        from m3d import prep

        if set(params) != {"eps", "min_points"}:
            raise ValueError("keep_cluster: {'eps', 'min_points'}")
        labels, out = prep.cluster_dbscan(self.pcd.points, params["eps"], params["min_points"], with_details=True)
        if out.num_clusters == 0:
            raise ValueError("keep_cluster: no cluster found (every point is noise)")
        self.cluster_label = out.largest_label
        self.cluster_size = out.largest_size
        self.num_clusters = out.num_clusters
        self.pcd = self.pcd.select_by_index(np.flatnonzero(labels == out.largest_label))

    _ISS_KEYS = {"salient_radius", "non_max_radius", "gamma_21", "gamma_32", "min_neighbors"}

    def _keep_keypoints(self, params: dict, cloud) -> None:
        """``pcd_down`` and ``pcd_fpfh`` ← their rows at the ISS keypoints of ``pcd_down``."""
        from m3d import prep

        idx, out = prep.compute_iss_keypoints(cloud, **params, with_details=True)
        self.keypoint_indices = idx
        self.keypoint_radii = (out.salient_radius, out.non_max_radius)
        self.pcd_down = self.pcd_down.select_by_index(idx)
        self.pcd_fpfh = Feature(np.ascontiguousarray(self.pcd_fpfh.data[:, idx]))

    def _preprocess(self, voxel_size: float, remove_outliers: dict | None = None,
                    remove_plane: dict | None = None, keep_cluster: dict | None = None,
                    keypoints: dict | None = None) -> None:
        """ply.py:53-66.  Wall time of each stage lands in ``stage_ms`` (every stage returns host
        arrays, so the device work is complete when its timer stops)."""
        from m3d import prep
        from m3d.core import Cloud, to_device

        if keypoints is not None and not set(keypoints) <= self._ISS_KEYS:
            raise ValueError("keypoints: any of 'salient_radius', 'non_max_radius', 'gamma_21', 'gamma_32', "
                             "'min_neighbors'")
        v = voxel_size
        ms = getattr(self, "stage_ms", None)
        if ms is None:
            ms = self.stage_ms = {}
        t = time.perf_counter()

        def lap(name):
            nonlocal t
            now = time.perf_counter()
            ms[name] = (now - t) * 1e3
            t = now

        if remove_outliers is not None:
            self._remove_outliers(remove_outliers)
            lap("remove_outliers")
        if remove_plane is not None:
            self._remove_plane(remove_plane)
            lap("remove_plane")
        if keep_cluster is not None:
            self._keep_cluster(keep_cluster)
            lap("keep_cluster")
        # the full cloud goes to the device once (down-sampling, then its normals), the
        # down-sampled one once (its normals, then FPFH: the noise is added after, ply.py:61-62)
        p_dev = to_device(self.pcd.points)
        prev = self.pcd.normals if self.pcd.has_normals() else None
        # VoxelDownSample carries the file's normals (their plain per-voxel mean) into pcd_down,
        # and EstimateNormals then orients each new normal by that mean (ply.py:106-112)
        down, down_prev = prep.voxel_down_sample(p_dev, v, normals=prev)
        # ... and the file's colours, the same way (Colored ICP reads them from pcd_down)
        down_col = prep.voxel_down_sample(p_dev, v, normals=self.pcd.colors)[1] if self.pcd.has_colors() else None
        lap("voxel_down_sample")
        c_down = Cloud(down, down_prev)
        down_n = prep.estimate_normals(c_down, 2 * v, 30)
        lap("normals_down")
        self.pcd_down = PointCloud(down, down_n, colors=down_col)
        self.pcd_fpfh = Feature(prep.compute_fpfh(c_down, down_n, 5 * v, 100).T)
        lap("fpfh")
        if keypoints is not None:
            self._keep_keypoints(keypoints, c_down)
            lap("keypoints")
        noise = 0.05 * np.random.randn(*self.pcd_down.points.shape)      # ply.py:61-62
        self.pcd_down.points = self.pcd_down.points + noise
        lap("noise")
        # existing normals orient the estimate like Open3D (the cloud carries them)
        self.pcd.normals = prep.estimate_normals(Cloud(p_dev, prev), 2 * v, 30)
        lap("normals_full")

    @classmethod
    def from_arrays(cls, points, normals=None, points_down=None, fpfh=None, voxel_size: float = 0.3,
                    preprocess: bool = False, remove_outliers: dict | None = None,
                    remove_plane: dict | None = None, keep_cluster: dict | None = None,
                    keypoints: dict | None = None):
        obj = cls.__new__(cls)
        obj.path = None
        obj.voxel_size = voxel_size
        obj.pcd = PointCloud(points, normals)
        if preprocess:
            obj._preprocess(voxel_size, remove_outliers, remove_plane, keep_cluster, keypoints)
            return obj
        obj.pcd_down = PointCloud(points if points_down is None else points_down)
        obj.pcd_fpfh = None if fpfh is None else Feature(np.asarray(fpfh, np.float64))
        return obj

    @classmethod
    def from_mesh(cls, mesh, voxel_size: float = 0.3, number_of_points: int | None = None, seed: int = 0,
                  remove_outliers: dict | None = None, remove_plane: dict | None = None,
                  keep_cluster: dict | None = None, keypoints: dict | None = None):
        """A ``Ply`` of a triangle mesh (``TriangleMesh``, ``(vertices, triangles)`` or an STL path):
        ``pcd`` = ``number_of_points`` uniform samples of the surface with their face normals (None:
        ``mesh_sample_count(area, voxel_size)``), then the unchanged preprocessing — the face normals
        orient the estimated ones, which a PLY of the model's vertices never had."""
        m = _mesh_of(mesh)
        if not (np.isfinite(float(voxel_size)) and float(voxel_size) > 0.0):
            raise ValueError("voxel_size must be finite and > 0")
        if number_of_points is None:
            number_of_points = mesh_sample_count(m.get_surface_area(), voxel_size)
        if int(number_of_points) < 1:
            raise ValueError("number_of_points >= 1")
        obj = cls.__new__(cls)
        obj.path = Path(mesh) if isinstance(mesh, (str, Path)) else None
        obj.voxel_size = voxel_size
        t0 = time.perf_counter()
        obj.pcd = m.sample_points_uniformly(int(number_of_points), seed=seed)
        obj.stage_ms = {"sample": (time.perf_counter() - t0) * 1e3}
        obj.mesh = m
        obj._preprocess(voxel_size, remove_outliers, remove_plane, keep_cluster, keypoints)
        return obj
