"""Open3D's ``o3d.geometry.keypoint`` module on the device.

``compute_iss_keypoints(pcd, ...)`` is Open3D's free function with its signature and its return: a
``PointCloud`` holding the keypoints (``select_by_index`` of their indices, so normals and
covariances are carried), in ascending index order.  The indices themselves, the third eigenvalues
and the neighbour counts come from ``m3d.prep.compute_iss_keypoints``; the contract is in
include/m3d.h.
"""

from __future__ import annotations

from .prep import compute_iss_keypoints as _iss_indices
from .types import PointCloud


def compute_iss_keypoints(input: PointCloud, salient_radius: float = 0.0, non_max_radius: float = 0.0,
                          gamma_21: float = 0.975, gamma_32: float = 0.975, min_neighbors: int = 5) -> PointCloud:
    idx = _iss_indices(input.points, salient_radius, non_max_radius, gamma_21, gamma_32, min_neighbors)
    return input.select_by_index(idx)
