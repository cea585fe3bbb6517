"""Judging a given transform on the device: Open3D's ``evaluate_registration``,
``get_information_matrix_from_point_clouds`` and ``PointCloud.compute_point_cloud_distance``, and
the distance to a triangle mesh's SURFACE (``compute_point_cloud_to_mesh_distance``: Open3D's
``RaycastingScene.compute_distance``) where the target is a CAD model.

The three functions take what ``matcher.icp.registration_icp`` takes (Ply-likes with ``.pcd``,
objects with ``.points``, (N, 3) arrays), pack the clouds through the drop-in cache and run
``m3d.core.evaluate`` (m3d_evaluate_registration): the radius-bounded exact 1-NN of the ICP half
followed by one fp64 reduction over the matched pairs.  Nothing is summed on the host.

PARITY UNPINNED against Open3D itself, as for the rest of the ICP half (oracle/icp_oracle.py):
the semantics restate Open3D 0.19 ``Registration.cpp`` (GetRegistrationResultAndCorrespondences,
GetInformationMatrixFromPointClouds) and ``PointCloud::ComputePointCloudDistance``.
"""

from __future__ import annotations

import numpy as np

from m3d import cache as _cache
from m3d.core import evaluate as _evaluate
from m3d.types import RegistrationResult

from .icp import _full_cloud

__all__ = ["evaluate_registration", "get_information_matrix_from_point_clouds",
           "compute_point_cloud_distance", "compute_point_cloud_to_mesh_distance"]


def _T(transformation):
    return np.eye(4) if transformation is None else np.asarray(transformation, np.float64).reshape(4, 4)


def _clouds(source, target):
    sp, _ = _full_cloud(source)
    tp, _ = _full_cloud(target)
    return _cache.clouds([(sp, None), (tp, None)])


def evaluate_registration(source, target, max_correspondence_distance, transformation=None) -> RegistrationResult:
    """Open3D ``pipelines.registration.evaluate_registration``: fitness (matched / source points),
    inlier_rmse and the correspondence set of ``transformation`` (default identity).  A radius
    <= 0 gives the empty result (fitness 0, rmse 0, no pairs), as
    GetRegistrationResultAndCorrespondences returns it, without touching the device."""
    T = _T(transformation)
    if max_correspondence_distance <= 0.0:
        return RegistrationResult(T, 0.0, 0.0, np.zeros((0, 2), np.int32))
    src, tgt = _clouds(source, target)
    out = _evaluate(src, tgt, T, max_correspondence_distance)
    return RegistrationResult(T, out.fitness, out.inlier_rmse, out.correspondence_set)


def get_information_matrix_from_point_clouds(source, target, max_correspondence_distance, transformation):
    """Open3D ``get_information_matrix_from_point_clouds``: the (6, 6) float64 GᵀG over the target
    points matched under ``transformation`` within the radius (rows (0, z, −y, 1, 0, 0),
    (−z, 0, x, 0, 1, 0), (y, −x, 0, 0, 0, 1) per pair) — the edge weight of a pose graph.  Zeros
    for a radius <= 0 (no correspondences)."""
    if max_correspondence_distance <= 0.0:
        return np.zeros((6, 6))
    src, tgt = _clouds(source, target)
    return _evaluate(src, tgt, _T(transformation), max_correspondence_distance, information=True,
                     with_correspondences=False).information


def _reach(sp, tp, T):
    """A radius strictly above every distance between T·sp and tp: 1.001 × the largest
    corner-to-corner distance of their bounding boxes (plus the rounding of the coordinates
    themselves, which matters only for boxes far smaller than their offset), at least tiny."""
    q = sp @ T[:3, :3].T + T[:3, 3]
    lo_s, hi_s, lo_t, hi_t = q.min(axis=0), q.max(axis=0), tp.min(axis=0), tp.max(axis=0)
    span = np.maximum(np.abs(hi_s - lo_t), np.abs(hi_t - lo_s))
    mag = max(np.abs(q).max(), np.abs(tp).max(), np.abs(sp).max() * np.abs(T[:3, :3]).sum(axis=1).max())
    return max(1.001 * (float(np.sqrt(np.sum(span * span))) + 64.0 * np.finfo(np.float64).eps * float(mag)),
               1e-30)


def compute_point_cloud_distance(source, target, transformation=None) -> np.ndarray:
    """Open3D ``PointCloud.compute_point_cloud_distance``: for every point of ``source`` (moved by
    ``transformation`` when given) the distance to its nearest point of ``target`` — the per-point
    deviation of a registered scan from its model.  (ns,) float64.

    The search is the exact brute-force 1-NN at a finite radius beyond both clouds, so no point is
    left unmatched; the result is the square root of the fp64 d² of ``m3d.core.nn1``.  An empty
    target gives 0.0 for every point, as ComputePointCloudDistance does ("Found a point without
    neighbors"); parity with Open3D itself is unpinned, as for the rest of the ICP half."""
    T = _T(transformation)
    sp, _ = _full_cloud(source)
    tp, _ = _full_cloud(target)
    if len(sp) == 0 or len(tp) == 0:
        return np.zeros(len(sp))
    src, tgt = _cache.clouds([(sp, None), (tp, None)])
    out = _evaluate(src, tgt, T, _reach(sp, tp, T), nn="brute", with_correspondences=False,
                    with_distances=True)
    return np.sqrt(out.d2.cpu().numpy())


def compute_point_cloud_to_mesh_distance(source, mesh, transformation=None) -> np.ndarray:
    """For every point of ``source`` (moved by ``transformation`` when given) the distance to the
    closest point on the SURFACE of ``mesh`` (an ``m3d.mesh.TriangleMesh``, or a ``(vertices,
    triangles)`` pair) — Open3D's ``RaycastingScene.compute_distance`` on the transformed points.
    (ns,) float64, the square root of the fp64 d² of ``m3d.mesh.closest_points``.

    ``compute_point_cloud_distance`` against the mesh's vertices answers another question: on a
    flat face made of two large triangles the nearest vertex can be far where the surface is
    touched.  ``source`` is resolved as there (a Ply-like, an object with ``.points``, an array)."""
    from m3d.mesh import TriangleMesh, closest_points

    if not isinstance(mesh, TriangleMesh):
        mesh = TriangleMesh(*mesh)
    sp, _ = _full_cloud(source)
    if len(sp) == 0:
        return np.zeros(0)
    T = None if transformation is None else _T(transformation)
    return np.sqrt(closest_points(mesh, np.ascontiguousarray(sp, np.float64), T)["d2"])
