"""ICP against a triangle mesh's SURFACE: refine a scan against the CAD model itself.

``refine_registration`` and every other ICP of this package take a point cloud as target; against
a CAD-like tessellation (large flat triangles, few vertices) the model's vertices are the wrong
target.  Here the target of a source point is the closest point on the mesh's surface
(``m3d.mesh.closest_points``' winner within ``max_correspondence_distance``) and the normal is the
winning triangle's face normal: Open3D's ``registration_icp`` with
``TransformationEstimationPointToPlane(kernel)`` and that correspondence, entirely on the device
(csrc/mesh_icp.hip, restated in numpy by tests/mesh_icp_restatement.py).

Point-to-point estimation, Generalized and Colored ICP against a mesh are not implemented.
"""

from __future__ import annotations

import numpy as np

from m3d import cache as _cache
from m3d import mesh as _mesh
from m3d.types import RegistrationResult

from .icp import _full_cloud

__all__ = ["registration_icp_to_mesh", "evaluate_registration_to_mesh", "refine_registration_to_mesh"]


def _as_mesh(mesh) -> _mesh.TriangleMesh:
    """A ``TriangleMesh``, or a ``(vertices, triangles)`` pair."""
    if isinstance(mesh, _mesh.TriangleMesh):
        return mesh
    vertices, triangles = mesh
    return _mesh.TriangleMesh(vertices, triangles)


def _source(source):
    pts, _ = _full_cloud(source)
    return _cache.clouds([(pts, None)])[0]


def _check_radius(max_correspondence_distance):
    if not (np.isfinite(max_correspondence_distance) and max_correspondence_distance > 0.0):
        raise ValueError("Invalid max_correspondence_distance.")


def registration_icp_to_mesh(source, mesh, max_correspondence_distance, init=None, relative_fitness=1e-6,
                             relative_rmse=1e-6, max_iteration=30, kernel=None, path=None) -> RegistrationResult:
    """``registration_icp`` of ``source`` (anything ``registration_icp`` accepts) against the surface
    of ``mesh`` (a ``TriangleMesh`` or a ``(vertices, triangles)`` pair).  ``kernel``: a robust kernel
    of ``matcher.robust``; ``path``: "auto" | "brute" | "grid", which changes the work and not a bit
    of the result.  ``correspondence_set`` is (M, 2): source index, triangle index."""
    _check_radius(max_correspondence_distance)
    out = _mesh.icp_to_mesh(_source(source), _as_mesh(mesh), max_correspondence_distance, init=init,
                            relative_fitness=relative_fitness, relative_rmse=relative_rmse,
                            max_iteration=max_iteration, kernel=kernel, path=path)
    return RegistrationResult(out.transformation, out.fitness, out.inlier_rmse, out.correspondence_set)


def evaluate_registration_to_mesh(source, mesh, max_correspondence_distance, transformation=None) -> RegistrationResult:
    """``evaluate_registration`` against the surface of ``mesh``: fitness, inlier_rmse and the
    (source index, triangle index) pairs of the pose ``transformation``, in one evaluation."""
    _check_radius(max_correspondence_distance)
    T = np.eye(4) if transformation is None else np.asarray(transformation, np.float64).reshape(4, 4)
    out = _mesh.icp_to_mesh(_source(source), _as_mesh(mesh), max_correspondence_distance, init=T, max_iteration=0)
    return RegistrationResult(out.transformation, out.fitness, out.inlier_rmse, out.correspondence_set)


def refine_registration_to_mesh(src, mesh, init_trans, voxel_size, kernel=None) -> RegistrationResult:
    """``refine_registration`` with the model's surface as target: radius 0.4·voxel_size."""
    return registration_icp_to_mesh(src, mesh, voxel_size * 0.4, init_trans, kernel=kernel)
