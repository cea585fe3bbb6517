"""Open3D ``pipelines.registration.registration_colored_icp`` on the device.

Colored ICP (Park, Zhou, Koltun 2017) is ``registration_icp`` with another update: beside the
point-to-plane row, every correspondence adds a photometric row that compares the source point's
intensity with the target's intensity field, linearised in the target point's tangent plane by a
colour gradient built once per call over ``KDTreeSearchParamHybrid(2·max_correspondence_distance,
30)`` (m3d_colored_icp_run; semantics restated in ``tests/colored_restatement.py`` from Open3D
0.19 ``ColoredICP.cpp``).  It locks the in-plane slide that geometry alone leaves on flat or
extruded parts.  The target needs normals and both clouds colours (``PointCloud.colors``, N×3 in
[0, 1]): a ``ValueError`` otherwise, as Open3D raises.

PARITY UNPINNED against Open3D itself, as for the rest of the ICP half.
"""

from __future__ import annotations

import numpy as np

from m3d import cache as _cache
from m3d.core import colored_icp as _colored_icp
from m3d.types import RegistrationResult

from .icp import _full_cloud

__all__ = ["registration_colored_icp"]


def _colored_cloud(x):
    """(points, normals or None, colours or None) of a Ply-like or a PointCloud."""
    pts, nrm = _full_cloud(x)
    pc = x.pcd if hasattr(x, "pcd") else x
    col = getattr(pc, "colors", None)
    if col is None or len(col) != len(pts) or len(pts) == 0:
        return pts, nrm, None
    return pts, nrm, np.ascontiguousarray(np.asarray(col, np.float64).reshape(-1, 3))


def registration_colored_icp(source, target, max_correspondence_distance, init=None, lambda_geometric=0.968,
                             relative_fitness=1e-6, relative_rmse=1e-6, max_iteration=30,
                             kernel=None) -> RegistrationResult:
    """Open3D ``registration_colored_icp(source, target, max_correspondence_distance, init,
    TransformationEstimationForColoredICP(lambda_geometric, kernel), ICPConvergenceCriteria(
    relative_fitness, relative_rmse, max_iteration))`` on the device.  ``kernel``: a robust kernel
    of ``matcher.robust``, applied to the geometric and the photometric row each on its own; None
    or ``L2Loss()`` is the unweighted estimator."""
    if max_correspondence_distance <= 0.0:
        raise ValueError("Invalid max_correspondence_distance.")
    if not 0.0 <= lambda_geometric <= 1.0:
        raise ValueError("lambda_geometric must lie in [0, 1]")
    sp, sn, sc = _colored_cloud(source)
    tp, tn, tc = _colored_cloud(target)
    if tn is None:
        raise ValueError("ColoredICP requires pre-computed normal vectors for target PointCloud.")
    if sc is None or tc is None:
        raise ValueError("ColoredICP requires pre-computed colors for source and target PointCloud.")
    src, tgt = _cache.clouds([(sp, sn), (tp, tn)])
    out = _colored_icp(src, tgt, sc, tc, max_correspondence_distance, init=np.eye(4) if init is None else init,
                       lambda_geometric=lambda_geometric, relative_fitness=relative_fitness,
                       relative_rmse=relative_rmse, max_iteration=max_iteration, kernel=kernel)
    return RegistrationResult(out.transformation, out.fitness, out.inlier_rmse, out.correspondence_set)
