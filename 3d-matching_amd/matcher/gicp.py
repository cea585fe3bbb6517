"""Open3D ``pipelines.registration.registration_generalized_icp`` on the device.

Generalized ICP (plane-to-plane) is ``registration_icp`` with another update: every point
carries a 3×3 covariance, and a correspondence's residual d = vs − vt is weighted by
(Ct + Cs)⁻¹ (m3d_gicp_run; semantics restated in ``tests/gicp_restatement.py`` from Open3D 0.19
``GeneralizedICP.cpp``).  As ``InitializePointCloudForGeneralizedICP`` does, each cloud's
covariances are, in this order: its own ``covariances``; else from its ``normals``
(C = Rx·diag(ε, 1, 1)·Rxᵀ); else from normals estimated over every point's 20 nearest neighbours
(``EstimateNormals(KDTreeSearchParamKNN(20))``, m3d.prep.estimate_normals_knn).

PARITY UNPINNED against Open3D itself, as for the rest of the ICP half.
"""

from __future__ import annotations

import numpy as np

from m3d import cache as _cache
from m3d.core import gicp as _gicp
from m3d.prep import estimate_normals_knn
from m3d.types import RegistrationResult

from .icp import _full_cloud

__all__ = ["registration_generalized_icp"]

KNN_NORMALS = 20  # GeneralizedICP.cpp: EstimateNormals(KDTreeSearchParamKNN(20))


def _gicp_cloud(x):
    """(points, normals or None, covariances or None) of a Ply-like, a PointCloud or an array; the
    normals are None when the covariances are given (they take precedence), and estimated over
    KNN(20) when the cloud has neither."""
    pts, nrm = _full_cloud(x)
    pc = x.pcd if hasattr(x, "pcd") else x
    cov = getattr(pc, "covariances", None)
    if cov is not None and len(cov) == len(pts) and len(pts) > 0:
        return pts, None, np.ascontiguousarray(np.asarray(cov, np.float64).reshape(-1, 3, 3))
    if nrm is None and len(pts) > 0:
        nrm = estimate_normals_knn(pts, KNN_NORMALS)
    return pts, nrm, None


def registration_generalized_icp(source, target, max_correspondence_distance, init=None, epsilon=1e-3,
                                 relative_fitness=1e-6, relative_rmse=1e-6,
                                 max_iteration=30, kernel=None) -> RegistrationResult:
    """Open3D ``registration_generalized_icp(source, target, max_correspondence_distance, init,
    TransformationEstimationForGeneralizedICP(epsilon, kernel), ICPConvergenceCriteria(
    relative_fitness, relative_rmse, max_iteration))`` on the device.  ``kernel``: a robust kernel
    of ``matcher.robust``, applied to each whitened residual row; None or ``L2Loss()`` is the
    unweighted estimator."""
    if max_correspondence_distance <= 0.0:
        raise ValueError("Invalid max_correspondence_distance.")
    if not epsilon > 0.0:
        raise ValueError("epsilon must be > 0")
    sp, sn, sc = _gicp_cloud(source)
    tp, tn, tc = _gicp_cloud(target)
    src, tgt = _cache.clouds([(sp, sn), (tp, tn)])
    out = _gicp(src, tgt, max_correspondence_distance, init=np.eye(4) if init is None else init,
                src_cov=sc, tgt_cov=tc, epsilon=epsilon, relative_fitness=relative_fitness,
                relative_rmse=relative_rmse, max_iteration=max_iteration, kernel=kernel)
    return RegistrationResult(out.transformation, out.fitness, out.inlier_rmse, out.correspondence_set)
