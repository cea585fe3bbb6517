"""Fast Global Registration (Zhou, Park, Koltun) on the device: Open3D's
``registration_fgr_based_on_feature_matching`` and ``registration_fgr_based_on_correspondence``.

The coarse pose without a sample budget: the mutual nearest neighbours in FPFH space (or the
caller's rows), the tuple test, then 64 Gauss–Newton steps with a graduated robust weight
(``m3d.prep.fgr_on_correspondences``, csrc/fgr.hip; the semantics are restated in include/m3d.h).
The tuple test draws from the project's counter sampler keyed by ``option.seed`` — not Open3D's
mt19937 stream — so a call is reproducible bit for bit.

PARITY UNPINNED against Open3D itself, as for every other Open3D-backed step.
"""

from __future__ import annotations

import numpy as np

from m3d.types import FastGlobalRegistrationOption, RegistrationResult

from .ransac import _down_points

__all__ = ["registration_fgr_based_on_feature_matching", "registration_fgr_based_on_correspondence",
           "global_registration_fgr"]


def _result(out) -> RegistrationResult:
    return RegistrationResult(out.transformation, out.fitness, out.inlier_rmse, out.correspondence_set)


def _feature_count(f) -> int:
    if not isinstance(f, np.ndarray) and hasattr(f, "data") and hasattr(f, "num"):
        return int(f.num())
    shape = tuple(f.shape) if hasattr(f, "shape") else np.asarray(f).shape  # (a device tensor stays there)
    return int(shape[0]) if len(shape) == 2 else -1


def registration_fgr_based_on_correspondence(source, target, corres, option=None) -> RegistrationResult:
    """Open3D ``registration_fgr_based_on_correspondence``: ``corres`` is (N, 2) (source, target)
    rows into the two clouds (Ply-likes with ``pcd_down``, objects with ``points``, (N, 3) arrays)."""
    from m3d import prep

    return _result(prep.fgr_on_correspondences(_down_points(source), _down_points(target), corres, option))


def registration_fgr_based_on_feature_matching(source, target, source_feature, target_feature,
                                               option=None) -> RegistrationResult:
    """Open3D ``registration_fgr_based_on_feature_matching``: the rows are the mutual nearest
    neighbours of the two feature sets (N×33 rows, or Open3D-style ``Feature`` with 33×N ``data``),
    in increasing source index."""
    from m3d import prep

    s_pts, t_pts = _down_points(source), _down_points(target)
    ns_f, nt_f = _feature_count(source_feature), _feature_count(target_feature)
    if ns_f != len(s_pts) or nt_f != len(t_pts):
        raise ValueError("fgr: one feature row per point of its cloud")
    if ns_f == 0 or nt_f == 0:
        corres = np.zeros((0, 2), np.int32)
    else:  # mutual_consistent_ratio = 0: the one-directional fallback never fires
        corres = prep.feature_correspondences(source_feature, target_feature, True, 0.0)
    return _result(prep.fgr_on_correspondences(s_pts, t_pts, corres, option))


def global_registration_fgr(src, tgt, voxel_size: float, option=None) -> RegistrationResult:
    """The Ply-level call beside ``global_registration``: FGR over ``pcd_down`` / ``pcd_fpfh`` with
    ``maximum_correspondence_distance`` = 0.5·voxel_size (Open3D's tutorial value) unless an
    option is given."""
    if option is None:
        option = FastGlobalRegistrationOption(maximum_correspondence_distance=0.5 * float(voxel_size))
    return registration_fgr_based_on_feature_matching(src, tgt, src.pcd_fpfh, tgt.pcd_fpfh, option)
