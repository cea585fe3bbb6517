"""MI355X-native ``matcher`` package — drop-in for KTC-Security-Circle/3d-matching ``src/matcher``.

Put ``3d-matching_amd`` on ``PYTHONPATH`` where the reference put ``src``
(`.devcontainer/Dockerfile:39`) and ``from matcher.ransac import ...`` / ``from matcher.icp
import ...`` resolve to these modules.  (The package namespace keeps ``matcher.ransac`` and
``matcher.icp`` as the submodules, exactly like the reference's empty ``__init__``.)  ``register(source, target)`` is the coarse-to-fine
façade the reference's ``main()`` intends (`src/main.py:34-38`).
"""

from __future__ import annotations

from .colored import registration_colored_icp
from .evaluate import (
    compute_point_cloud_distance,
    compute_point_cloud_to_mesh_distance,
    evaluate_registration,
    get_information_matrix_from_point_clouds,
)
from .fgr import (
    global_registration_fgr,
    registration_fgr_based_on_correspondence,
    registration_fgr_based_on_feature_matching,
)
from .gicp import registration_generalized_icp
from .icp import refine_registration, registration_icp
from .mesh_icp import (
    evaluate_registration_to_mesh,
    refine_registration_to_mesh,
    registration_icp_to_mesh,
)
from .ransac import (
    compute_feature_correspondences,
    compute_step_transformation,
    evaluate_inlier_ratio,
    evaluate_inlier_ratio_fast,
    global_registration,
    run_ransac,
)
from .register import register, register_to_mesh
from .robust import CauchyLoss, GMLoss, HuberLoss, L1Loss, L2Loss, TukeyLoss

__all__ = [
    "CauchyLoss",
    "GMLoss",
    "HuberLoss",
    "L1Loss",
    "L2Loss",
    "TukeyLoss",
    "compute_feature_correspondences",
    "compute_point_cloud_distance",
    "compute_point_cloud_to_mesh_distance",
    "compute_step_transformation",
    "evaluate_inlier_ratio",
    "evaluate_inlier_ratio_fast",
    "evaluate_registration",
    "evaluate_registration_to_mesh",
    "get_information_matrix_from_point_clouds",
    "global_registration",
    "global_registration_fgr",
    "registration_fgr_based_on_correspondence",
    "registration_fgr_based_on_feature_matching",
    "run_ransac",
    "refine_registration",
    "refine_registration_to_mesh",
    "registration_colored_icp",
    "registration_generalized_icp",
    "registration_icp",
    "registration_icp_to_mesh",
    "register",
    "register_to_mesh",
]
