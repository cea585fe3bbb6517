"""``register(source, target)`` — the coarse-to-fine pipeline `src/main.py:24-43` intends.

The reference's ``main()`` calls ``global_registration(src_ply, tgt_ply)`` and
``refine_registration(src_ply, tgt_ply, T)`` without the required ``voxel_size`` (TypeError as
written).  This façade supplies it (``Ply.voxel_size``, default 0.3) and composes
the same two stages on the device:

1. coarse: ``global_registration`` when both inputs carry FPFH features (``pcd_fpfh``), else the
   step-RANSAC loop (``run_ransac``) over the given ``correspondences``; ``coarse="fgr"`` runs Fast
   Global Registration instead (``matcher.fgr``: no sample budget, no dependence on a seed's luck);
2. fine: ``refine_registration`` (point-to-plane ICP, radius 0.4·voxel) from the coarse result;
   ``kernel``: a robust kernel of ``matcher.robust`` for that stage.

``register_to_mesh(source, mesh)`` is the same pipeline against a CAD model: the coarse stage runs
against ``Ply.from_mesh`` (points sampled from the model's SURFACE, with its face normals), the
fine stage against the surface itself (``refine_registration_to_mesh``).
"""

from __future__ import annotations

from .fgr import global_registration_fgr, registration_fgr_based_on_correspondence
from .icp import refine_registration
from .ransac import global_registration, run_ransac


def register(source, target, voxel_size=None, correspondences=None, ransac_iterations: int = 10000,
             refine: bool = True, iteration: int = 30, coarse: str = "ransac", fgr_option=None, kernel=None,
             **ransac_kwargs):
    """Return the refined ``RegistrationResult`` mapping ``source`` onto ``target``.

    ``iteration``: RANSACConvergenceCriteria max_iteration of the feature path
    (global_registration's own default, 30); ``ransac_iterations``: hypotheses of the
    correspondence path.  ``coarse``: "ransac" (the default) or "fgr" (``fgr_option``: a
    ``FastGlobalRegistrationOption``; default maximum_correspondence_distance = 0.5·voxel).
    ``kernel``: the ICP stage's robust kernel (``refine_registration``'s)."""
    v = voxel_size if voxel_size is not None else getattr(source, "voxel_size", 0.3)
    if coarse not in ("ransac", "fgr"):
        raise ValueError("coarse must be 'ransac' or 'fgr'")
    if coarse == "fgr":
        if ransac_kwargs:
            raise TypeError(f"unexpected arguments with coarse='fgr': {sorted(ransac_kwargs)}")
        if correspondences is None and getattr(source, "pcd_fpfh", None) is not None \
                and getattr(target, "pcd_fpfh", None) is not None:
            first = global_registration_fgr(source, target, v, fgr_option)
        elif correspondences is not None:
            if fgr_option is None:
                from m3d.types import FastGlobalRegistrationOption

                fgr_option = FastGlobalRegistrationOption(maximum_correspondence_distance=0.5 * float(v))
            first = registration_fgr_based_on_correspondence(source, target, correspondences, fgr_option)
        else:
            raise ValueError("register needs FPFH features on both inputs (pcd_fpfh) or correspondences")
        return first if not refine else refine_registration(source, target, first.transformation, v, kernel)
    if correspondences is None and getattr(source, "pcd_fpfh", None) is not None \
            and getattr(target, "pcd_fpfh", None) is not None:
        coarse = global_registration(source, target, v, iteration=iteration)
    elif correspondences is not None:
        coarse, _ = run_ransac(source, target, correspondences, voxel_size=v, max_iter=ransac_iterations,
                           **ransac_kwargs)
    else:
        raise ValueError("register needs FPFH features on both inputs (pcd_fpfh) or correspondences")
    if not refine:
        return coarse
    return refine_registration(source, target, coarse.transformation, v, kernel)


def register_to_mesh(source, mesh, voxel_size=None, coarse: str = "ransac", number_of_points=None, seed: int = 0,
                     kernel=None, **register_kwargs):
    """Register the scan ``source`` (a ``Ply``) against the triangle mesh ``mesh`` (a
    ``TriangleMesh``, a ``(vertices, triangles)`` pair or the path of an STL file), end to end:

    1. ``target = Ply.from_mesh(mesh, v, number_of_points, seed)``: uniform samples of the surface,
       preprocessed like a scan (``number_of_points`` None: ``Ply.from_mesh``'s default density);
    2. ``first = register(source, target, v, refine=False, coarse=coarse, **register_kwargs)``;
    3. ``refine_registration_to_mesh(source, mesh, first.transformation, v, kernel)``: point-to-plane
       ICP against the surface itself.

    ``voxel_size`` None: ``source.voxel_size`` (default 0.3)."""
    from ply.ply import Ply, _mesh_of

    from .mesh_icp import refine_registration_to_mesh

    if "refine" in register_kwargs:
        raise TypeError("register_to_mesh always refines against the mesh; use register(..., refine=False) with "
                        "Ply.from_mesh for the coarse stage alone")
    v = voxel_size if voxel_size is not None else getattr(source, "voxel_size", 0.3)
    m = _mesh_of(mesh)
    target = Ply.from_mesh(m, voxel_size=v, number_of_points=number_of_points, seed=seed)
    first = register(source, target, v, refine=False, coarse=coarse, **register_kwargs)
    return refine_registration_to_mesh(source, m, first.transformation, v, kernel)
