"""Ray casting against triangle meshes (mesh_ray.hip through the C ABI): what a ray hits, how often,
inside/outside by ray parity, the signed distance, and a virtual scan of a model from a pose.

| Open3D                                                   | here                                         |
|----------------------------------------------------------|----------------------------------------------|
| ``RaycastingScene.cast_rays``                             | ``RaycastingScene.cast_rays``, ``cast_rays`` |
| ``RaycastingScene.test_occlusions``                       | ``RaycastingScene.test_occlusions``          |
| ``RaycastingScene.count_intersections``                   | the same method, ``count_intersections``     |
| ``RaycastingScene.compute_occupancy``                     | the same method (ray parity, fixed directions) |
| ``RaycastingScene.compute_signed_distance``               | the same method (``compute_distance`` with the parity's sign) |
| ``RaycastingScene.create_rays_pinhole`` (fov form)        | the same static method                       |
| a depth rendering of the model from a sensor pose         | ``virtual_scan``                             |
| ``RaycastingScene.list_intersections``                    | not implemented                              |

The contract is mesh_ray.h's (restated in numpy by tests/mesh_ray_restatement.py): the watertight
ray-triangle test of Woop, Benthin and Wald (2013) in fp64 in one fixed operation order; the first
hit is the smallest (t, triangle index), ``t`` in units of the ray's direction, which need not be
normalised.  Rays are float64 (..., 6): origin, direction.  The brute-force path and the grid path
return the same bits.  Parity with Open3D itself is unpinned: Embree works in float32.

A ray that passes EXACTLY through an edge or a vertex hits every triangle that shares it (an edge
value of exactly zero counts for both sides, as in Embree without its robust mode): from the
centre of a unit cube along +x, through a face's diagonal, the count is 2.  ``compute_occupancy``
therefore never casts along an axis: its directions are fixed pseudo-random numbers.

``m3d.mesh.RaycastingScene`` keeps its stubs; the scene that casts rays is the subclass here.
"""

from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from . import mesh as _mesh
from .mesh import INVALID_ID, TriangleMesh, _PATHS, _queries, _sample_keys

__all__ = ["RaycastingScene", "cast_rays", "count_intersections", "virtual_scan"]

OCCUPANCY_SEED = 0x6F6363


def _rays(rays) -> np.ndarray:
    r = np.asarray(rays)
    if r.dtype != np.float64 or r.ndim < 1 or r.shape[-1] != 6:
        raise ValueError("rays must be float64 (..., 6): origin, direction")
    return r


def cast_rays(mesh: TriangleMesh, rays, tnear: float = 0.0, tfar: float = np.inf, path=None) -> dict:
    """m3d_mesh_cast_rays: the first hit of every ray with ``tnear <= t <= tfar`` → ``t_hit`` (...)
    f64 (+inf on a miss), ``triangle`` (...) int32 (−1), ``uv`` (..., 2) f64 (NaN; point ≈
    (1−u−v)·a + u·b + v·c).  ``path``: "auto" | "brute" | "grid", which changes no bit of the result.
    ValueError for a mesh without a usable triangle."""
    from .core import _torch, device_empty, ptr, stream_handle, to_device

    r = _rays(rays)
    lead = r.shape[:-1]
    flat = np.ascontiguousarray(r.reshape(-1, 6))
    n = len(flat)
    ctx, h = mesh._handle()
    torch = _torch()
    rd = to_device(flat, "float64", (6,))
    m = max(n, 1)
    t = device_empty((m,), torch.float64)
    tri = device_empty((m,), torch.int32)
    uv = device_empty((m, 2), torch.float64)
    ctx.check(ctx.lib.m3d_mesh_cast_rays(ctx.h, h, ptr(rd), n, float(tnear), float(tfar), _PATHS[path], ptr(t),
                                         ptr(tri), ptr(uv), stream_handle()), "mesh_cast_rays")
    return {"t_hit": t[:n].cpu().numpy().reshape(lead), "triangle": tri[:n].cpu().numpy().reshape(lead),
            "uv": uv[:n].cpu().numpy().reshape(lead + (2,))}


def count_intersections(mesh: TriangleMesh, rays, tnear: float = 0.0, tfar: float = np.inf, path=None) -> np.ndarray:
    """m3d_mesh_count_rays: (...) int32, the usable triangles every ray hits with
    ``tnear <= t <= tfar``."""
    from .core import _torch, device_empty, ptr, stream_handle, to_device

    r = _rays(rays)
    lead = r.shape[:-1]
    flat = np.ascontiguousarray(r.reshape(-1, 6))
    n = len(flat)
    ctx, h = mesh._handle()
    rd = to_device(flat, "float64", (6,))
    cnt = device_empty((max(n, 1),), _torch().int32)
    ctx.check(ctx.lib.m3d_mesh_count_rays(ctx.h, h, ptr(rd), n, float(tnear), float(tfar), _PATHS[path], ptr(cnt),
                                          stream_handle()), "mesh_count_rays")
    return cnt[:n].cpu().numpy().reshape(lead)


def ray_info(mesh: TriangleMesh) -> dict:
    """m3d_mesh_ray_info: the path the mesh's last ray call ran ("brute" | "grid" | None) and how
    many of its rays took the whole-grid fallback."""
    ctx, h = mesh._handle()
    out = (C.c_int64 * 2)()
    ctx.check(ctx.lib.m3d_mesh_ray_info(h, out), "mesh_ray_info")
    return {"path": {0: None, 1: "brute", 2: "grid"}[int(out[0])], "fallback": int(out[1])}


def occupancy_directions(nsamples: int) -> np.ndarray:
    """(nsamples, 3) the fixed directions of ``compute_occupancy``: component k of sample s is
    2u − 1 with u = (key >> 11)·2^-53 and key = ``m3d.mesh._sample_keys(0x6f6363, 3s + k)``.  Not
    normalised."""
    key = _sample_keys(OCCUPANCY_SEED, np.arange(3 * int(nsamples), dtype=np.uint64))
    u = (key >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    return (2.0 * u - 1.0).reshape(-1, 3)


def _face_normals(scene: TriangleMesh, tri: np.ndarray) -> np.ndarray:
    a, b, c = (scene.vertices[scene.triangles[tri, k]] for k in range(3))
    nrm = np.cross(b - a, c - a)
    ln = np.linalg.norm(nrm, axis=-1, keepdims=True)
    return np.divide(nrm, ln, out=np.zeros_like(nrm), where=ln > 0)


class RaycastingScene(_mesh.RaycastingScene):
    """Open3D ``t.geometry.RaycastingScene`` with its ray queries.  ``add_triangles``,
    ``compute_closest_points`` and ``compute_distance`` are the base class's;
    ``list_intersections`` stays unimplemented."""

    def cast_rays(self, rays) -> dict:
        """→ ``t_hit`` (...) f64 (inf on a miss), ``geometry_ids`` and ``primitive_ids`` (...) uint32
        (``INVALID_ID`` on a miss), ``primitive_uvs`` (..., 2) and ``primitive_normals`` (..., 3)
        (zeros on a miss; the unit face normal, as in ``compute_closest_points``)."""
        scene = self._scene()
        out = cast_rays(scene, _rays(rays))
        tri = np.asarray(out["triangle"], np.int64)
        hit = tri >= 0
        safe = np.where(hit, tri, 0)
        geo = np.searchsorted(self._first, safe, side="right") - 1
        local = safe - self._first[geo]
        nrm = _face_normals(scene, safe)
        nrm[~hit] = 0.0
        uv = np.where(hit[..., None], out["uv"], 0.0)
        return {"t_hit": out["t_hit"],
                "geometry_ids": np.where(hit, geo, int(INVALID_ID)).astype(np.uint32),
                "primitive_ids": np.where(hit, local, int(INVALID_ID)).astype(np.uint32),
                "primitive_uvs": uv, "primitive_normals": nrm}

    def test_occlusions(self, rays, tnear: float = 0.0, tfar: float = np.inf) -> np.ndarray:
        """(...) bool: whether the ray hits anything with ``tnear <= t <= tfar``."""
        return cast_rays(self._scene(), _rays(rays), tnear, tfar)["triangle"] >= 0

    def count_intersections(self, rays) -> np.ndarray:
        """(...) int32: the triangles the ray hits."""
        return count_intersections(self._scene(), _rays(rays))

    def compute_occupancy(self, query_points, nsamples: int = 1) -> np.ndarray:
        """(n,) float32, 1 inside and 0 outside a closed mesh: sample s casts every query along
        the same fixed direction (``occupancy_directions``); a point is inside when most of its
        ``nsamples`` (odd) rays hit an odd number of triangles.  The rays are built on the host,
        the counts run on the device."""
        nsamples = int(nsamples)
        if nsamples < 1 or nsamples % 2 == 0:
            raise ValueError("compute_occupancy: nsamples must be odd and >= 1")
        q = _queries(query_points)
        scene = self._scene()
        rays = np.empty((nsamples, len(q), 6))
        rays[:, :, :3] = q[None, :, :]
        rays[:, :, 3:] = occupancy_directions(nsamples)[:, None, :]
        odd = (count_intersections(scene, rays) & 1).sum(axis=0)
        return (2 * odd > nsamples).astype(np.float32)

    def compute_signed_distance(self, query_points, nsamples: int = 1) -> np.ndarray:
        """(n,) float64: ``compute_distance`` with a minus sign where ``compute_occupancy`` is 1."""
        q = _queries(query_points)
        d = self.compute_distance(q)
        return np.where(self.compute_occupancy(q, nsamples) > 0, -d, d)

    @staticmethod
    def create_rays_pinhole(fov_deg: float, center, eye, up, width_px: int, height_px: int) -> np.ndarray:
        """(height_px, width_px, 6) float64 rays of a pinhole camera at ``eye`` looking at
        ``center``, image x to the right and y down:

            z = (center − eye)/|·|, x = (z × up)/|·|, y = z × x, f = 0.5·w / tan(0.5·fov)
            d(row i, column j) = (j + 0.5 − 0.5·w)·x + (i + 0.5 − 0.5·h)·y + f·z,   o = eye

        ``fov_deg`` is the horizontal field of view; the directions are not normalised (the length
        along the viewing axis is f), so ``t_hit``·f is a depth in pixels' units of the axis."""
        w, h = int(width_px), int(height_px)
        if w < 1 or h < 1:
            raise ValueError("create_rays_pinhole: width_px and height_px >= 1")
        eye = np.asarray(eye, np.float64).reshape(3)
        z = np.asarray(center, np.float64).reshape(3) - eye
        x = np.cross(z, np.asarray(up, np.float64).reshape(3))
        f = 0.5 * w / np.tan(0.5 * np.deg2rad(float(fov_deg)))
        lz, lx = np.linalg.norm(z), np.linalg.norm(x)
        if not (np.isfinite(f) and f > 0 and np.isfinite(lz) and np.isfinite(lx) and lz > 0 and lx > 0):
            raise ValueError("create_rays_pinhole: 0 < fov_deg < 180, eye != center, up not along the view")
        z = z / lz
        x = np.cross(z, np.asarray(up, np.float64).reshape(3))
        x = x / np.linalg.norm(x)
        y = np.cross(z, x)
        jj = (np.arange(w) + 0.5 - 0.5 * w)[None, :, None]
        ii = (np.arange(h) + 0.5 - 0.5 * h)[:, None, None]
        rays = np.empty((h, w, 6))
        rays[..., :3] = eye
        rays[..., 3:] = jj * x + ii * y + f * z
        return rays


def virtual_scan(mesh: TriangleMesh, eye, center, up, fov_deg: float, width_px: int, height_px: int,
                 with_details: bool = False):
    """What a depth sensor at ``eye`` looking at ``center`` sees of ``mesh``: one ray per pixel
    (``RaycastingScene.create_rays_pinhole``), the first hits as a ``PointCloud`` of the points
    o + t·d (numpy fp64) with the hit triangles' unit face normals flipped to face the eye.
    ``with_details=True`` → (cloud, {"pixel" (M, 2) int32 row and column, "triangle" (M,) int32,
    "t_hit" (M,) f64})."""
    from .types import PointCloud

    rays = RaycastingScene.create_rays_pinhole(fov_deg, center, eye, up, width_px, height_px)
    out = cast_rays(mesh, rays)
    hit = out["triangle"] >= 0
    r, t, tri = rays[hit], out["t_hit"][hit], out["triangle"][hit]
    pts = r[:, :3] + t[:, None] * r[:, 3:]
    nrm = _face_normals(mesh, tri)
    away = (nrm * r[:, 3:]).sum(axis=1) > 0
    nrm[away] = -nrm[away]
    pc = PointCloud(pts, nrm)
    if not with_details:
        return pc
    return pc, {"pixel": np.argwhere(hit).astype(np.int32), "triangle": tri, "t_hit": t}
