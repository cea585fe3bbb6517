"""Triangle meshes and the point-to-mesh distance (mesh.hip through the C ABI).

What an Open3D user runs after registering a CAD model against a scan and its replacement here:

| Open3D                                                        | here                                   |
|---------------------------------------------------------------|----------------------------------------|
| ``o3d.io.read_triangle_mesh(path)`` (STL)                      | ``read_triangle_mesh``                 |
| ``t.geometry.RaycastingScene.add_triangles``                   | ``RaycastingScene.add_triangles``      |
| ``RaycastingScene.compute_closest_points`` / ``compute_distance`` | the same methods, ``closest_points`` |
| ``registration_icp`` against points sampled from the model      | ``icp_to_mesh`` (``matcher.registration_icp_to_mesh``): the surface itself as target |
| ``mesh.sample_points_uniformly(n)``                             | ``TriangleMesh.sample_points_uniformly``, ``sample_points`` |
| ``mesh.sample_points_poisson_disk(n)``                          | ``TriangleMesh.sample_points_poisson_disk`` (dart throwing, not sample elimination) |
| ``mesh.get_surface_area()``                                     | ``TriangleMesh.get_surface_area``      |
| ``RaycastingScene.cast_rays`` / ``test_occlusions`` / ``count_intersections`` / ``compute_occupancy`` / ``compute_signed_distance`` | ``m3d.raycast.RaycastingScene`` (a subclass of the scene here), ``m3d.raycast.cast_rays``, ``virtual_scan`` |

The contract is mesh.hip's (restated in numpy by tests/mesh_restatement.py): Ericson's closest point
on a triangle in fp64 in one fixed operation order, the winner the smallest (d², triangle index)
over every usable triangle.  Queries are float64 (n, 3); the arithmetic runs on the GPU, the brute
force path and the grid path return the same bits.  Parity with Open3D itself is unpinned (Embree
works in float32).  Ray casting, occupancy and signed distance (ray parity in Open3D) are in
``m3d.raycast``, whose ``RaycastingScene`` extends the one here; the six ray methods of this
module's scene stay stubs that say so.

``icp_to_mesh`` / ``icp_to_mesh_terms`` are mesh_icp.hip's loop and its one-evaluation hook
(restated by tests/mesh_icp_restatement.py): point-to-plane ICP whose target is the closest point
on the mesh's surface with the winning triangle's face normal.

``sample_points`` is mesh_sample.hip's call (restated by tests/mesh_sample_restatement.py): points
drawn from the surface with probability proportional to area, in integer weights and one fixed fp64
operation order, so a sample's bits depend on (mesh, seed, sample number) alone.
"""

from __future__ import annotations

import ctypes as C
from pathlib import Path

import numpy as np

from . import _lib

__all__ = ["TriangleMesh", "RaycastingScene", "read_triangle_mesh", "closest_points", "icp_to_mesh",
           "icp_to_mesh_terms", "sample_points"]

INVALID_ID = np.uint32(0xFFFFFFFF)  # Open3D RaycastingScene.INVALID_ID


class TriangleMesh:
    """Vertices (V, 3) float64 and triangles (F, 3) int32 on the host; the device object
    (m3d_mesh: the arrays, later the triangle grid) is made by the first query and owned here."""

    def __init__(self, vertices=None, triangles=None):
        v = np.zeros((0, 3)) if vertices is None else np.asarray(vertices, np.float64)
        t = np.zeros((0, 3), np.int64) if triangles is None else np.asarray(triangles)
        if v.ndim != 2 or v.shape[1] != 3:
            raise ValueError("vertices must be (V, 3)")
        if t.size and (t.ndim != 2 or t.shape[1] != 3):
            raise ValueError("triangles must be (F, 3)")
        t = t.reshape(-1, 3)
        if t.size and not np.issubdtype(t.dtype, np.integer):
            raise ValueError("triangles must be integers")
        if t.size and (int(t.min()) < 0 or int(t.max()) >= len(v)):
            raise ValueError(f"triangle index outside [0, {len(v)})")
        self.vertices = np.ascontiguousarray(v)
        self.triangles = np.ascontiguousarray(t, np.int32)
        self._h = None
        self._ctx = None

    def has_vertices(self) -> bool:
        return len(self.vertices) > 0

    def has_triangles(self) -> bool:
        return len(self.vertices) > 0 and len(self.triangles) > 0

    def triangle_normals(self) -> np.ndarray:
        """(F, 3) unit face normals (b − a) × (c − a) / |·| (zeros for a zero-area triangle)."""
        a, b, c = (self.vertices[self.triangles[:, k]] for k in range(3))
        n = np.cross(b - a, c - a)
        ln = np.linalg.norm(n, axis=1, keepdims=True)
        return np.divide(n, ln, out=np.zeros_like(n), where=ln > 0)

    def transform(self, T) -> "TriangleMesh":
        """Open3D ``TriangleMesh.transform``: the vertices moved by the 4×4 ``T`` in place; the
        device object is dropped and made again by the next query."""
        T = np.asarray(T, np.float64).reshape(4, 4)
        self.vertices = np.ascontiguousarray(self.vertices @ T[:3, :3].T + T[:3, 3])
        self._release()
        return self

    # ---- device object
    def _handle(self):
        if self._h is None:
            from .core import context, ptr, to_device

            ctx = context()
            v = to_device(self.vertices)
            t = to_device(self.triangles, "int32", (3,))
            h = C.c_void_p()
            ctx.check(ctx.lib.m3d_mesh_create(ctx.h, ptr(v), len(self.vertices), ptr(t), len(self.triangles),
                                              C.byref(h)), "mesh_create")
            self._h, self._ctx = h, ctx
        return self._ctx, self._h

    def _release(self):
        h, self._h = self._h, None
        if h:
            self._ctx.lib.m3d_mesh_destroy(h)

    def __del__(self):
        try:
            self._release()
        except Exception:  # interpreter teardown
            pass

    def grid_info(self) -> dict:
        """m3d_mesh_grid_info: the triangle grid's cells and references, the cell-size doublings of
        its build and the ladder rounds of the last query (0: it ran brute force)."""
        ctx, h = self._handle()
        out = (C.c_int64 * 4)()
        ctx.check(ctx.lib.m3d_mesh_grid_info(h, out), "mesh_grid_info")
        return {"cells": out[0], "references": out[1], "doublings": out[2], "rounds": out[3]}

    def sample_info(self) -> dict:
        """m3d_mesh_sample_info: the total integer weight ``W`` of the sampling table and the
        number of triangles with a non-zero weight (0 and 0 before the first sampling call)."""
        ctx, h = self._handle()
        out = (C.c_uint64 * 2)()
        ctx.check(ctx.lib.m3d_mesh_sample_info(h, out), "mesh_sample_info")
        return {"W": int(out[0]), "nonzero": int(out[1])}

    def get_surface_area(self) -> float:
        """Open3D ``TriangleMesh.get_surface_area``: the sum of the triangles' areas (host numpy;
        a triangle with a coordinate that is not finite counts as 0)."""
        if not self.has_triangles():
            return 0.0
        a, b, c = (self.vertices[self.triangles[:, k]] for k in range(3))
        with np.errstate(all="ignore"):
            ar = 0.5 * np.linalg.norm(np.cross(b - a, c - a), axis=1)
        return float(ar[np.isfinite(ar)].sum())

    def sample_points_uniformly(self, number_of_points: int = 100, use_triangle_normal: bool = True,
                                seed: int = 0, with_details: bool = False):
        """Open3D ``TriangleMesh.sample_points_uniformly`` on the device (``sample_points``) → a
        ``PointCloud`` of ``number_of_points`` points with the face normal of each point's triangle
        (this mesh keeps no vertex normals, so ``use_triangle_normal=False`` returns the points
        without normals).  ``with_details=True`` → (cloud, {"triangle", "uv"}).  The same ``seed``
        gives the same bits; sample k does not depend on ``number_of_points``."""
        from .types import PointCloud

        n = int(number_of_points)
        if n < 0:
            raise ValueError("number_of_points must be >= 0")
        out = sample_points(self, n, seed)
        pc = PointCloud(out["point"], out["normal"] if use_triangle_normal else None)
        return (pc, {"triangle": out["triangle"], "uv": out["uv"]}) if with_details else pc

    def sample_points_poisson_disk(self, number_of_points=None, init_factor: int = 5, radius=None, seed: int = 0,
                                   with_details: bool = False):
        """The call shape of Open3D ``TriangleMesh.sample_points_poisson_disk``; the method is
        DART THROWING, not Open3D's sample elimination: ``init_factor``·N uniform samples
        (``sample_points_uniformly``) thinned to a minimum distance (``prep.thin_min_distance``), so
        no two returned points are closer than the radius used and every point is an original
        uniform sample with its face normal.

        ``radius`` given: the samples are thinned at it and every kept point is returned (N, where
        ``number_of_points`` is None, is ceil(area / radius²) — the count at which the start radius
        below would be this one).  ``number_of_points`` = N alone: the radius starts at
        sqrt(area / N), is bracketed by factors of 1.5 and then cut by at most 6 geometric
        bisections; of the radii tried the largest whose kept count is ≥ N is used and the first N
        kept points in key order (the thinning's own rank) are returned.
        → ``PointCloud``; ``with_details=True`` → (cloud, {"radius", "indices" into the uniform
        samples, "kept" at that radius, "tried": [(radius, kept count)]})."""
        from . import prep
        from .types import PointCloud

        if number_of_points is None and radius is None:
            raise ValueError("sample_points_poisson_disk: number_of_points or radius")
        if radius is not None and not (np.isfinite(float(radius)) and float(radius) > 0.0):
            raise ValueError("sample_points_poisson_disk: radius must be finite and > 0")
        if number_of_points is not None and int(number_of_points) < 1:
            raise ValueError("sample_points_poisson_disk: number_of_points >= 1")
        if int(init_factor) < 1:
            raise ValueError("sample_points_poisson_disk: init_factor >= 1")
        area = self.get_surface_area()
        if radius is not None and number_of_points is None:
            N = max(int(np.ceil(area / (float(radius) * float(radius)))), 1)
        else:
            N = int(number_of_points)
        base = self.sample_points_uniformly(int(init_factor) * N, seed=seed)
        tried = []

        def kept_at(r):
            idx = prep.thin_min_distance(base.points, r, seed=seed)
            tried.append((float(r), len(idx)))
            return idx

        if radius is not None:
            r_used, idx = float(radius), kept_at(float(radius))
        else:
            if not area > 0.0:
                raise ValueError("sample_points_poisson_disk: the mesh has no surface area")
            r = float(np.sqrt(area / N))
            idx = kept_at(r)
            lo = hi = None  # lo: the largest radius tried with ≥ N kept; hi: the smallest with fewer
            if len(idx) >= N:
                lo = (r, idx)
                for _ in range(24):
                    r *= 1.5
                    idx = kept_at(r)
                    if len(idx) < N:
                        hi = r
                        break
                    lo = (r, idx)
            else:
                hi = r
                for _ in range(64):
                    r /= 1.5
                    idx = kept_at(r)
                    if len(idx) >= N:
                        lo = (r, idx)
                        break
                    hi = r
                if lo is None:
                    raise ValueError(f"sample_points_poisson_disk: fewer than {N} distinct samples")
            if hi is not None:
                for _ in range(6):
                    mid = float(np.sqrt(lo[0] * hi))
                    idx = kept_at(mid)
                    if len(idx) >= N:
                        lo = (mid, idx)
                    else:
                        hi = mid
            r_used, idx = lo
        kept = len(idx)
        if number_of_points is not None and radius is None:
            key = _sample_keys(seed, idx)
            idx = np.sort(idx[np.lexsort((idx, key))[:N]])
        pc = PointCloud(base.points[idx], base.normals[idx])
        if not with_details:
            return pc
        return pc, {"radius": r_used, "indices": idx, "kept": kept, "tried": tried}

    def __repr__(self):
        return f"TriangleMesh with {len(self.vertices)} points and {len(self.triangles)} triangles."


def read_triangle_mesh(path) -> TriangleMesh:
    """``o3d.io.read_triangle_mesh`` for STL (binary or ASCII, ``m3d.plyio.read_stl``: vertices
    merged by exact equality).  PLY face lists are not read: a ``.ply`` raises."""
    from .plyio import read_stl

    ext = Path(path).suffix.lower()
    if ext == ".ply":
        raise ValueError(f"{path}: PLY face lists are not supported; read_triangle_mesh reads STL "
                         "(m3d.plyio.read_point_cloud reads a PLY's vertices)")
    if ext != ".stl":
        raise ValueError(f"{path}: unsupported mesh format {ext or '(none)'}; read_triangle_mesh reads STL")
    v, f = read_stl(path)
    return TriangleMesh(v, f)


_PATHS = {None: _lib.MESH_AUTO, "auto": _lib.MESH_AUTO, "brute": _lib.MESH_BRUTE, "grid": _lib.MESH_GRID}


def _queries(points) -> np.ndarray:
    q = np.asarray(points)
    if q.dtype != np.float64:
        raise ValueError("queries must be float64 (n, 3)")
    if q.ndim != 2 or q.shape[1] != 3:
        raise ValueError("queries must be float64 (n, 3)")
    return np.ascontiguousarray(q)


def closest_points(mesh: TriangleMesh, points, transformation=None, path=None, r0: float = 0.0) -> dict:
    """m3d_mesh_closest: for every query (moved by ``transformation`` when given) the closest
    triangle of ``mesh``.  → ``d2`` (n,), ``triangle`` (n,) int32, ``point`` (n, 3), ``uv`` (n, 2)
    (v, w: point ≈ (1−v−w)·a + v·b + w·c), ``region`` (n,) uint8 (0 1 2 vertex a b c, 3 4 5 edge
    ab ac bc, 6 face).  ``path``: "auto" | "brute" | "grid"; ``r0``: the grid path's first radius
    (<= 0: one cell) — neither changes a bit of the result.  ValueError for a mesh without a usable
    triangle."""
    from .core import _torch, device_empty, ptr, stream_handle, to_device

    q = _queries(points)
    n = len(q)
    ctx, h = mesh._handle()
    torch = _torch()
    qd = to_device(q)
    m = max(n, 1)
    d2 = device_empty((m,), torch.float64)
    tri = device_empty((m,), torch.int32)
    pt = device_empty((m, 3), torch.float64)
    uv = device_empty((m, 2), torch.float64)
    reg = device_empty((m,), torch.uint8)
    Tc = None
    if transformation is not None:
        Tc = (C.c_double * 16)(*np.asarray(transformation, np.float64).reshape(16).tolist())
    ctx.check(ctx.lib.m3d_mesh_closest(ctx.h, h, ptr(qd), n, Tc, _PATHS[path], float(r0), ptr(d2), ptr(tri),
                                       ptr(pt), ptr(uv), ptr(reg), stream_handle()), "mesh_closest")
    return {"d2": d2[:n].cpu().numpy(), "triangle": tri[:n].cpu().numpy(), "point": pt[:n].cpu().numpy(),
            "uv": uv[:n].cpu().numpy(), "region": reg[:n].cpu().numpy()}


def _sample_keys(seed: int, index) -> np.ndarray:
    """sampler.h ``sample_base(seed, i)`` for every i of ``index`` (uint64): the thinning's rank key."""
    u = np.uint64
    with np.errstate(over="ignore"):
        z = (u(int(seed) & 0xFFFFFFFFFFFFFFFF) ^ (np.asarray(index).astype(u) * u(0x9E3779B97F4A7C15))) \
            + u(0x9E3779B97F4A7C15)
        z = (z ^ (z >> u(30))) * u(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> u(27))) * u(0x94D049BB133111EB)
        return z ^ (z >> u(31))


def sample_points(mesh: TriangleMesh, n: int, seed: int = 0) -> dict:
    """m3d_mesh_sample: ``n`` points of the surface of ``mesh`` drawn with probability proportional
    to area → ``point`` (n, 3) f64, ``triangle`` (n,) int32, ``uv`` (n, 2) f64 (``closest_points``'
    convention: point ≈ (1−u−v)·a + u·b + v·c), ``normal`` (n, 3) f64 (the triangle's unit face
    normal).  Sample k of a call is a function of (mesh, seed, k) alone.  ValueError for a mesh
    without a usable triangle (or without one of finite non-zero area)."""
    from .core import _torch, device_empty, ptr, stream_handle

    n = int(n)
    if n < 0:
        raise ValueError("sample_points: n >= 0")
    ctx, h = mesh._handle()
    torch = _torch()
    m = max(n, 1)
    pt = device_empty((m, 3), torch.float64)
    tri = device_empty((m,), torch.int32)
    uv = device_empty((m, 2), torch.float64)
    nrm = device_empty((m, 3), torch.float64)
    ctx.check(ctx.lib.m3d_mesh_sample(ctx.h, h, n, int(seed) & 0xFFFFFFFFFFFFFFFF, ptr(pt), ptr(tri), ptr(uv),
                                      ptr(nrm), stream_handle()), "mesh_sample")
    return {"point": pt[:n].cpu().numpy(), "triangle": tri[:n].cpu().numpy(), "uv": uv[:n].cpu().numpy(),
            "normal": nrm[:n].cpu().numpy()}


# The seeded box of the grid scan (mesh_icp.hip) never changes a bit of the result; it is on by
# default only where it measured faster than the unseeded scan (DESIGN §3.21, 180k points, r = 0.12):
# slower by 4–14 % up to 2,304 triangles, equal at 4,096, faster from 16,384 on (2 × at 435,600).
ICP_SEED_MIN_TRIANGLES = 4096


def icp_to_mesh_terms(src, mesh: TriangleMesh, T=None, max_dist: float = 0.0, kernel=None, path=None,
                      seed_triangles=None):
    """m3d_mesh_icp_terms: ONE evaluation of ``src`` (an ``m3d.core.Cloud``) against ``mesh`` at the
    transform ``T`` → (sums (30,) f64 in ``robust_terms``' layout, triangle (ns,) int32 with −1 for
    an unmatched point, d2 (ns,) f64 with inf).  ``seed_triangles`` (ns,) int32 or None: the
    triangles the grid scan tries first; they change the work, never the result."""
    from .core import _T16, _colored_kernel, _torch, device_empty, ptr, stream_handle, to_device

    ctx, h = mesh._handle()
    torch = _torch()
    n = src.n
    tri = device_empty((max(n, 1),), torch.int32)
    d2 = device_empty((max(n, 1),), torch.float64)
    seed = None
    if seed_triangles is not None:
        seed = to_device(np.ascontiguousarray(seed_triangles, np.int32).reshape(-1), "int32", ())
        if seed.shape[0] != n:
            raise ValueError(f"seed_triangles must be ({n},)")
    rk = _colored_kernel(kernel)  # L2 handed on: this loop has one terms pass for every kind
    sums = (C.c_double * 32)()
    ctx.check(ctx.lib.m3d_mesh_icp_terms(ctx.h, h, src.h, _T16(np.eye(4) if T is None else T), float(max_dist),
                                         None if rk is None else C.byref(rk), _PATHS[path],
                                         ptr(seed), sums, ptr(tri), ptr(d2), stream_handle()),
              "mesh_icp_terms")
    return np.array(sums[:30]), tri[:n].cpu().numpy(), d2[:n].cpu().numpy()


def icp_to_mesh(src, mesh: TriangleMesh, max_dist: float, init=None, relative_fitness=1e-6, relative_rmse=1e-6,
                max_iteration=30, kernel=None, path=None, seed=None):
    """m3d_mesh_icp_run: registration_icp of ``src`` (an ``m3d.core.Cloud``) against the surface of
    ``mesh`` → ``m3d.core.IcpOutcome`` whose correspondence_set is (M, 2): source index, triangle
    index.  ``seed``: the grid scan's seeded box (None: on from
    ``ICP_SEED_MIN_TRIANGLES`` triangles)."""
    from .core import _T16, _colored_kernel, _outcome, _torch, device_empty, ptr, stream_handle

    ctx, h = mesh._handle()
    p = _lib.IcpParams(float(relative_fitness), float(relative_rmse), int(max_iteration), _lib.EST_POINT_TO_PLANE,
                       _lib.NN_GRID, 0)
    rk = _colored_kernel(kernel)
    res = _lib.IcpResult()
    tri = device_empty((max(src.n, 1),), _torch().int32)
    use_seed = len(mesh.triangles) >= ICP_SEED_MIN_TRIANGLES if seed is None else bool(seed)
    ctx.check(ctx.lib.m3d_mesh_icp_run(ctx.h, h, src.h, _T16(np.eye(4) if init is None else init), float(max_dist),
                                       C.byref(p), None if rk is None else C.byref(rk), _PATHS[path],
                                       int(use_seed), C.byref(res), ptr(tri), stream_handle()), "mesh_icp_run")
    return _outcome(ctx, res, tri, src.n, True)


class RaycastingScene:
    """Open3D ``t.geometry.RaycastingScene`` as far as closest-point queries go.  Meshes added
    with ``add_triangles`` are concatenated (vertex indices offset) into one mesh at the first
    query; a query's winner is mapped back to (geometry id, triangle of that geometry)."""

    INVALID_ID = INVALID_ID

    def __init__(self):
        self._meshes: list[TriangleMesh] = []
        self._joined: TriangleMesh | None = None
        self._first = np.zeros(1, np.int64)  # first global triangle of each geometry, then the total

    def add_triangles(self, mesh, triangles=None) -> int:
        """``add_triangles(mesh)`` or ``add_triangles(vertices, triangles)`` → the geometry id."""
        m = mesh if isinstance(mesh, TriangleMesh) else TriangleMesh(mesh, triangles)
        if not m.has_triangles():
            raise ValueError("add_triangles: the mesh has no triangles")
        self._meshes.append(m)
        self._joined = None
        return len(self._meshes) - 1

    def _scene(self) -> TriangleMesh:
        if not self._meshes:
            raise ValueError("RaycastingScene: no geometry added")
        if self._joined is None:
            voff = np.cumsum([0] + [len(m.vertices) for m in self._meshes])
            self._first = np.cumsum([0] + [len(m.triangles) for m in self._meshes]).astype(np.int64)
            if len(self._meshes) == 1:
                self._joined = self._meshes[0]
            else:
                v = np.vstack([m.vertices for m in self._meshes])
                t = np.vstack([m.triangles.astype(np.int64) + o for m, o in zip(self._meshes, voff)])
                self._joined = TriangleMesh(v, t)
        return self._joined

    def compute_closest_points(self, query_points) -> dict:
        """→ ``points`` (n, 3), ``geometry_ids`` and ``primitive_ids`` (n,) uint32 (the triangle's
        index within its geometry), ``primitive_uvs`` (n, 2), ``primitive_normals`` (n, 3): the unit
        face normal of the winning triangle."""
        scene = self._scene()
        out = closest_points(scene, _queries(query_points))
        tri = np.asarray(out["triangle"], np.int64)
        hit = tri >= 0
        safe = np.where(hit, tri, 0)
        geo = np.searchsorted(self._first, safe, side="right") - 1
        local = safe - self._first[geo]
        a, b, c = (scene.vertices[scene.triangles[safe, k]] for k in range(3))
        nrm = np.cross(b - a, c - a)
        ln = np.linalg.norm(nrm, axis=1, keepdims=True)
        nrm = np.divide(nrm, ln, out=np.zeros_like(nrm), where=ln > 0)
        nrm[~hit] = 0.0
        return {"points": out["point"],
                "geometry_ids": np.where(hit, geo, int(INVALID_ID)).astype(np.uint32),
                "primitive_ids": np.where(hit, local, int(INVALID_ID)).astype(np.uint32),
                "primitive_uvs": out["uv"], "primitive_normals": nrm}

    def compute_distance(self, query_points) -> np.ndarray:
        """(n,) float64: the distance to the closest triangle, sqrt of the contract's d²."""
        return np.sqrt(closest_points(self._scene(), _queries(query_points))["d2"])

    # Open3D methods that need a ray caster: m3d.raycast.RaycastingScene, a subclass, has them
    def cast_rays(self, *args, **kwargs):
        raise NotImplementedError("RaycastingScene.cast_rays: use m3d.raycast.RaycastingScene")

    def test_occlusions(self, *args, **kwargs):
        raise NotImplementedError("RaycastingScene.test_occlusions: use m3d.raycast.RaycastingScene")

    def count_intersections(self, *args, **kwargs):
        raise NotImplementedError("RaycastingScene.count_intersections: use m3d.raycast.RaycastingScene")

    def list_intersections(self, *args, **kwargs):
        raise NotImplementedError("RaycastingScene.list_intersections: not implemented (a variable-length "
                                  "output; m3d.raycast has the other ray queries)")

    def compute_signed_distance(self, *args, **kwargs):
        raise NotImplementedError("RaycastingScene.compute_signed_distance: use m3d.raycast.RaycastingScene "
                                  "(the sign is ray parity)")

    def compute_occupancy(self, *args, **kwargs):
        raise NotImplementedError("RaycastingScene.compute_occupancy: use m3d.raycast.RaycastingScene")
