"""Point-to-mesh distance without a GPU: the numpy restatement of the contract
(tests/mesh_restatement.py) against answers worked out by hand, and the host side of m3d.mesh (STL
round trip, RaycastingScene's index offsets, index validation, the C symbols)."""
import ctypes as C

import numpy as np
import pytest

import mesh_restatement as R
import m3d.mesh as M
from m3d import _lib, plyio, synth

A, B, Cc, TRI_V, TRI_F = R.A, R.B, R.Cc, R.TRI_V, R.TRI_F
REGION_CASES, ZERO_CASES = R.REGION_CASES, R.ZERO_CASES


def test_seven_regions_by_hand():
    q = np.array([c[0] for c in REGION_CASES])
    out = R.closest_points(TRI_V, TRI_F, q)
    np.testing.assert_array_equal(out["region"], [c[1] for c in REGION_CASES])
    np.testing.assert_array_equal(out["point"], np.array([c[2] for c in REGION_CASES]))
    np.testing.assert_array_equal(out["uv"], np.array([c[3] for c in REGION_CASES]))
    np.testing.assert_array_equal(out["d2"], [c[4] for c in REGION_CASES])
    np.testing.assert_array_equal(out["triangle"], 0)


def test_zero_distance_is_exact():
    q = np.array([c[0] for c in ZERO_CASES])
    out = R.closest_points(TRI_V, TRI_F, q)
    np.testing.assert_array_equal(out["region"], [c[1] for c in ZERO_CASES])
    assert (out["d2"] == 0.0).all()
    np.testing.assert_array_equal(out["point"], q)


def test_random_queries_against_samples_and_plane():
    """d² is no larger than the distance to any sampled point of the triangle and no smaller than
    the plane distance where the projection falls inside.  Slack 1e-12 relative: both sides are a
    handful of fp64 operations on numbers of order one."""
    rng = np.random.default_rng(7)
    q = rng.uniform(-1.5, 2.5, (200, 3))
    out = R.closest_points(TRI_V, TRI_F, q)
    g = np.arange(41) / 40.0
    v, w = np.meshgrid(g, g, indexing="ij")
    keep = v + w <= 1.0
    samples = v[keep][:, None] * np.array(B) + w[keep][:, None] * np.array(Cc)
    dmin = ((q[:, None, :] - samples[None, :, :]) ** 2).sum(axis=2).min(axis=1)
    assert (out["d2"] <= dmin * (1 + 1e-12)).all()
    inside = (q[:, 0] > 0) & (q[:, 1] > 0) & (q[:, 0] + q[:, 1] < 1)
    assert inside.sum() >= 5
    assert (out["d2"][inside] >= q[inside, 2] ** 2 * (1 - 1e-12)).all()
    assert (out["region"][inside] == 6).all()
    assert (out["d2"] >= q[:, 2] ** 2 * (1 - 1e-12)).all()
    # the barycentric pair reproduces the point
    a, b, c = TRI_V
    rec = (1 - out["uv"][:, :1] - out["uv"][:, 1:]) * a + out["uv"][:, :1] * b + out["uv"][:, 1:] * c
    np.testing.assert_allclose(rec, out["point"], atol=1e-14)


def test_ties_and_skipped_triangles():
    v = np.array([A, B, Cc, (0.0, 0.0, 0.0), (2.0, 0.0, 0.0), (4.0, 0.0, 0.0)])
    f = np.array([[3, 4, 5], [3, 3, 3], [0, 1, 2], [0, 1, 2]])  # collinear, a point, two copies
    np.testing.assert_array_equal(R.usable(v, f), [False, False, True, True])
    out = R.closest_points(v, f, np.array([[0.0, 0.0, 0.0], [3.0, 0.0, 0.5]]))
    np.testing.assert_array_equal(out["triangle"], [2, 2])
    with pytest.raises(ValueError):
        R.closest_points(v, f[:2], np.zeros((1, 3)))


def test_q64_of_order():
    T = np.array([[0.0, -1.0, 0.0, 0.5], [1.0, 0.0, 0.0, -2.0], [0.0, 0.0, 1.0, 3.0], [0, 0, 0, 1.0]])
    p = np.array([[1.0, 2.0, 3.0]])
    np.testing.assert_array_equal(R.q64_of(T, p), [[-1.5, -1.0, 6.0]])


def test_read_triangle_mesh_round_trips_stl(tmp_path):
    v, f = synth.surface_mesh(4, 6, seed=3)
    for binary in (True, False):
        path = tmp_path / f"m{int(binary)}.stl"
        plyio.write_stl(path, v, f, binary=binary)
        m = M.read_triangle_mesh(path)
        assert m.has_triangles() and len(m.triangles) == len(f) and m.triangles.dtype == np.int32
        v32 = v.astype(np.float32)  # what an STL stores (ASCII: nine digits, which name one float32)
        assert m.vertices.dtype == np.float64
        np.testing.assert_array_equal(m.vertices[m.triangles].astype(np.float32), v32[f])
        if binary:
            np.testing.assert_array_equal(m.vertices[m.triangles], v32[f].astype(np.float64))
        assert len(m.vertices) == len(np.unique(v32, axis=0))
    ply = tmp_path / "m.ply"
    plyio.write_ply(ply, v)
    with pytest.raises(ValueError, match="PLY face lists"):
        M.read_triangle_mesh(ply)


def test_triangle_mesh_host_side():
    m = M.TriangleMesh(TRI_V, TRI_F)
    np.testing.assert_array_equal(m.triangle_normals(), [[0.0, 0.0, 1.0]])
    T = np.eye(4)
    T[:3, 3] = (1.0, 2.0, 3.0)
    m.transform(T)
    np.testing.assert_array_equal(m.vertices, TRI_V + (1.0, 2.0, 3.0))
    assert not M.TriangleMesh().has_triangles()
    for bad in ([[0, 1, 3]], [[0, -1, 2]]):
        with pytest.raises(ValueError, match="triangle index"):
            M.TriangleMesh(TRI_V, bad)
    with pytest.raises(ValueError):
        M.TriangleMesh(TRI_V, [[0.0, 1.0, 2.5]])


def test_raycasting_scene_offsets(monkeypatch):
    """Two meshes in one scene: the concatenation offsets the second mesh's vertex indices, and a
    winner is mapped back to (geometry, triangle of that geometry).  The closest call is replaced
    by the restatement, so this runs without a device."""
    calls = []

    def fake(mesh, points, transformation=None, path=None, r0=0.0):
        calls.append((len(mesh.vertices), len(mesh.triangles)))
        return R.closest_points(mesh.vertices, mesh.triangles, points, transformation)

    monkeypatch.setattr(M, "closest_points", fake)
    v0 = np.array([A, B, Cc, (1.0, 1.0, 0.0)])
    f0 = np.array([[0, 1, 2], [1, 3, 2]])
    v1 = v0 + (0.0, 0.0, 10.0)
    f1 = np.array([[1, 3, 2], [0, 1, 2], [0, 1, 2]])
    scene = M.RaycastingScene()
    assert scene.add_triangles(M.TriangleMesh(v0, f0)) == 0
    assert scene.add_triangles(v1, f1) == 1
    q = np.array([[0.25, 0.25, 1.0], [0.875, 0.875, 1.0], [0.875, 0.875, 9.0], [0.25, 0.25, 12.0]])
    out = scene.compute_closest_points(q)
    assert calls == [(8, 5)]
    np.testing.assert_array_equal(out["geometry_ids"], [0, 0, 1, 1])
    np.testing.assert_array_equal(out["primitive_ids"], [0, 1, 0, 1])  # local; the copy at 2 loses the tie
    assert out["geometry_ids"].dtype == np.uint32 and out["primitive_ids"].dtype == np.uint32
    np.testing.assert_array_equal(out["points"], [[0.25, 0.25, 0.0], [0.875, 0.875, 0.0], [0.875, 0.875, 10.0], [0.25, 0.25, 10.0]])
    np.testing.assert_array_equal(np.abs(out["primitive_normals"]), np.tile([0.0, 0.0, 1.0], (4, 1)))
    np.testing.assert_array_equal(scene.compute_distance(q), [1.0, 1.0, 1.0, 2.0])
    for name in ("cast_rays", "test_occlusions", "count_intersections", "list_intersections",
                 "compute_signed_distance", "compute_occupancy"):
        with pytest.raises(NotImplementedError):
            getattr(scene, name)(q)
    with pytest.raises(ValueError):
        M.RaycastingScene().compute_distance(q)
    with pytest.raises(ValueError, match="float64"):
        scene.compute_distance(q.astype(np.float32))


def test_c_symbols_and_constants():
    lib = _lib.load()
    assert lib.m3d_mesh_brute_tile() == _lib.MESH_BRUTE_TILE
    assert lib.m3d_mesh_auto_brute_max() >= 0
    assert lib.m3d_mesh_size(None) == -1
    out = (C.c_int64 * 4)()
    assert lib.m3d_mesh_grid_info(None, out) == _lib.M3D_ERR_INVALID
    lib.m3d_mesh_destroy(None)
    h = C.c_void_p()
    assert lib.m3d_mesh_create(None, None, 0, None, 0, C.byref(h)) == _lib.M3D_ERR_INVALID
