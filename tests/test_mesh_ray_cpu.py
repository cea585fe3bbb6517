"""Ray casting without a GPU: the numpy restatement of the contract (tests/mesh_ray_restatement.py)
against answers worked out by hand, the parity property the contract is chosen for, and the host
side of m3d.raycast (the scene's id mapping, the pinhole rays, argument checks, the C symbols)."""
import ctypes as C

import numpy as np
import pytest

import mesh_ray_restatement as R
import m3d.mesh as M
import m3d.raycast as RC
from m3d import _lib

F1 = np.array([[0, 1, 2]])


@pytest.mark.parametrize("case", R.truth_table(), ids=lambda c: c[0])
def test_truth_table_by_hand(case):
    label, v, ray, tnear, tfar, hit, t = case
    out = R.cast_rays(v, F1, ray[None], tnear, tfar)
    cnt = R.count_intersections(v, F1, ray[None], tnear, tfar)
    assert cnt.dtype == np.int32 and cnt[0] == int(hit)
    assert out["triangle"][0] == (0 if hit else -1)
    if hit:
        assert out["t_hit"][0] == t
        a, b, c = v
        u, w = out["uv"][0]
        p = ray[:3] + t * ray[3:]
        np.testing.assert_array_equal((1 - u - w) * a + u * b + w * c, p)  # dyadic: exact
    else:
        assert out["t_hit"][0] == np.inf and np.isnan(out["uv"][0]).all()


def test_edge_values_of_an_exact_edge_are_zero():
    """The edge cases of the table are hits BECAUSE an edge value is exactly zero."""
    for label, v, ray, *_ in R.truth_table():
        if label.startswith("edge ") or label.startswith("vertex "):
            assert (R.edge_values(v, F1, ray[None]) == 0.0).any(), label


def test_lowest_axis_wins_a_tie_and_ties_go_to_the_lower_triangle():
    # |d| equal on x and y: kz = 0; the result does not depend on it, the restatement must not fail
    out = R.cast_rays(R.TRI_V + (0.0, 0.0, 0.0), F1, np.array([[0.25, 1.25, 1.0, 0.0, -1.0, -1.0]]))
    assert out["triangle"][0] == 0 and out["t_hit"][0] == 1.0
    # the same triangle twice, an unusable one between: the lower index wins, the count is 2
    v = np.vstack([R.TRI_V, [[0, 0, 0], [1, 1, 1], [2, 2, 2]], R.TRI_V])
    f = np.array([[6, 7, 8], [3, 4, 5], [0, 1, 2]])
    ray = np.array([[0.25, 0.25, 1.0, 0.0, 0.0, -1.0]])
    assert R.cast_rays(v, f, ray)["triangle"][0] == 0
    assert R.count_intersections(v, f, ray)[0] == 2
    with pytest.raises(ValueError):
        R.cast_rays(v, f[1:2], ray)


def test_icosphere_parity_is_exact():
    """1280 triangles, 4096 rays from inside (all odd) and 4096 from outside (all even), and no
    edge value of any pair is zero: the inputs stay clear of the documented tie."""
    v, f = R.icosphere(3)
    assert len(f) == 1280
    rng = np.random.default_rng(1)
    inside = np.hstack([rng.uniform(-0.5, 0.5, (4096, 3)), rng.standard_normal((4096, 3))])
    o = rng.standard_normal((4096, 3))
    o = o / np.linalg.norm(o, axis=1, keepdims=True) * rng.uniform(1.5, 3.0, (4096, 1))
    outside = np.hstack([o, rng.standard_normal((4096, 3))])
    ci, co = R.count_intersections(v, f, inside), R.count_intersections(v, f, outside)
    assert (ci == 1).all()
    assert np.isin(co, (0, 2)).all() and (co == 2).sum() > 100
    for rays in (inside, outside):
        for i0 in range(0, len(rays), 512):
            assert (R.edge_values(v, f, rays[i0:i0 + 512]) != 0.0).all()
    # the first hit from inside lies on the sphere's mesh: between the inscribed and the unit radius
    out = R.cast_rays(v, f, inside)
    r = np.linalg.norm(inside[:, :3] + out["t_hit"][:, None] * inside[:, 3:], axis=1)
    assert (out["triangle"] >= 0).all() and (r > 0.99).all() and (r <= 1.0 + 1e-15).all()


def test_unit_cube_diagonal_counts_two():
    """The documented tie: from the centre along +x the ray runs through the diagonal of the face
    x = 1 and an edge value of exactly zero counts for both triangles."""
    ray = np.array([[0.5, 0.5, 0.5, 1.0, 0.0, 0.0]])
    assert R.count_intersections(R.CUBE_V, R.CUBE_F, ray)[0] == 2
    assert R.count_intersections(R.CUBE_V, R.CUBE_F, np.array([[0.5, 0.5, 0.5, 1.0, 0.3, 0.2]]))[0] == 1
    # the cube is closed and outward: parity holds off the ties
    rng = np.random.default_rng(5)
    rays = np.hstack([rng.uniform(0.1, 0.9, (500, 3)), rng.standard_normal((500, 3))])
    assert (R.count_intersections(R.CUBE_V, R.CUBE_F, rays) == 1).all()


def test_occupancy_directions_are_the_documented_keys():
    d = RC.occupancy_directions(5)
    np.testing.assert_array_equal(d, R.occupancy_directions(5))
    key = M._sample_keys(0x6F6363, np.arange(15))
    np.testing.assert_array_equal(d.reshape(-1), 2.0 * ((key >> np.uint64(11)).astype(np.float64) * 2.0 ** -53) - 1.0)
    assert (np.abs(d) < 1).all() and (np.abs(d) > 1e-3).all()  # no axis direction among them


def test_scene_maps_hits_to_geometry_and_local_ids(monkeypatch):
    """Two meshes in one scene with the device calls replaced by the restatement."""
    calls = []

    def fake_cast(mesh, rays, tnear=0.0, tfar=np.inf, path=None):
        calls.append((len(mesh.vertices), len(mesh.triangles)))
        return R.cast_rays(mesh.vertices, mesh.triangles, rays, tnear, tfar)

    def fake_count(mesh, rays, tnear=0.0, tfar=np.inf, path=None):
        return R.count_intersections(mesh.vertices, mesh.triangles, rays, tnear, tfar)

    monkeypatch.setattr(RC, "cast_rays", fake_cast)
    monkeypatch.setattr(RC, "count_intersections", fake_count)
    v0 = np.array([(0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (1.0, 1.0, 0.0)])
    f0 = np.array([[0, 1, 2], [1, 3, 2]])
    v1 = v0 + (0.0, 0.0, 10.0)
    f1 = np.array([[1, 3, 2], [0, 1, 2], [0, 1, 2]])
    scene = RC.RaycastingScene()
    assert isinstance(scene, M.RaycastingScene)
    assert scene.add_triangles(M.TriangleMesh(v0, f0)) == 0
    assert scene.add_triangles(v1, f1) == 1
    rays = np.array([[[0.25, 0.25, 1.0, 0.0, 0.0, -1.0], [0.875, 0.875, 2.0, 0.0, 0.0, -2.0]],
                     [[0.875, 0.875, 12.0, 0.0, 0.0, -1.0], [0.25, 0.25, 9.0, 0.0, 0.0, 1.0]],
                     [[5.0, 5.0, 1.0, 0.0, 0.0, -1.0], [0.25, 0.25, 11.0, 0.0, 0.0, 1.0]]])
    out = scene.cast_rays(rays)
    assert calls == [(8, 5)]
    M32 = 0xFFFFFFFF
    np.testing.assert_array_equal(out["geometry_ids"], [[0, 0], [1, 1], [M32, M32]])
    np.testing.assert_array_equal(out["primitive_ids"], [[0, 1], [0, 1], [M32, M32]])  # local; the copy at 2 loses
    assert out["geometry_ids"].dtype == np.uint32 and out["primitive_ids"].dtype == np.uint32
    np.testing.assert_array_equal(out["t_hit"], [[1.0, 1.0], [2.0, 1.0], [np.inf, np.inf]])
    np.testing.assert_array_equal(out["primitive_uvs"][2], np.zeros((2, 2)))
    np.testing.assert_array_equal(out["primitive_normals"][2], np.zeros((2, 3)))
    np.testing.assert_array_equal(np.abs(out["primitive_normals"][:2]), np.tile([0.0, 0.0, 1.0], (2, 2, 1)))
    np.testing.assert_array_equal(out["primitive_uvs"][0, 0], [0.25, 0.25])
    np.testing.assert_array_equal(scene.test_occlusions(rays), [[True, True], [True, True], [False, False]])
    np.testing.assert_array_equal(scene.test_occlusions(rays, 0.0, 1.5), [[True, True], [False, True], [False, False]])
    # a ray from above crosses both sheets; the copies at local 1 and 2 of the second mesh both count
    np.testing.assert_array_equal(scene.count_intersections(rays), [[1, 1], [2, 2], [0, 0]])
    assert scene.count_intersections(rays).dtype == np.int32
    with pytest.raises(NotImplementedError):
        scene.list_intersections(rays)
    with pytest.raises(ValueError):
        RC.RaycastingScene().cast_rays(rays)
    with pytest.raises(ValueError, match="odd"):
        scene.compute_occupancy(np.zeros((1, 3)), nsamples=2)


def test_occupancy_and_signed_distance_on_the_host(monkeypatch):
    """compute_occupancy's ray construction and majority vote, compute_signed_distance's sign, with
    the two device calls replaced by restatements."""
    import mesh_restatement as MR

    monkeypatch.setattr(RC, "count_intersections",
                        lambda mesh, rays, tnear=0.0, tfar=np.inf, path=None:
                        R.count_intersections(mesh.vertices, mesh.triangles, rays, tnear, tfar))
    monkeypatch.setattr(M, "closest_points",
                        lambda mesh, points, transformation=None, path=None, r0=0.0:
                        MR.closest_points(mesh.vertices, mesh.triangles, points, transformation))
    scene = RC.RaycastingScene()
    scene.add_triangles(R.CUBE_V, R.CUBE_F)
    q = np.array([[0.5, 0.5, 0.5], [0.25, 0.5, 0.75], [1.5, 0.5, 0.5], [-0.25, -0.25, -0.25], [0.5, 0.5, 0.875]])
    for ns in (1, 3):
        occ = scene.compute_occupancy(q, ns)
        assert occ.dtype == np.float32
        np.testing.assert_array_equal(occ, [1, 1, 0, 0, 1])
        sd = scene.compute_signed_distance(q, ns)
        np.testing.assert_array_equal(sd, [-0.5, -0.25, 0.5, np.sqrt(3 * 0.0625), -0.125])


def test_create_rays_pinhole():
    eye, center, up = np.array([1.0, 2.0, 5.0]), np.array([1.0, 2.0, 0.0]), (0.0, 1.0, 0.0)
    for w, h in ((5, 3), (4, 2), (64, 64)):
        r = RC.RaycastingScene.create_rays_pinhole(90.0, center, eye, up, w, h)
        assert r.shape == (h, w, 6) and r.dtype == np.float64
        np.testing.assert_array_equal(r[..., :3], np.broadcast_to(eye, (h, w, 3)))
        d = r[..., 3:]
        f = 0.5 * w / np.tan(np.pi / 4)
        np.testing.assert_allclose(d[..., 2], -f, rtol=1e-15)  # the view axis is −z, length f
        # x to the right (+x of the world here), y down (−y of the world), pixel centres at +0.5
        np.testing.assert_allclose(d[..., 0], np.broadcast_to(np.arange(w) + 0.5 - 0.5 * w, (h, w)), atol=1e-13)
        np.testing.assert_allclose(d[..., 1], -np.broadcast_to((np.arange(h) + 0.5 - 0.5 * h)[:, None], (h, w)),
                                   atol=1e-13)
        # corner rays symmetric about the axis
        np.testing.assert_allclose(d[0, 0] * (-1, -1, 1), d[-1, -1], atol=1e-13)
        np.testing.assert_allclose(d[0, -1] * (-1, -1, 1), d[-1, 0], atol=1e-13)
    r = RC.RaycastingScene.create_rays_pinhole(60.0, center, eye, up, 5, 3)
    mid = r[1, 2, 3:]  # odd sizes: the central pixel's ray points at `center`
    np.testing.assert_allclose(np.cross(mid, center - eye), 0.0, atol=1e-13)
    assert mid @ (center - eye) > 0
    with pytest.raises(ValueError):
        RC.RaycastingScene.create_rays_pinhole(60.0, eye, eye, up, 4, 4)
    with pytest.raises(ValueError):
        RC.RaycastingScene.create_rays_pinhole(60.0, center, eye, up, 0, 4)


def test_base_scene_keeps_its_six_stubs():
    scene = M.RaycastingScene()
    scene.add_triangles(R.TRI_V, F1)
    for name in ("cast_rays", "test_occlusions", "count_intersections", "list_intersections",
                 "compute_signed_distance", "compute_occupancy"):
        with pytest.raises(NotImplementedError):
            getattr(scene, name)(np.zeros((1, 6)))
    assert "raycast" in __import__("m3d").__dict__


def test_ray_arguments_are_checked_before_any_device_call():
    mesh = M.TriangleMesh(R.TRI_V, F1)
    for bad in (np.zeros((4, 6), np.float32), np.zeros((4, 3)), np.zeros(()), np.zeros((4, 6), np.int64)):
        for fn in (RC.cast_rays, RC.count_intersections):
            with pytest.raises(ValueError, match="float64"):
                fn(mesh, bad)
    scene = RC.RaycastingScene()
    scene.add_triangles(mesh)
    with pytest.raises(ValueError, match="float64"):
        scene.cast_rays(np.zeros((4, 6), np.float32))
    with pytest.raises(ValueError, match="float64"):
        scene.count_intersections(np.zeros((4, 3)))


def test_c_symbols_answer_null_arguments():
    lib = _lib.load()
    assert lib.m3d_mesh_ray_auto_brute_max() >= 0
    out = (C.c_int64 * 2)()
    assert lib.m3d_mesh_ray_info(None, out) == _lib.M3D_ERR_INVALID
    assert lib.m3d_mesh_cast_rays(None, None, None, 0, 0.0, 1.0, 0, None, None, None, None) == _lib.M3D_ERR_INVALID
    assert lib.m3d_mesh_count_rays(None, None, None, 0, 0.0, 1.0, 0, None, None) == _lib.M3D_ERR_INVALID
