"""Surface sampling and minimum-distance thinning without a device: the numpy restatement of the two
contracts (tests/mesh_sample_restatement.py) against their own statements — the distribution, the
zero-weight triangles, the boundaries of the cumulative table, the fold, the thinning's definition
against its synchronous rounds — and the Python layer above the device calls
(``sample_points_poisson_disk``, ``Ply.from_mesh``, ``register_to_mesh``) with those calls replaced
by the restatement.
"""
import importlib

import numpy as np
import pytest

import mesh_sample_restatement as R
import m3d.mesh as M
from m3d import prep
from m3d.types import PointCloud, RegistrationResult
from ply import Ply

U64 = np.uint64

# three well-shaped triangles in the plane z = 0, areas 0.5, 2, 1
GOOD_V = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0],
                   [2, 0, 0], [4, 0, 0], [2, 2, 0],
                   [5, 0, 0], [6, 0, 0], [5, 2, 0]], np.float64)


def x0_for_t(t: int, W: int) -> int:
    """The smallest x0 whose draw is t = floor(x0·W / 2^64): x0·W lies in [t·2^64, t·2^64 + W)."""
    return -((-t << 64) // W)


def with_bad(kind: str, where: int):
    """GOOD_V's three triangles with one zero-weight triangle at position `where` (0, 1 or 3)."""
    bad = {"zero_area": np.array([[0, 0, 1], [1, 1, 2], [2, 2, 3]], np.float64),        # collinear
           "nan": np.array([[0, 0, 1], [np.nan, 0, 1], [0, 1, 1]], np.float64),
           "tiny": np.array([[0, 0, 1], [1, 0, 1], [0, 1, 1]], np.float64) * 2.0 ** -40}[kind]
    tris = [GOOD_V[0:3], GOOD_V[3:6], GOOD_V[6:9]]
    tris.insert(where, bad)
    v = np.vstack(tris)
    return v, np.arange(12).reshape(4, 3), where


# --------------------------------------------------------------------------------- distribution
def test_two_triangles_share_and_barycentric_means():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 2, 0], [2, 0, 0], [5, 0, 0], [2, 2, 0]], np.float64)  # areas 1 : 3
    f = np.arange(6).reshape(2, 3)
    n = 40000
    s = R.sample(v, f, n, seed=1)
    share = float((s["triangle"] == 0).mean())
    print("share of the small triangle", share)
    assert abs(share - 0.25) <= 0.01  # 4σ, σ = sqrt(0.25·0.75/40000) = 0.0022
    u, w = s["uv"][:, 0], s["uv"][:, 1]
    means = [float((1.0 - u - w).mean()), float(u.mean()), float(w.mean())]
    print("barycentric means", means)
    for m in means:
        assert abs(m - 1.0 / 3.0) <= 0.005  # 4σ, σ = sqrt(1/18/40000) = 0.0012


@pytest.mark.parametrize("kind", ["zero_area", "nan", "tiny"])
@pytest.mark.parametrize("where", [0, 1, 3])
def test_zero_weight_triangles_never_win(kind, where):
    v, f, bad = with_bad(kind, where)
    w, cum, W = R.weights(v, f)
    assert w[bad] == 0 and (np.delete(w, bad) > 0).all()
    assert int(w.max()) >> 31 == 1  # the largest triangle lands in [2^31, 2^32)
    s = R.sample(v, f, 20000, seed=3)
    assert not (s["triangle"] == bad).any()
    assert set(np.unique(s["triangle"])) == set(range(4)) - {bad}
    # the two ends of the stream's range
    ends = R.triangle_of_x0(cum, np.array([0, 2 ** 64 - 1], U64))
    good = [k for k in range(4) if k != bad]
    assert list(ends) == [good[0], good[-1]]
    assert np.isfinite(s["point"]).all() and np.isfinite(s["normal"]).all()


def test_draws_on_the_boundaries_of_the_cumulative_table():
    # triangles 0 2 3 5 have weight, 1 and 4 have none (zero area, NaN)
    tris = [GOOD_V[0:3], np.zeros((3, 3)), GOOD_V[3:6], GOOD_V[6:9],
            np.array([[np.nan, 0, 0], [1, 0, 0], [0, 1, 0]]), GOOD_V[0:3] + [0, 0, 2.0]]
    v, f = np.vstack(tris), np.arange(18).reshape(6, 3)
    w, cum, W = R.weights(v, f)
    assert list(w > 0) == [True, False, True, True, False, True]
    nonzero = [0, 2, 3, 5]
    for k, t in enumerate(nonzero):
        below = x0_for_t(int(cum[t]) - 1, W)
        assert int(R.umul64hi(np.array([below], U64), W)[0]) == int(cum[t]) - 1
        assert int(R.triangle_of_x0(cum, np.array([below], U64))[0]) == t
        if k + 1 < len(nonzero):
            at = x0_for_t(int(cum[t]), W)
            assert int(R.umul64hi(np.array([at], U64), W)[0]) == int(cum[t])
            assert int(R.triangle_of_x0(cum, np.array([at], U64))[0]) == nonzero[k + 1]
    assert int(R.triangle_of_x0(cum, np.array([0], U64))[0]) == 0
    # the 64 × 64 → high 64 product against Python's integers
    xs = R.splitmix64(np.arange(1000, dtype=U64))
    assert [int(t) for t in R.umul64hi(xs, W)] == [(int(x) * W) >> 64 for x in xs]


def test_the_fold_lands_inside_the_triangle():
    u, w = R.fold(np.array([0.75, 0.25, 1.0, 0.5]), np.array([0.75, 0.25, 0.5, 0.5]))
    np.testing.assert_array_equal(u, [0.25, 0.25, 0.0, 0.5])
    np.testing.assert_array_equal(w, [0.25, 0.25, 0.5, 0.5])
    v, f = GOOD_V[3:6], np.arange(3).reshape(1, 3)
    n = 4000
    base = R.sample_base(5, np.arange(n, dtype=U64))
    with np.errstate(over="ignore"):
        u0 = (R.splitmix64(base + U64(1)) >> U64(11)).astype(np.float64) * 2.0 ** -53
        w0 = (R.splitmix64(base + U64(2)) >> U64(11)).astype(np.float64) * 2.0 ** -53
    folded = u0 + w0 > 1.0
    assert 0.4 < folded.mean() < 0.6
    s = R.sample(v, f, n, seed=5)
    uu, ww = s["uv"][:, 0], s["uv"][:, 1]
    np.testing.assert_array_equal(uu[folded], 1.0 - u0[folded])
    np.testing.assert_array_equal(ww[~folded], w0[~folded])
    assert (uu >= 0).all() and (ww >= 0).all() and (uu + ww <= 1.0).all()
    # inside the triangle (2,0) (4,0) (2,2): x ≥ 2, y ≥ 0, (x − 2) + y ≤ 2, up to rounding
    p = s["point"]
    assert (p[:, 0] >= 2.0).all() and (p[:, 1] >= 0.0).all() and ((p[:, 0] - 2.0) + p[:, 1] <= 2.0 + 1e-12).all()
    np.testing.assert_array_equal(s["normal"], np.broadcast_to([0.0, 0.0, 1.0], (n, 3)))


def test_a_mesh_without_a_usable_triangle():
    with pytest.raises(ValueError):
        R.sample(np.zeros((3, 3)), np.arange(3).reshape(1, 3), 4)
    with pytest.raises(ValueError):
        R.sample(np.full((3, 3), np.nan), np.arange(3).reshape(1, 3), 4)


# --------------------------------------------------------------------------------- thinning
def by_rank(points, seed):
    """`points` (in the order lowest rank first) placed at the indices whose keys have that order."""
    out = np.empty_like(points)
    out[R.rank_order(seed, len(points))] = points
    return out


def test_rounds_and_sequential_greedy_agree():
    p = np.random.default_rng(2).uniform(0.0, 1.0, (3000, 3))
    for seed in (0, 7):
        g = R.thin_greedy(p, 0.08, seed)
        d, rounds = R.thin_rounds(p, 0.08, seed)
        assert (d != 0).all() and 1 < rounds <= 32
        np.testing.assert_array_equal(d > 0, g)
        np.testing.assert_array_equal(R.thin_min_distance(p, 0.08, seed), np.flatnonzero(g))
    assert 0 < g.sum() < len(p)


def test_chain_keeps_the_two_ends():
    seed = 4
    p = by_rank(np.array([[0.0, 0, 0], [0.9, 0, 0], [1.8, 0, 0]]), seed)  # a < b < c, ab < r, bc < r, ac ≥ r
    order = R.rank_order(seed, 3)
    kept = R.thin_greedy(p, 1.0, seed)
    assert kept[order[0]] and not kept[order[1]] and kept[order[2]]
    d, rounds = R.thin_rounds(p, 1.0, seed)
    assert d[order[0]] == 1 and d[order[1]] == -2 and d[order[2]] == 3 and rounds == 3


def test_distance_exactly_the_radius_keeps_both():
    p = np.array([[0.0, 0, 0], [3.0, 4.0, 0]])
    assert R.thin_greedy(p, 5.0, 0).all()
    assert R.thin_greedy(p, np.nextafter(5.0, 6.0), 0).sum() == 1


def test_of_two_equal_points_the_lower_rank_is_kept():
    for seed in (0, 1, 2, 3):
        order = R.rank_order(seed, 2)
        kept = R.thin_greedy(np.ones((2, 3)), 0.5, seed)
        assert kept[order[0]] and not kept[order[1]]


def test_a_point_that_is_not_finite_is_dropped_and_blocks_nobody():
    p = np.array([[0.0, 0, 0], [np.nan, 0, 0], [0.1, 0, 0], [np.inf, 0, 0]])
    d, _ = R.thin_rounds(p, 1.0, 0)
    assert d[1] == -1 and d[3] == -1 and (d[[0, 2]] > 0).sum() == 1


# --------------------------------------------------------------------------------- the Python layer
@pytest.fixture
def host_calls(monkeypatch):
    """The two device calls replaced by the restatement."""
    monkeypatch.setattr(M, "sample_points", lambda mesh, n, seed=0: R.sample(mesh.vertices, mesh.triangles, n, seed))
    monkeypatch.setattr(prep, "thin_min_distance",
                        lambda points, radius, seed=0, with_details=False: R.thin_min_distance(points, radius, seed))


def square():
    return M.TriangleMesh([[0, 0, 0], [2, 0, 0], [2, 2, 0], [0, 2, 0]], [[0, 1, 2], [0, 2, 3]])


def min_distance(p):
    d = np.linalg.norm(p[:, None, :] - p[None, :, :], axis=2)
    return float(d[np.triu_indices(len(p), 1)].min())


def test_uniform_samples_through_the_mesh(host_calls):
    m = square()
    assert m.get_surface_area() == 4.0
    pc, det = m.sample_points_uniformly(500, seed=2, with_details=True)
    assert isinstance(pc, PointCloud) and pc.points.shape == (500, 3) and pc.points.dtype == np.float64
    assert pc.has_normals() and (pc.normals == [0.0, 0.0, 1.0]).all()
    assert det["triangle"].dtype == np.int32 and det["uv"].shape == (500, 2)
    assert not m.sample_points_uniformly(10, use_triangle_normal=False).has_normals()
    assert len(m.sample_points_uniformly(0).points) == 0
    # sample k does not depend on the count
    np.testing.assert_array_equal(m.sample_points_uniformly(100, seed=2).points, pc.points[:100])
    with pytest.raises(ValueError):
        m.sample_points_uniformly(-1)
    with pytest.raises(ValueError):
        M.TriangleMesh(np.zeros((3, 3)), [[0, 1, 2]]).sample_points_uniformly(5)


def test_poisson_disk_by_count_and_by_radius(host_calls):
    m = square()
    pc, det = m.sample_points_poisson_disk(60, init_factor=5, seed=1, with_details=True)
    assert pc.points.shape == (60, 3) and pc.has_normals()
    assert det["kept"] >= 60 and len(det["indices"]) == 60 and det["indices"].dtype == np.int64
    assert min_distance(pc.points) >= det["radius"]
    # the radius used is the largest tried one that kept enough
    assert det["radius"] == max(r for r, k in det["tried"] if k >= 60)
    assert len(det["tried"]) <= 1 + 24 + 6
    # every returned point is one of the uniform samples
    base = m.sample_points_uniformly(300, seed=1)
    np.testing.assert_array_equal(pc.points, base.points[det["indices"]])
    pr, dr = m.sample_points_poisson_disk(radius=0.3, seed=1, with_details=True)
    assert dr["radius"] == 0.3 and len(pr.points) == dr["kept"] > 0
    assert min_distance(pr.points) >= 0.3
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            m.sample_points_poisson_disk(radius=bad)
    with pytest.raises(ValueError):
        m.sample_points_poisson_disk()
    with pytest.raises(ValueError):
        m.sample_points_poisson_disk(0)


def test_thin_min_distance_refuses_a_bad_radius_before_any_device_call():
    p = np.zeros((4, 3))
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            prep.thin_min_distance(p, bad)
    idx = prep.thin_min_distance(np.zeros((0, 3)), 1.0)
    assert idx.dtype == np.int64 and len(idx) == 0


def test_point_cloud_thin_min_distance(host_calls):
    p = np.random.default_rng(3).uniform(0, 1, (400, 3))
    pc, ind = PointCloud(p, p).thin_min_distance(0.2, seed=5)
    np.testing.assert_array_equal(ind, R.thin_min_distance(p, 0.2, 5))
    assert ind.dtype == np.int64 and (np.diff(ind) > 0).all()
    np.testing.assert_array_equal(pc.points, p[ind])
    np.testing.assert_array_equal(pc.normals, p[ind])


def test_ply_from_mesh(host_calls, monkeypatch, tmp_path):
    import ply.ply as P

    seen = {}

    def fake_preprocess(self, voxel_size, *options):
        seen["voxel"], seen["options"] = voxel_size, options
        self.pcd_down, self.pcd_fpfh = self.pcd, None

    monkeypatch.setattr(Ply, "_preprocess", fake_preprocess)
    m = square()
    a = Ply.from_mesh(m, voxel_size=0.5, number_of_points=777, seed=3, keep_cluster={"eps": 1.0, "min_points": 2})
    assert a.pcd.points.shape == (777, 3) and a.pcd.has_normals() and a.voxel_size == 0.5 and a.path is None
    assert seen["voxel"] == 0.5 and seen["options"] == (None, None, {"eps": 1.0, "min_points": 2}, None)
    np.testing.assert_array_equal(a.pcd.points, R.sample(m.vertices, m.triangles, 777, 3)["point"])
    # the default count: ceil(16·area / voxel²) clamped to [10,000, 5,000,000]
    assert P.mesh_sample_count(4.0, 0.5) == 10_000
    assert P.mesh_sample_count(4.0, 0.05) == 25_600
    assert P.mesh_sample_count(4.0, 0.05 + 1e-9) == 25_600 and P.mesh_sample_count(4.0 + 1e-6, 0.05) == 25_601
    assert P.mesh_sample_count(1e9, 0.01) == 5_000_000
    assert len(Ply.from_mesh(m, voxel_size=0.3).pcd.points) == 10_000
    assert len(Ply.from_mesh((m.vertices, m.triangles), number_of_points=5).pcd.points) == 5
    with pytest.raises(ValueError):
        Ply.from_mesh(m, voxel_size=0.0)
    with pytest.raises(ValueError):
        Ply.from_mesh(M.TriangleMesh(np.zeros((3, 3)), [[0, 1, 2]]), number_of_points=5)
    # Ply(path) itself keeps refusing anything but a .ply
    stl = tmp_path / "x.stl"
    stl.write_bytes(b"solid x\nendsolid x\n")
    with pytest.raises(TypeError):
        Ply(stl)


def test_register_to_mesh_composes_the_two_stages(host_calls, monkeypatch):
    import matcher

    reg = importlib.import_module("matcher.register")
    mesh_icp = importlib.import_module("matcher.mesh_icp")
    monkeypatch.setattr(Ply, "_preprocess", lambda self, *a: setattr(self, "pcd_down", self.pcd))
    calls = {}
    T1 = np.eye(4)
    T1[0, 3] = 0.25

    def fake_register(source, target, voxel_size=None, **kw):
        calls["register"] = (source, target, voxel_size, kw)
        return RegistrationResult(T1, 0.5, 0.1)

    def fake_refine(src, mesh, init, voxel_size, kernel=None):
        calls["refine"] = (src, mesh, np.array(init), voxel_size, kernel)
        return RegistrationResult(np.array(init), 1.0, 0.0)

    monkeypatch.setattr(reg, "register", fake_register)
    monkeypatch.setattr(mesh_icp, "refine_registration_to_mesh", fake_refine)
    m = square()
    src = Ply.from_arrays(np.zeros((5, 3)), voxel_size=0.4)
    out = matcher.register_to_mesh(src, m, coarse="fgr", number_of_points=321, seed=9, kernel="K", iteration=7)
    s, target, v, kw = calls["register"]
    assert s is src and v == 0.4 and kw == {"refine": False, "coarse": "fgr", "iteration": 7}
    assert isinstance(target, Ply) and len(target.pcd.points) == 321 and target.voxel_size == 0.4
    np.testing.assert_array_equal(target.pcd.points, R.sample(m.vertices, m.triangles, 321, 9)["point"])
    rs, rm, rT, rv, rk = calls["refine"]
    assert rs is src and rm is m and rv == 0.4 and rk == "K"
    np.testing.assert_array_equal(rT, T1)
    np.testing.assert_array_equal(out.transformation, T1)
    assert matcher.register_to_mesh(src, m, voxel_size=0.2) is not None and calls["register"][2] == 0.2
    with pytest.raises(TypeError):
        matcher.register_to_mesh(src, m, refine=False)
    assert "register_to_mesh" in matcher.__all__
