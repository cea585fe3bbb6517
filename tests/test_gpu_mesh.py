"""GPU parity of the point-to-mesh distance (m3d_mesh_closest through m3d.mesh and matcher) against
the numpy restatement of the contract in tests/mesh_restatement.py.

Every comparison is BIT FOR BIT on d2, triangle, point, uv and region: the brute-force path
(path=1), the grid path (path=2) and the restatement run the same elementwise IEEE fp64
operations in one fixed order on the same operands, so there is nothing to tolerate.  The tile of
the brute kernel (its LDS edge) is read from the library (m3d_mesh_brute_tile).
"""
import numpy as np
import pytest

import mesh_restatement as R
import m3d.mesh as M
from m3d import _lib, synth

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:The given NumPy array is not writable")]

REGION_CASES, ZERO_CASES, TRI_V, TRI_F = R.REGION_CASES, R.ZERO_CASES, R.TRI_V, R.TRI_F
FIELDS = ("d2", "triangle", "point", "uv", "region")
TILE = _lib.load().m3d_mesh_brute_tile()


def same_bits(got, ref, what=""):
    for k in FIELDS:
        g, r = np.asarray(got[k]), np.asarray(ref[k])
        assert g.dtype == r.dtype and g.shape == r.shape, (what, k, g.dtype, r.dtype, g.shape, r.shape)
        if g.tobytes() != r.tobytes():
            bad = np.nonzero((g != r).reshape(len(g), -1).any(axis=1))[0]
            raise AssertionError(f"{what}: {k} differs at {len(bad)} queries, first {bad[:5]}: "
                                 f"{g[bad[:3]]} != {r[bad[:3]]}")


def both_paths(mesh, q, ref, T=None, what=""):
    """path 1 and path 2 against the restatement's result; returns the grid path's info."""
    same_bits(M.closest_points(mesh, q, T, path="brute"), ref, what + " brute")
    assert mesh.grid_info()["rounds"] == 0
    same_bits(M.closest_points(mesh, q, T, path="grid"), ref, what + " grid")
    info = mesh.grid_info()
    assert info["rounds"] >= (1 if len(q) else 0)
    return info


def soup(F, seed):
    """F well-shaped random triangles in the unit cube (each its own three vertices)."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(0.0, 1.0, (F, 1, 3))
    v = (c + rng.uniform(-0.1, 0.1, (F, 3, 3))).reshape(-1, 3)
    return v, np.arange(3 * F).reshape(F, 3)


def test_one_triangle_regions_and_zero_distance():
    q = np.array([c[0] for c in REGION_CASES] + [c[0] for c in ZERO_CASES])
    ref = R.closest_points(TRI_V, TRI_F, q)
    np.testing.assert_array_equal(ref["region"], [c[1] for c in REGION_CASES] + [c[1] for c in ZERO_CASES])
    assert (ref["d2"][len(REGION_CASES):] == 0.0).all()
    both_paths(M.TriangleMesh(TRI_V, TRI_F), q, ref, what="one triangle")


def test_duplicate_and_tie():
    rng = np.random.default_rng(2)
    far = [np.array([[5.0, 5.0, k], [6.0, 5.0, k], [5.0, 6.0, k]]) for k in (1.0, 2.0, 3.0, 4.0)]
    q = np.vstack([rng.uniform(-0.5, 1.5, (40, 3)), [[0.25, 0.25, 0.5]]])
    # the same triangle at 0 and 5: index 0 wins
    v = np.vstack([TRI_V, far[0], far[1], far[2], far[3], TRI_V])
    f = np.arange(18).reshape(6, 3)
    ref = R.closest_points(v, f, q)
    assert (ref["triangle"] == 0).all()
    both_paths(M.TriangleMesh(v, f), q, ref, what="duplicate")
    # the copies swapped with a nearer triangle at 3: index 3 wins
    near = TRI_V + (0.0, 0.0, 0.25)
    qn = q[q[:, 2] > 0.25]
    v = np.vstack([far[0], far[1], far[2], near, far[3], TRI_V])
    ref = R.closest_points(v, f, qn)
    assert len(qn) > 5 and (ref["triangle"] == 3).all()
    both_paths(M.TriangleMesh(v, f), qn, ref, what="nearer at 3")


def test_two_triangles_sharing_an_edge():
    """A query above the shared edge: both triangles answer with the edge point.  The restatement
    reports both distances; the winner is decided by bit-equal d² and then the index, which is why
    no cross-implementation index check may be looser than that."""
    v = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [1.0, 1.0, 0.1]])
    f = np.array([[0, 1, 2], [1, 3, 2]])
    q = np.array([[0.5, 0.5, 0.75], [0.3, 0.7, 0.2], [0.61, 0.39, 1.3]])
    per = R.per_triangle_d2(v, f, q)
    print("d² per triangle above the shared edge:", per.tolist())
    ref = R.closest_points(v, f, q)
    for k in range(len(q)):
        assert ref["triangle"][k] == (0 if per[0, k] <= per[1, k] else 1)
        assert ref["d2"][k] == per[:, k].min()
    both_paths(M.TriangleMesh(v, f), q, ref, what="shared edge")


def test_skipped_triangles():
    q = np.array([[0.0, 0.0, 1.0], [0.5, 0.25, 1.0], [2.0, 2.0, 0.9]])
    line = np.array([[-1.0, 0.0, 1.0], [0.5, 0.25, 1.0], [2.0, 0.5, 1.0]])  # collinear, through a query
    dot = np.tile([[2.0, 2.0, 0.9]], (3, 1))                              # three equal vertices, on a query
    v = np.vstack([line, dot, TRI_V])
    f = np.arange(9).reshape(3, 3)
    np.testing.assert_array_equal(R.usable(v, f), [False, False, True])
    ref = R.closest_points(v, f, q)
    assert (ref["triangle"] == 2).all() and (ref["d2"] > 0).all()
    both_paths(M.TriangleMesh(v, f), q, ref, what="skipped")
    bad = M.TriangleMesh(v[:6], f[:2])
    for path in ("brute", "grid", "auto"):
        with pytest.raises(ValueError, match="no usable triangle"):
            M.closest_points(bad, q, path=path)
    with pytest.raises(ValueError, match="no usable triangle"):
        M.closest_points(M.TriangleMesh(v, np.zeros((0, 3), np.int32)), q)


def test_bad_index_is_an_error_code_not_a_read():
    import ctypes as C

    from m3d.core import context, ptr, to_device

    ctx = context()
    v = to_device(TRI_V)
    for tri in ([[0, 1, 3]], [[0, -1, 2]], [[0, 1, 2], [2, 1, 2 ** 31 - 1]]):
        t = to_device(np.array(tri, np.int32), "int32", (3,))
        h = C.c_void_p()
        rc = ctx.lib.m3d_mesh_create(ctx.h, ptr(v), 3, ptr(t), len(tri), C.byref(h))
        assert rc == _lib.M3D_ERR_INVALID and not h.value


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_query_counts(n):
    v, f = soup(40, 5)
    q = np.random.default_rng(n).uniform(-0.5, 1.5, (n, 3))
    ref = R.closest_points(v, f, q)
    both_paths(M.TriangleMesh(v, f), q, ref, what=f"n={n}")


@pytest.mark.parametrize("F", [1, 2, TILE - 1, TILE, TILE + 1])
def test_triangle_counts_across_the_brute_tile(F):
    assert TILE == _lib.MESH_BRUTE_TILE == 256
    v, f = soup(F, 11)
    q = np.random.default_rng(F).uniform(-0.2, 1.2, (300, 3))
    ref = R.closest_points(v, f, q)
    if F > 1:  # the last triangle of the mesh (past the tile edge at TILE + 1) wins somewhere
        q[:3] = v[f[F - 1]].mean(axis=0) + [[0, 0, 0], [1e-3, 0, 0], [0, 1e-3, 0]]
        ref = R.closest_points(v, f, q)
        assert (ref["triangle"][:3] == F - 1).any()
    both_paths(M.TriangleMesh(v, f), q, ref, what=f"F={F}")


@pytest.fixture(scope="module")
def closed_mesh():
    """m3d.synth's closed surface at a coarse setting (12 rings × 16 segments: 384 triangles) and
    2,000 seeded queries: a quarter within 1 % of the surface, a quarter inside, a quarter in the
    bounding box, the rest 10× and 1000× the box away; 64 of them sit exactly on vertices.  The
    restatement's answer is computed once."""
    v, f = synth.surface_mesh(12, 16, seed=4)
    rng = np.random.default_rng(9)
    lo, hi = v.min(axis=0), v.max(axis=0)
    ext = float((hi - lo).max())
    a, b, c = (v[f[:, k]] for k in range(3))
    t = rng.integers(0, len(f), 500)
    w = rng.dirichlet((1.0, 1.0, 1.0), 500)
    on = w[:, :1] * a[t] + w[:, 1:2] * b[t] + w[:, 2:] * c[t]
    near = on + rng.uniform(-0.01, 0.01, (500, 3)) * ext
    inside = v.mean(axis=0) + 0.5 * (v[rng.integers(0, len(v), 500)] - v.mean(axis=0)) * rng.uniform(0, 1, (500, 1))
    box = rng.uniform(lo, hi, (500, 3))
    d = rng.standard_normal((500, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    away = v.mean(axis=0) + d * ext * np.where(np.arange(500) < 250, 10.0, 1000.0)[:, None]
    q = np.vstack([near, inside, box, away])
    q[rng.choice(1500, 64, replace=False)] = v[rng.choice(len(v), 64, replace=False)]
    assert len(f) == 384 and q.shape == (2000, 3)
    return v, f, q, R.closest_points(v, f, q)


def test_closed_mesh_ladder_and_clamping(closed_mesh):
    v, f, q, ref = closed_mesh
    assert (ref["d2"] == 0.0).sum() >= 64 and set(np.unique(ref["region"])) == set(range(7))
    mesh = M.TriangleMesh(v, f)
    info = both_paths(mesh, q, ref, what="closed mesh")
    assert 0 < info["references"] <= 16 * len(f) and info["cells"] > 1
    cell = float((v.max(axis=0) - v.min(axis=0)).max()) / round(info["cells"] ** (1 / 3))  # ≈, the order matters only
    same_bits(M.closest_points(mesh, q, path="grid", r0=0.1 * cell), ref, "closed mesh r0 = cell / 10")
    assert mesh.grid_info()["rounds"] >= 2
    same_bits(M.closest_points(mesh, q), ref, "closed mesh auto")


def test_huge_triangle_and_tiny_ones():
    """One triangle spanning the whole (flat) box plus 500 tiny ones in a corner: at the first cell
    size the huge one alone would be referenced from more than 16·F cells, so the cell doubles."""
    rng = np.random.default_rng(13)
    huge = np.array([[0.0, 0.0, 0.0], [100.0, 0.0, 0.0], [0.0, 100.0, 0.01]])
    c = rng.uniform(0.0, 1.0, (500, 1, 3)) * (1.0, 1.0, 0.01)
    tiny = (c + rng.uniform(-0.01, 0.01, (500, 3, 3)) * (1.0, 1.0, 0.1)).reshape(-1, 3)
    v = np.vstack([huge, tiny])
    f = np.arange(len(v)).reshape(-1, 3)
    F = len(f)
    q = np.vstack([rng.uniform(-0.5, 1.5, (300, 3)) * (1.0, 1.0, 0.05), rng.uniform(0.0, 100.0, (300, 3)) * (1, 1, 0.1)])
    ref = R.closest_points(v, f, q)
    assert 0 < (ref["triangle"] == 0).sum() < len(q)
    info = both_paths(M.TriangleMesh(v, f), q, ref, what="huge + tiny")
    assert info["references"] <= 16 * F and info["doublings"] >= 1, info


def test_with_transformation(closed_mesh):
    v, f, q, _ = closed_mesh
    q = q[::7]
    T = synth.random_rigid(5, center=v.mean(axis=0), rot_range=0.4, trans_range=0.3)
    ref = R.closest_points(v, f, R.q64_of(T, q))
    same_bits(R.closest_points(v, f, q, T), ref, "restatement with T")
    both_paths(M.TriangleMesh(v, f), q, ref, T=T, what="with T")


def test_repeatable(closed_mesh):
    v, f, q, ref = closed_mesh
    q = q[::5]
    m1, m2 = M.TriangleMesh(v, f), M.TriangleMesh(v.copy(), f.copy())
    first = M.closest_points(m1, q, path="grid")
    same_bits(M.closest_points(m1, q, path="grid"), first, "second call")
    same_bits(M.closest_points(m2, q, path="grid"), first, "second mesh")
    same_bits(first, {k: ref[k][::5] for k in FIELDS}, "against the restatement")


def test_scene_and_matcher_api():
    from matcher import compute_point_cloud_distance, compute_point_cloud_to_mesh_distance
    from m3d.types import PointCloud

    v0, f0 = soup(30, 21)
    v1, f1 = soup(20, 22)
    v1 = v1 + (2.0, 0.0, 0.0)
    scene = M.RaycastingScene()
    assert (scene.add_triangles(M.TriangleMesh(v0, f0)), scene.add_triangles(v1, f1)) == (0, 1)
    q = np.random.default_rng(3).uniform(-0.2, 3.2, (400, 3)) * (1.0, 0.4, 0.4)
    out = scene.compute_closest_points(q)
    r0, r1 = R.closest_points(v0, f0, q), R.closest_points(v1, f1, q)
    first = r0["d2"] <= r1["d2"]
    assert 50 < first.sum() < 350
    np.testing.assert_array_equal(out["geometry_ids"], np.where(first, 0, 1))
    np.testing.assert_array_equal(out["primitive_ids"], np.where(first, r0["triangle"], r1["triangle"]))
    assert out["points"].tobytes() == np.where(first[:, None], r0["point"], r1["point"]).tobytes()
    assert out["primitive_uvs"].tobytes() == np.where(first[:, None], r0["uv"], r1["uv"]).tobytes()
    n0, n1 = M.TriangleMesh(v0, f0).triangle_normals(), M.TriangleMesh(v1, f1).triangle_normals()
    np.testing.assert_array_equal(out["primitive_normals"],
                                  np.where(first[:, None], n0[r0["triangle"]], n1[r1["triangle"]]))
    np.testing.assert_allclose(np.linalg.norm(out["primitive_normals"], axis=1), 1.0, atol=1e-15)
    d = scene.compute_distance(q)
    assert d.tobytes() == np.sqrt(np.where(first, r0["d2"], r1["d2"])).tobytes()

    # the reason for the feature: scan points above the middle of a flat square made of two large
    # triangles are their height away from the SURFACE, and much farther from its four vertices
    sq = np.array([[0.0, 0.0, 0.0], [8.0, 0.0, 0.0], [8.0, 8.0, 0.0], [0.0, 8.0, 0.0]])
    mesh = M.TriangleMesh(sq, [[0, 1, 2], [0, 2, 3]])
    scan = np.array([[4.0, 4.0, 0.5], [3.0, 5.0, 0.25], [5.0, 2.0, 1.0]])
    np.testing.assert_array_equal(compute_point_cloud_to_mesh_distance(scan, mesh), scan[:, 2])
    np.testing.assert_array_equal(compute_point_cloud_to_mesh_distance(PointCloud(scan), (sq, mesh.triangles)),
                                  scan[:, 2])
    to_vertices = compute_point_cloud_distance(scan, sq)
    np.testing.assert_allclose(to_vertices, np.sqrt(((scan[:, None] - sq[None]) ** 2).sum(axis=2)).min(axis=1),
                               rtol=1e-15)
    assert (to_vertices > 3.0 * scan[:, 2]).all()  # 5.68, 4.25, 3.74 against heights 0.5, 0.25, 1
    T = np.eye(4)
    T[2, 3] = 1.0
    np.testing.assert_array_equal(compute_point_cloud_to_mesh_distance(scan, mesh, T), scan[:, 2] + 1.0)
