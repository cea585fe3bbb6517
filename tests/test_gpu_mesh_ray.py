"""GPU parity of ray casting (m3d_mesh_cast_rays / m3d_mesh_count_rays through m3d.raycast) against
the numpy restatement of the contract in tests/mesh_ray_restatement.py.

Every comparison is BIT FOR BIT on t_hit, triangle, uv and count: the brute-force path (path=1), the
grid walk (path=2) and the restatement run the same elementwise IEEE fp64 operations in one fixed
order on the same operands, so there is nothing to tolerate.  After a grid call m3d_mesh_ray_info
must report path 2 and — everywhere but the far-origin case — zero rays on the whole-grid fallback:
a grid path that quietly scans everything does not pass.
"""
import numpy as np
import pytest

import mesh_ray_restatement as R
import m3d.raycast as RC
from m3d import _lib, synth
from m3d.mesh import TriangleMesh

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:The given NumPy array is not writable")]

TILE = _lib.load().m3d_mesh_brute_tile()
F1 = np.array([[0, 1, 2]])
INF = np.inf


def same_bits(got, ref, what):
    for k in ("t_hit", "triangle", "uv"):
        g, r = np.asarray(got[k]), np.asarray(ref[k])
        assert g.dtype == r.dtype and g.shape == r.shape, (what, k, g.dtype, r.dtype, g.shape, r.shape)
        if g.tobytes() != r.tobytes():
            n = int(np.prod(ref["triangle"].shape))
            bad = np.nonzero((g.reshape(n, -1).view(np.uint8) != r.reshape(n, -1).view(np.uint8)).any(axis=1))[0]
            raise AssertionError(f"{what}: {k} differs at {len(bad)} rays, first {bad[:5]}: "
                                 f"{g.reshape(n, -1)[bad[:3]]} != {r.reshape(n, -1)[bad[:3]]}")


def same_count(got, ref, what):
    assert got.dtype == np.int32 and got.shape == ref.shape, (what, got.dtype, got.shape)
    if got.tobytes() != ref.tobytes():
        bad = np.nonzero(got.reshape(-1) != ref.reshape(-1))[0]
        raise AssertionError(f"{what}: count differs at {len(bad)} rays, first {bad[:5]}: "
                             f"{got.reshape(-1)[bad[:5]]} != {ref.reshape(-1)[bad[:5]]}")


def both_paths(mesh, rays, tnear=0.0, tfar=INF, what="", fallback=0):
    """First hit and count through path 1 and path 2 against the restatement; `fallback`: the
    whole-grid rays the grid calls must report (None: any)."""
    ref, ref_cnt = R.cast_and_count(mesh.vertices, mesh.triangles, rays, tnear, tfar)
    same_bits(RC.cast_rays(mesh, rays, tnear, tfar, path="brute"), ref, what + " brute")
    assert RC.ray_info(mesh) == {"path": "brute", "fallback": 0}
    same_count(RC.count_intersections(mesh, rays, tnear, tfar, path="brute"), ref_cnt, what + " brute")
    assert RC.ray_info(mesh) == {"path": "brute", "fallback": 0}
    for mode in ("first", "count"):
        if mode == "first":
            same_bits(RC.cast_rays(mesh, rays, tnear, tfar, path="grid"), ref, what + " grid")
        else:
            same_count(RC.count_intersections(mesh, rays, tnear, tfar, path="grid"), ref_cnt, what + " grid")
        info = RC.ray_info(mesh)
        assert info["path"] == "grid", (what, mode, info)
        if fallback is not None:
            assert info["fallback"] == fallback, (what, mode, info)
    return ref, ref_cnt


def soup(F, seed):
    """F well-shaped random triangles in the unit cube (each its own three vertices)."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(0.0, 1.0, (F, 1, 3))
    v = (c + rng.uniform(-0.1, 0.1, (F, 3, 3))).reshape(-1, 3)
    return v, np.arange(3 * F).reshape(F, 3)


def aimed_rays(rng, n, lo=-0.1, hi=1.1, radius=(1.5, 3.0)):
    """n rays from outside the box [lo, hi]³ aimed at random points inside it."""
    o = rng.standard_normal((n, 3))
    o = 0.5 * (lo + hi) + o / np.linalg.norm(o, axis=1, keepdims=True) * rng.uniform(*radius, (n, 1)) * (hi - lo)
    return np.hstack([o, rng.uniform(lo, hi, (n, 3)) - o])


def test_one_triangle_truth_table():
    table = R.truth_table()
    tris = []
    for case in table:
        if not any(np.array_equal(case[1], t) for t in tris):
            tris.append(case[1])
    for v in tris:
        mesh = TriangleMesh(v, F1)
        for tn, tf in sorted({(c[3], c[4]) for c in table if np.array_equal(c[1], v)}):
            cases = [c for c in table if np.array_equal(c[1], v) and (c[3], c[4]) == (tn, tf)]
            rays = np.array([c[2] for c in cases])
            ref, cnt = both_paths(mesh, rays, tn, tf, what=f"table [{tn}, {tf}]")
            np.testing.assert_array_equal(cnt, [int(c[5]) for c in cases])
            np.testing.assert_array_equal(ref["t_hit"], [c[6] if c[5] else INF for c in cases])


def test_ties_and_skipped_triangles():
    T = R.TRI_V
    far = [T + (5.0, 5.0, float(k)) for k in (1, 2, 3, 4)]
    rng = np.random.default_rng(2)
    rays = np.hstack([rng.uniform(0.05, 0.45, (40, 2)), np.full((40, 1), 1.0), rng.uniform(-0.05, 0.05, (40, 2)),
                      np.full((40, 1), -1.0)])
    # the same triangle at indices 0 and 5: 0 wins, both count
    v = np.vstack([T, far[0], far[1], far[2], far[3], T])
    f = np.arange(18).reshape(6, 3)
    ref, cnt = both_paths(TriangleMesh(v, f), rays, what="duplicate")
    assert (ref["triangle"] == 0).all() and (cnt == 2).all()
    # two different triangles with bit-equal t (the same plane, overlapping, other vertices), a
    # zero-area and a NaN-vertex triangle between them: the lower index wins
    other = np.array([(-1.0, -1.0, 0.0), (2.0, -1.0, 0.0), (-1.0, 2.0, 0.0)])
    line = np.array([(0.0, 0.0, 0.5), (0.25, 0.25, 0.5), (0.5, 0.5, 0.5)])
    nanv = np.array([(0.0, 0.0, 0.5), (1.0, 0.0, np.nan), (0.0, 1.0, 0.5)])
    straight = rays.copy()
    straight[:, 3:5] = 0.0
    v = np.vstack([far[0], other, line, nanv, T, far[1]])
    ref, cnt = both_paths(TriangleMesh(v, f), straight, what="equal t")
    assert (ref["triangle"] == 1).all() and (ref["t_hit"] == 1.0).all() and (cnt == 2).all()
    v = np.vstack([far[0], T, line, nanv, other, far[1]])
    ref, cnt = both_paths(TriangleMesh(v, f), straight, what="equal t swapped")
    assert (ref["triangle"] == 1).all() and (cnt == 2).all()
    with pytest.raises(ValueError, match="no usable triangle"):
        RC.cast_rays(TriangleMesh(np.vstack([line, nanv]), f[:2]), rays)
    with pytest.raises(ValueError, match="no usable triangle"):
        RC.count_intersections(TriangleMesh(np.vstack([line, nanv]), f[:2]), rays, path="grid")


@pytest.mark.parametrize("F", [TILE - 1, TILE, TILE + 1])
def test_tile_and_wave_edges(F):
    v, f = soup(F, 10 + F)
    mesh = TriangleMesh(v, f)
    rng = np.random.default_rng(F)
    for n in (1, 63, 64, 65, 257):
        rays = aimed_rays(rng, n)
        ref, cnt = both_paths(mesh, rays, what=f"F {F} n {n}")
        assert n < 60 or ((cnt > 0).any() and (cnt == 0).any())
    out = RC.cast_rays(mesh, np.zeros((0, 6)), path="grid")
    assert out["t_hit"].shape == (0,) and out["uv"].shape == (0, 2)
    assert RC.count_intersections(mesh, np.zeros((3, 0, 6))).shape == (3, 0)


def walk_rays():
    """4,096 rays around and inside the box of the walk's soup ([−0.1, 1.1]³): every kind of start
    and direction the walk treats differently."""
    rng = np.random.default_rng(77)
    unit = lambda x: x / np.linalg.norm(x, axis=1, keepdims=True)
    parts = []
    parts.append(np.hstack([rng.uniform(0.0, 1.0, (1024, 3)), unit(rng.standard_normal((1024, 3)))]))  # start inside
    a = aimed_rays(rng, 1024)                                                                           # from outside
    a[:, 3:] = unit(a[:, 3:])
    parts.append(a)
    away = aimed_rays(rng, 512)                                                                         # miss the box
    away[:, 3:] = -unit(away[:, 3:])
    parts.append(away)
    beside = np.hstack([rng.uniform(1.3, 2.0, (256, 1)), rng.uniform(0, 1, (256, 2)), np.zeros((256, 1)),
                        unit(rng.standard_normal((256, 2)))])                                           # pass beside it
    parts.append(beside)
    one = np.hstack([rng.uniform(-0.5, 1.5, (640, 3)), unit(rng.standard_normal((640, 3)))])            # one zero
    one[np.arange(640), 3 + rng.integers(0, 3, 640)] = 0.0
    parts.append(one)
    two = np.zeros((640, 6))                                                                            # two zeros
    two[:, :3] = rng.uniform(0.0, 1.0, (640, 3))
    axis, sign = np.arange(640) % 3, np.where((np.arange(640) // 3) % 2 == 0, 1.0, -1.0)
    two[np.arange(640), 3 + axis] = sign
    two[np.arange(640), axis] = np.where(np.arange(640) % 4 == 0, two[np.arange(640), axis],
                                         0.5 - 1.5 * sign)  # three in four start outside, aimed in
    parts.append(two)
    rays = np.vstack(parts)
    assert rays.shape == (4096, 6)
    return rays


@pytest.fixture(scope="module")
def walk_scene():
    v, f = soup(2000, 5)
    span = np.array([(-0.1, -0.1, -0.1), (1.1, -0.05, 1.1), (-0.07, 1.1, 1.05)])  # its box is the whole box
    v = np.vstack([v[:3000], span, v[3000:]])
    f = np.arange(3 * 2001).reshape(2001, 3)
    return TriangleMesh(v, f), walk_rays()


@pytest.mark.parametrize("tnear,tfar", [(0.0, INF), (0.1, 0.7)])
def test_grid_walk(walk_scene, tnear, tfar):
    """The spanning triangle (index 1000) is referenced from every cell a ray visits: the count
    rule's case.  It must count once."""
    mesh, rays = walk_scene
    d = rays[:, 3:]
    kz = np.argmax(np.abs(d), axis=1)
    assert {(int(k), bool(s)) for k, s in zip(kz, d[np.arange(len(d)), kz] > 0)} == \
        {(k, s) for k in range(3) for s in (False, True)}
    ref, cnt = both_paths(mesh, rays, tnear, tfar, what=f"walk [{tnear}, {tfar}]")
    info = mesh.grid_info()
    assert info["cells"] > 100 and info["references"] > 2 * info["cells"]  # the spanning triangle is everywhere
    hits_span = R.ray_tri(rays, *(mesh.vertices[3000:3003][k][None] for k in range(3)), tnear, tfar)["hit"][:, 0]
    assert hits_span.sum() > 100 and (cnt[hits_span] >= 1).all()
    assert (cnt == 0).sum() > 200 and (cnt >= 3).sum() > 200
    if tfar == INF:
        assert (ref["triangle"] == 1000).sum() > 20


def test_far_origin_takes_the_fallback_and_keeps_the_bits():
    v, f = soup(300, 9)
    mesh = TriangleMesh(v, f)
    rng = np.random.default_rng(3)
    near = aimed_rays(rng, 64)
    u = near[:, 3:] / np.linalg.norm(near[:, 3:], axis=1, keepdims=True)
    far = np.hstack([0.5 - u * 2.0 ** 30 * 1.2, u])  # 2^30 box sizes away, aimed at the box
    ref, cnt = both_paths(mesh, far, what="far", fallback=None)
    assert RC.ray_info(mesh)["fallback"] == len(far)  # the documented bound: |o| > 2^18 · the largest coordinate
    both_paths(mesh, near, what="near again")           # and the counter is per call
    mixed = np.vstack([near[:5], far[:3], [[1e200, 0.0, 0.0, -1.0, 0.0, 0.0], [np.nan, 0, 0, 1, 0, 0]]])
    both_paths(mesh, mixed, what="mixed", fallback=4)    # a ray that is not finite is no fallback ray


@pytest.fixture(scope="module")
def view():
    v, f = synth.surface_mesh(40, 60, seed=4)
    mesh = TriangleMesh(v, f)
    scale = float(np.abs(v).max())
    eye = np.array([2.0, 1.2, 2.5]) * scale
    rays = RC.RaycastingScene.create_rays_pinhole(40.0, np.zeros(3), eye, (0.0, 0.0, 1.0), 64, 64)
    return mesh, scale, eye, rays, R.cast_and_count(v, f, rays)


def test_pinhole_view_of_a_surface(view):
    mesh, scale, eye, rays, (ref, ref_cnt) = view
    assert len(mesh.triangles) == 4800
    both_paths(mesh, rays, what="pinhole")
    same_bits(RC.cast_rays(mesh, rays), ref, "pinhole auto")
    assert RC.ray_info(mesh)["path"] == "grid"  # 4,800 triangles are above the automatic threshold
    hit = ref["triangle"] >= 0
    assert 500 < hit.sum() < 64 * 64 and (ref_cnt[hit] % 2 == 0).all()  # a closed surface seen from outside


def test_virtual_scan(view):
    mesh, scale, eye, rays, (ref, _) = view
    pc, det = RC.virtual_scan(mesh, eye, np.zeros(3), (0.0, 0.0, 1.0), 40.0, 64, 64, with_details=True)
    hit = ref["triangle"] >= 0
    assert len(pc.points) == hit.sum() == len(pc.normals)
    np.testing.assert_array_equal(det["triangle"], ref["triangle"][hit])
    np.testing.assert_array_equal(det["t_hit"], ref["t_hit"][hit])
    np.testing.assert_array_equal(det["pixel"], np.argwhere(hit))
    # every point within 1e-12·scale of its triangle's plane, every normal a unit normal facing the eye
    a = mesh.vertices[mesh.triangles[det["triangle"], 0]]
    off = np.abs(((pc.points - a) * pc.normals).sum(axis=1))
    print("largest distance to the hit triangle's plane / scale:", off.max() / scale)
    assert (off <= 1e-12 * scale).all()
    np.testing.assert_allclose(np.linalg.norm(pc.normals, axis=1), 1.0, atol=1e-14)
    assert (((eye - pc.points) * pc.normals).sum(axis=1) > 0).all()
    assert len(RC.virtual_scan(mesh, eye, np.zeros(3), (0.0, 0.0, 1.0), 40.0, 64, 64).points) == hit.sum()


def test_occupancy_and_signed_distance_on_the_icosphere():
    v, f = R.icosphere(3)
    scene = RC.RaycastingScene()
    scene.add_triangles(v, f)
    rng = np.random.default_rng(8)
    u = rng.standard_normal((2048, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    radius = np.concatenate([rng.uniform(0.0, 0.9, 1024), rng.uniform(1.1, 3.0, 1024)])
    q = u * radius[:, None]
    truth = (radius < 1.0).astype(np.float32)
    dist = scene.compute_distance(q)
    for ns in (1, 3):
        occ = scene.compute_occupancy(q, ns)
        assert occ.dtype == np.float32
        np.testing.assert_array_equal(occ, truth)
        sd = scene.compute_signed_distance(q, ns)
        assert sd.dtype == np.float64
        assert np.abs(sd).tobytes() == dist.tobytes()
        np.testing.assert_array_equal(sd < 0, truth > 0)
    # the device counts are the restatement's for the very rays compute_occupancy builds
    rays = np.hstack([q, np.broadcast_to(RC.occupancy_directions(1)[0], (len(q), 3))])
    same_count(scene.count_intersections(rays), R.count_intersections(v, f, rays), "occupancy rays")
    out = scene.cast_rays(rays[:1024])
    assert (out["geometry_ids"] == 0).all() and (out["primitive_ids"] < len(f)).all()
    np.testing.assert_allclose(np.linalg.norm(out["primitive_normals"], axis=1), 1.0, atol=1e-14)
    assert scene.test_occlusions(rays[:1024]).all() and not scene.test_occlusions(rays[:1024], 0.0, 0.05).any()


def test_same_call_twice_gives_the_same_bytes(walk_scene):
    mesh, rays = walk_scene
    for path in ("brute", "grid"):
        a, b = (RC.cast_rays(mesh, rays, path=path) for _ in range(2))
        assert all(a[k].tobytes() == b[k].tobytes() for k in a)
        c, d = (RC.count_intersections(mesh, rays, path=path) for _ in range(2))
        assert c.tobytes() == d.tobytes()
