"""GPU parity of ICP against a mesh's surface (m3d_mesh_icp_terms / m3d_mesh_icp_run through m3d.mesh
and matcher) against the numpy restatement of the contract in tests/mesh_icp_restatement.py.

Winners (triangle and d² per point) are compared BIT FOR BIT: the brute-force path, the one-box grid
path with and without seeds and the restatement evaluate the same fp64 operations in one order on
the same operands.  Sums are compared within the bound of ANY summation order, ns·2^-52·Σ|term| per
slot, computed from the restatement's rows; the paths among themselves bit for bit.  The loop is
compared evaluation by evaluation on the device loop's own points (rebuilt from its updates): the
same triangles and fitness, rmse to 1e-12, every update and the pose to 1e-9 (test_gpu_robust.py's
tolerance for the same comparison), the same iteration count and stop decision.
"""
import numpy as np
import pytest

import icp_oracle as I
import mesh_icp_restatement as R
import mesh_restatement as MR
import matcher
import m3d.mesh as M
from m3d import _lib, synth
from m3d.core import Cloud

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:The given NumPy array is not writable")]

TILE = _lib.load().m3d_mesh_brute_tile()
LOSS = {R.L2: matcher.L2Loss, R.L1: matcher.L1Loss, R.HUBER: matcher.HuberLoss, R.CAUCHY: matcher.CauchyLoss,
        R.GM: matcher.GMLoss, R.TUKEY: matcher.TukeyLoss}
EPS = 2.0 ** -52


def loss_of(kind, k):
    return LOSS[kind]() if kind in (R.L2, R.L1) else LOSS[kind](k)


def filtered(ref, r):
    """The mesh contract's winners filtered by the radius → (triangle, d²)."""
    hit = (ref["triangle"] >= 0) & (ref["d2"] < r * r)
    return np.where(hit, ref["triangle"], -1).astype(np.int32), np.where(hit, ref["d2"], np.inf)


def check_winners(cloud, mesh, T, r, tri, d2, seeds, what, paths=("brute", "grid")):
    """One evaluation on every path, without and with seeds, against (tri, d2); returns the sums."""
    first = None
    for path in paths:
        for seed in (None, seeds):
            s, t, d = M.icp_to_mesh_terms(cloud, mesh, T, r, path=path, seed_triangles=seed)
            tag = f"{what} {path} {'seeded' if seed is not None else 'unseeded'}"
            bad = np.nonzero(t != tri)[0]
            assert len(bad) == 0, f"{tag}: triangle differs at {len(bad)} points, first {bad[:5]}: {t[bad[:5]]} != {tri[bad[:5]]}"
            assert d.tobytes() == d2.tobytes(), f"{tag}: d² differs at {np.nonzero(d != d2)[0][:5]}"
            if first is None:
                first = s
            assert s.tobytes() == first.tobytes(), f"{tag}: sums differ from the first path's"
    return first


# --------------------------------------------------------------------------------- winners
@pytest.fixture(scope="module")
def closed():
    """test_gpu_mesh.py's closed-mesh recipe (384 triangles; 2,000 queries near, inside, in the box
    and far away, 64 of them on vertices) at a pose T, the restatement's winners at T and — the
    seeds — at a slightly different pose."""
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
    # the source is T⁻¹·q, so that the loop's points at T are near q; the reference is computed on
    # the points the contract defines, q64_of(T, source)
    T = synth.random_rigid(5, center=v.mean(axis=0), rot_range=0.2, trans_range=0.1)
    src = I.transform_points(np.linalg.inv(T), q)
    pcd = I.initial_points(T, src)
    ref = MR.closest_points(v, f, pcd)
    T2 = synth.random_rigid(6, center=v.mean(axis=0), rot_range=0.01, trans_range=0.01) @ T
    seeds = MR.closest_points(v, f, I.initial_points(T2, src))["triangle"].astype(np.int32)
    # d² = 0 on a vertex needs the untransformed point: an identity pose for those checks
    ref_id = MR.closest_points(v, f, q)
    assert (ref_id["d2"] == 0.0).sum() >= 64 and set(np.unique(ref_id["region"])) == set(range(7))
    return dict(v=v, f=f, q=q, src=src, T=T, ref=ref, seeds=seeds, ref_id=ref_id, ext=ext)


def cell_of(mesh, v):
    info = mesh.grid_info()
    return float((v.max(axis=0) - v.min(axis=0)).max()) / round(info["cells"] ** (1 / 3))


@pytest.mark.parametrize("radius", ["tenth of a cell", "one cell", "larger than the mesh"])
def test_winners_of_one_evaluation(closed, radius):
    c = closed
    mesh = M.TriangleMesh(c["v"], c["f"])
    M.closest_points(mesh, c["q"][:4], path="grid")  # builds the grid: its cell size sets the radii
    cell = cell_of(mesh, c["v"])
    r = {"tenth of a cell": 0.1 * cell, "one cell": cell, "larger than the mesh": 4000.0 * c["ext"]}[radius]
    for T, src, ref in ((c["T"], c["src"], c["ref"]), (None, c["q"], c["ref_id"])):
        tri, d2 = filtered(ref, r)
        share = (tri >= 0).mean()
        print(f"{radius}: r = {r:.4g}, matched {share:.3f}")
        if radius == "larger than the mesh":
            assert share == 1.0
        else:
            assert 0.05 < share < 0.95
        check_winners(Cloud(src), mesh, T, r, tri, d2, c["seeds"], radius)
    assert (d2[tri >= 0] == 0.0).sum() >= 64  # (identity pose) the points on vertices match at distance zero


def test_bad_seeds_change_nothing(closed):
    """Seeds that name no triangle, the wrong triangle, or an index out of range."""
    c = closed
    mesh = M.TriangleMesh(c["v"], c["f"])
    r = 0.05 * c["ext"]
    tri, d2 = filtered(c["ref"], r)
    rng = np.random.default_rng(1)
    seeds = rng.integers(-5, len(c["f"]) + 5, len(c["src"])).astype(np.int32)
    seeds[::7] = np.iinfo(np.int32).max
    check_winners(Cloud(c["src"]), mesh, c["T"], r, tri, d2, seeds, "bad seeds", paths=("grid",))


def test_huge_triangle_and_tiny_ones():
    """test_gpu_mesh.py's mesh whose grid build doubles the cell."""
    rng = np.random.default_rng(13)
    huge = np.array([[0.0, 0.0, 0.0], [100.0, 0.0, 0.0], [0.0, 100.0, 0.01]])
    cc = rng.uniform(0.0, 1.0, (500, 1, 3)) * (1.0, 1.0, 0.01)
    tiny = (cc + rng.uniform(-0.01, 0.01, (500, 3, 3)) * (1.0, 1.0, 0.1)).reshape(-1, 3)
    v = np.vstack([huge, tiny])
    f = np.arange(len(v)).reshape(-1, 3)
    q = np.vstack([rng.uniform(-0.5, 1.5, (300, 3)) * (1.0, 1.0, 0.05), rng.uniform(0.0, 100.0, (300, 3)) * (1, 1, 0.1)])
    ref = MR.closest_points(v, f, q)
    assert 0 < (ref["triangle"] == 0).sum() < len(q)
    mesh = M.TriangleMesh(v, f)
    seeds = np.roll(ref["triangle"], 1).astype(np.int32)
    for r in (0.02, 2.0, 1000.0):
        tri, d2 = filtered(ref, r)
        print(f"r = {r}: matched {(tri >= 0).mean():.3f}")
        check_winners(Cloud(q), mesh, None, r, tri, d2, seeds, f"huge + tiny r={r}")
    assert mesh.grid_info()["doublings"] >= 1


def soup(F, seed):
    rng = np.random.default_rng(seed)
    c = rng.uniform(0.0, 1.0, (F, 1, 3))
    v = (c + rng.uniform(-0.1, 0.1, (F, 3, 3))).reshape(-1, 3)
    return v, np.arange(3 * F).reshape(F, 3)


@pytest.mark.parametrize("F", [1, 2, TILE - 1, TILE, TILE + 1])
def test_triangle_counts_across_the_brute_tile(F):
    v, f = soup(F, 11)
    q = np.random.default_rng(F).uniform(-0.2, 1.2, (300, 3))
    if F > 1:  # the last triangle of the mesh (past the tile edge at TILE + 1) wins somewhere
        q[:3] = v[f[F - 1]].mean(axis=0) + [[0, 0, 0], [1e-3, 0, 0], [0, 1e-3, 0]]
    ref = MR.closest_points(v, f, q)
    assert F == 1 or (ref["triangle"][:3] == F - 1).any()
    r = float(np.sqrt(np.median(ref["d2"])))
    tri, d2 = filtered(ref, r)
    assert 0.3 < (tri >= 0).mean() < 0.7
    check_winners(Cloud(q), M.TriangleMesh(v, f), None, r, tri, d2, None, f"F={F}", paths=("brute",))


# ------------------------------------------------------------------------------------ sums
def eval_radius():
    """The distance 70 % of clean_pair's points are within at the evaluation's pose."""
    c = R.clean_pair()
    d2 = MR.closest_points(c["v"], c["f"], I.initial_points(R.loop_init("perturbed"), c["src"]))["d2"]
    return float(np.sqrt(np.quantile(d2, 0.7)))


def eval_case(ns, _r=[]):
    """clean_pair's first ns source points at a small non-identity pose, a radius that leaves some
    points unmatched, and the restatement's evaluation."""
    c = R.clean_pair()
    T = R.loop_init("perturbed")
    src = c["src"][:ns]
    pcd = I.initial_points(T, src)
    if not _r:
        _r.append(eval_radius())
    return c, T, src, pcd, _r[0], R.evaluate(pcd, c["v"], c["f"], _r[0])


def check_sums(got, pcd, c, ev, kind, k, ns, what):
    ref, mag = R.sums(pcd, c["v"], c["f"], ev, kind, k)
    bound = ns * EPS * mag
    err = np.abs(got - ref)
    worst = int(np.argmax(err - bound))
    print(f"{what}: worst slot {worst}: |Δ| {err[worst]:.3e}, bound {bound[worst]:.3e}")
    assert (err <= bound).all(), (what, np.nonzero(err > bound)[0], err, bound)
    assert got[28] == ref[28] == (ev["triangle"] >= 0).sum()


@pytest.mark.parametrize("ns", [0, 1, 63, 64, 65, 257, 600])
def test_sums_over_point_counts(ns):
    c, T, src, pcd, r, ev = eval_case(ns)
    mesh = M.TriangleMesh(c["v"], c["f"])
    if ns >= 63:
        assert 0 < (ev["triangle"] >= 0).sum() < ns
    seeds = np.roll(ev["triangle"], 3).astype(np.int32)
    got = check_winners(Cloud(src), mesh, T, r, ev["triangle"], ev["d2"], seeds, f"ns={ns}")
    check_sums(got, pcd, c, ev, R.L2, 1.0, ns, f"ns={ns}")
    again = check_winners(Cloud(src), mesh, T, r, ev["triangle"], ev["d2"], seeds, f"ns={ns} again")
    assert again.tobytes() == got.tobytes()
    if ns == 0:
        assert (got == 0.0).all()


@pytest.mark.parametrize("kind", [R.L2, R.L1, R.HUBER, R.CAUCHY, R.GM, R.TUKEY])
def test_sums_of_every_kernel(kind):
    c, T, src, pcd, r, ev = eval_case(600)
    k = float(np.median(np.abs(R.rows(pcd, c["v"], c["f"], ev)[0])))  # both branches of Huber and Tukey
    assert k > 0.0
    mesh, cloud = M.TriangleMesh(c["v"], c["f"]), Cloud(src)
    loss = loss_of(kind, k)
    per_path = []
    for path, seed in (("brute", None), ("grid", None), ("grid", ev["triangle"])):
        s, t, d = M.icp_to_mesh_terms(cloud, mesh, T, r, kernel=loss, path=path, seed_triangles=seed)
        np.testing.assert_array_equal(t, ev["triangle"])
        per_path.append(s)
    assert per_path[0].tobytes() == per_path[1].tobytes() == per_path[2].tobytes()
    check_sums(per_path[0], pcd, c, ev, kind, k, 600, f"kind {kind}")
    if kind == R.L2:  # no kernel is the L2 kernel
        s, _, _ = M.icp_to_mesh_terms(cloud, mesh, T, r, kernel=None, path="grid")
        assert s.tobytes() == per_path[0].tobytes()


# ------------------------------------------------------------------------------------ loop
_DEVICE = {}


def on_device(p):
    """A pair's cloud and mesh on the device, made once."""
    key = id(p["src"])
    if key not in _DEVICE:
        _DEVICE[key] = (Cloud(p["src"]), M.TriangleMesh(p["v"], p["f"]))
    return _DEVICE[key]


def run(p, init, loss, **kw):
    cloud, mesh = on_device(p)
    return M.icp_to_mesh(cloud, mesh, p["radius"], init=init, kernel=loss, **kw)


def tri_of(out, ns):
    t = np.full(ns, -1, np.int64)
    t[out.correspondence_set[:, 0]] = out.correspondence_set[:, 1]
    return t


def same(a, b):
    assert a.transformation.tobytes() == b.transformation.tobytes()
    assert (a.fitness, a.inlier_rmse, a.iterations, a.converged) == (b.fitness, b.inlier_rmse, b.iterations, b.converged)
    np.testing.assert_array_equal(a.correspondence_set, b.correspondence_set)
    assert a.update.tobytes() == b.update.tobytes()


@pytest.mark.parametrize("pair", ["clean", "outlier"])
@pytest.mark.parametrize("kind", [R.L2, R.TUKEY, R.HUBER])
@pytest.mark.parametrize("init_kind", ["identity", "perturbed"])
def test_loop_matches_restatement(pair, kind, init_kind):
    """Every evaluation, every update and the stop decision of the device loop against the
    restatement, which is driven along the device's own trajectory.

    A point whose closest point lies on an edge or a vertex shared by triangles is equally far from
    all of them, and the last bit of its coordinates decides the winner; the triangles have
    different normals, so two loops whose solves round differently (|ΔT| ~ 1e-16) can part there and
    are then not comparable at any tolerance.  So the restatement's points of evaluation k are built
    from the device's own updates (``result.update`` of the runs stopped after 1 … k updates, applied
    in q64_of's order: R.trajectory), which makes them the device's points bit for bit.  On them:
    the triangles of every evaluation are equal, without exception or allowance, and so is the
    fitness; d² is bit-equal on both paths; the rmse agrees to 1e-12; the restatement's ΔT from
    those points agrees with the device's to 1e-9; the restatement's stop rule on its own fitness
    and rmse gives the device's iteration count and converged flag; the pose composed from the
    restatement's ΔTs agrees with the device's to 1e-9."""
    p = R.clean_pair() if pair == "clean" else R.outlier_pair()
    init, kk = R.loop_init(init_kind), p.get("k", 0.005 * p["ext"])
    loss = loss_of(kind, kk)
    ns = len(p["src"])
    _, mesh = on_device(p)
    out = run(p, init, loss)
    K = out.iterations
    stops = [run(p, init, loss, max_iteration=k) for k in range(K + 1)]  # stops[k] ends on evaluation k
    same(stops[K], out)
    np.testing.assert_array_equal(stops[0].transformation, init)
    updates = [stops[k].update for k in range(1, K + 1)]
    pts = R.trajectory(p["src"], init, updates)
    T_ref, history = np.asarray(init, np.float64), []
    for k in range(K + 1):
        assert stops[k].iterations == k and (stops[k].converged == (k == K and out.converged))
        ev = R.evaluate(pts[k], p["v"], p["f"], p["radius"])
        history.append((ev["fitness"], ev["rmse"]))
        np.testing.assert_array_equal(tri_of(stops[k], ns), ev["triangle"], err_msg=f"evaluation {k}")
        assert stops[k].fitness == ev["fitness"], f"evaluation {k}"
        assert abs(stops[k].inlier_rmse - ev["rmse"]) <= 1e-12, f"evaluation {k}"
        cloud = Cloud(pts[k])
        for path in ("brute", "grid"):
            _, t, d = M.icp_to_mesh_terms(cloud, mesh, None, p["radius"], path=path)
            np.testing.assert_array_equal(t, ev["triangle"], err_msg=f"evaluation {k} {path}")
            assert d.tobytes() == ev["d2"].tobytes(), f"evaluation {k} {path}: d²"
        if k > 0:  # T ← ΔT·T, the device's product
            np.testing.assert_array_equal(stops[k].transformation, I.matmul4(updates[k - 1], stops[k - 1].transformation))
        if k < K:
            upd = R.update(pts[k], p["v"], p["f"], ev, kind, kk)
            np.testing.assert_allclose(updates[k], upd, rtol=0, atol=1e-9, err_msg=f"update {k}")
            T_ref = I.matmul4(upd, T_ref)
    assert R.stop_rule(history) == (K, out.converged), (history, K, out.converged)
    print(f"{pair} {kind} {init_kind}: {K} iterations, |T - ref| {np.abs(out.transformation - T_ref).max():.3e}, "
          f"|rmse - ref| {abs(out.inlier_rmse - history[-1][1]):.3e}")
    assert out.fitness == history[-1][0] and abs(out.inlier_rmse - history[-1][1]) <= 1e-12
    np.testing.assert_allclose(out.transformation, T_ref, rtol=0, atol=1e-9)
    np.testing.assert_array_equal(out.correspondence_set, R.pairs_of(ev["triangle"]))
    assert out.converged
    if pair == "clean":
        assert R.worst_error(out.transformation, p["T_true"], p["src"]) < 1e-12 and out.fitness == 1.0
    same(run(p, init, loss, path="brute"), out)             # brute force,
    same(run(p, init, loss, path="grid", seed=True), out)   # the grid with the seeded box
    same(run(p, init, loss, path="grid", seed=False), out)  # and without: the same bits
    same(run(p, init, loss), out)                           # and a second run
    same(run(p, init, loss, max_iteration=2, path="grid", seed=True), stops[min(2, K)])  # a run cut short, the same


def test_loop_edges_and_errors():
    p = R.clean_pair()
    init = R.loop_init("perturbed")
    mesh, cloud = M.TriangleMesh(p["v"], p["f"]), Cloud(p["src"])
    ev0 = R.evaluate(I.initial_points(init, p["src"]), p["v"], p["f"], p["radius"])
    for path in ("brute", "grid"):
        out = M.icp_to_mesh(cloud, mesh, p["radius"], init=init, max_iteration=0, path=path)
        np.testing.assert_array_equal(out.transformation, init)
        assert (out.iterations, out.converged) == (0, False)
        assert out.fitness == ev0["fitness"] and abs(out.inlier_rmse - ev0["rmse"]) <= 1e-12
        np.testing.assert_array_equal(out.correspondence_set, R.pairs_of(ev0["triangle"]))
        # a radius below every distance: nothing matches, the pose stays
        out = M.icp_to_mesh(cloud, mesh, 1e-9, init=init, path=path)
        np.testing.assert_array_equal(out.transformation, init)
        assert out.fitness == 0.0 and out.inlier_rmse == 0.0 and len(out.correspondence_set) == 0
        # an empty source is not an error
        out = M.icp_to_mesh(Cloud(np.zeros((0, 3))), mesh, p["radius"], init=init, path=path)
        np.testing.assert_array_equal(out.transformation, init)
        assert out.fitness == 0.0 and len(out.correspondence_set) == 0
    flat = M.TriangleMesh(np.array([[0.0, 0, 0], [1.0, 0, 0], [2.0, 0, 0], [1.0, 1.0, 1.0]]), [[0, 1, 2], [3, 3, 3]])
    with pytest.raises(ValueError, match="no usable triangle"):
        M.icp_to_mesh(cloud, flat, 1.0)
    with pytest.raises(ValueError, match="no usable triangle"):
        M.icp_to_mesh_terms(cloud, flat, None, 1.0)
    with pytest.raises(ValueError, match="k must be"):
        M.icp_to_mesh(cloud, mesh, 1.0, kernel=matcher.TukeyLoss(0.0))
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="max_correspondence_distance"):
            M.icp_to_mesh(cloud, mesh, bad)
        with pytest.raises(ValueError, match="max_correspondence_distance"):
            matcher.registration_icp_to_mesh(p["src"], mesh, bad)
    # point-to-point in params is refused by the C call
    import ctypes as C

    from m3d.core import _T16, ptr, stream_handle

    ctx, h = mesh._handle()
    prm = _lib.IcpParams(1e-6, 1e-6, 30, _lib.EST_POINT_TO_POINT, _lib.NN_GRID, 0)
    res = _lib.IcpResult()
    rc = ctx.lib.m3d_mesh_icp_run(ctx.h, h, cloud.h, _T16(np.eye(4)), 1.0, C.byref(prm), None, 0, 1, C.byref(res),
                                  ptr(None), stream_handle())
    assert rc == _lib.M3D_ERR_INVALID
    unknown = _lib.RobustKernel(17, 1.0)
    prm.estimation = _lib.EST_POINT_TO_PLANE
    rc = ctx.lib.m3d_mesh_icp_run(ctx.h, h, cloud.h, _T16(np.eye(4)), 1.0, C.byref(prm), C.byref(unknown), 0, 1,
                                  C.byref(res), ptr(None), stream_handle())
    assert rc == _lib.M3D_ERR_INVALID


# ------------------------------------------------------------------------------------- API
def test_api_returns_the_c_calls_bits():
    from m3d.types import PointCloud

    p = R.outlier_pair()
    mesh = M.TriangleMesh(p["v"], p["f"])
    loss = matcher.TukeyLoss(p["k"])
    low = M.icp_to_mesh(Cloud(p["src"]), mesh, p["radius"], kernel=loss)
    for source, target in ((p["src"], mesh), (PointCloud(p["src"]), (p["v"], p["f"]))):
        got = matcher.registration_icp_to_mesh(source, target, p["radius"], kernel=loss)
        assert got.transformation.tobytes() == low.transformation.tobytes()
        assert (got.fitness, got.inlier_rmse) == (low.fitness, low.inlier_rmse)
        np.testing.assert_array_equal(got.correspondence_set, low.correspondence_set)
    assert got.correspondence_set.shape[1] == 2 and 0.5 < got.fitness < 1.0
    ev = matcher.evaluate_registration_to_mesh(p["src"], mesh, p["radius"], got.transformation)
    # the loop's last evaluation ran on the incrementally moved points, this one on T·source: the
    # points differ by rounding, the matches are the same and the rmse agrees to 1e-12
    print(f"evaluate at the result: fitness {ev.fitness} ({got.fitness}), |Δrmse| {abs(ev.inlier_rmse - got.inlier_rmse):.3e}")
    assert ev.fitness == got.fitness and abs(ev.inlier_rmse - got.inlier_rmse) <= 1e-12
    np.testing.assert_array_equal(ev.correspondence_set, got.correspondence_set)
    np.testing.assert_array_equal(ev.transformation, got.transformation)
    # refine_registration_to_mesh: radius 0.4·voxel_size
    voxel = p["radius"] / 0.4
    ref = matcher.refine_registration_to_mesh(p["src"], mesh, np.eye(4), voxel, kernel=loss)
    exp = matcher.registration_icp_to_mesh(p["src"], mesh, voxel * 0.4, np.eye(4), kernel=loss)
    assert ref.transformation.tobytes() == exp.transformation.tobytes() and ref.fitness == exp.fitness
    other = matcher.registration_icp_to_mesh(p["src"], mesh, voxel, np.eye(4), kernel=loss)
    assert other.fitness > ref.fitness  # the radius matters on this pair


def test_flat_square_surface_against_its_vertices():
    """The flat 8 × 8 square of two triangles: a tilted, lifted grid of points comes back into the
    plane against the surface, while the four vertices as a target leave it where it was."""
    sq = np.array([[0.0, 0.0, 0.0], [8.0, 0.0, 0.0], [8.0, 8.0, 0.0], [0.0, 8.0, 0.0]])
    mesh = M.TriangleMesh(sq, [[0, 1, 2], [0, 2, 3]])
    g = np.linspace(2.5, 5.5, 7)
    flat = np.stack([*np.meshgrid(g, g, indexing="ij"), np.zeros((7, 7))], axis=2).reshape(-1, 3)
    tilt = I.vec6_to_matrix(np.array([0.03, -0.02, 0.0, 0.0, 0.0, 0.0]))
    pts = I.transform_points(tilt, flat - (4.0, 4.0, 0.0)) + (4.0, 4.0, 0.3)
    assert np.abs(pts[:, 2]).max() > 0.3
    out = matcher.registration_icp_to_mesh(pts, mesh, 1.0)
    moved = I.transform_points(out.transformation, pts)
    print(f"height before {np.abs(pts[:, 2]).max():.3g}, after {np.abs(moved[:, 2]).max():.3g}")
    assert out.fitness == 1.0 and np.abs(moved[:, 2]).max() <= 1e-12
    np.testing.assert_array_equal(np.unique(out.correspondence_set[:, 1]), [0, 1])
    up = np.tile([[0.0, 0.0, 1.0]], (4, 1))
    from m3d.types import PointCloud

    vert = matcher.registration_icp(pts, PointCloud(sq, up), 1.0)
    np.testing.assert_array_equal(vert.transformation, np.eye(4))
    assert vert.fitness == 0.0


# ------------------------------------------------------------------ bits of the recorded build
@pytest.mark.parametrize("call", ["run", "terms", "closest"])
def test_bits_of_the_recorded_build(call, golden):
    """m3d_mesh_icp_run (T, update, fitness, rmse, count, iterations, converged, triangles),
    m3d_mesh_icp_terms (30 sums, triangles, d²) and m3d_mesh_closest (d², triangle, point, uv,
    region) return, on the fixed cases of tests/mesh_bits_cases.py and on every path variant, the
    bits recorded in tests/golden/mesh_icp_bits.npz (tools/gen_mesh_bits.py) from the build that
    still had its own solve kernel, host-built state, triangle sweep and box walk in mesh_icp.hip."""
    import mesh_bits_cases as B

    assert B.TILE == TILE
    blob = golden("mesh_icp_bits.npz")[call].tobytes()
    at, seen = {}, 0
    for key, variant, fields in B.record(call):
        if key not in at:  # a case's variants share one record
            at[key], seen = seen, seen + sum(np.ascontiguousarray(a).nbytes for a in fields.values())
        o = at[key]
        for name, a in fields.items():
            got = np.ascontiguousarray(a).tobytes()
            exp = blob[o:o + len(got)]
            assert got == exp, (f"{key} {variant}: {name} differs from the recorded bits: "
                                f"{a.ravel()[:8]} != {np.frombuffer(exp, a.dtype)[:8]}")
            o += len(got)
    assert seen == len(blob) and len(at) >= len(B.SHAPES)
