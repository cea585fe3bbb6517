"""GPU parity of surface sampling (m3d_mesh_sample through m3d.mesh) and minimum-distance thinning
(m3d_thin_min_distance through m3d.prep) against the numpy restatement of the two contracts in
tests/mesh_sample_restatement.py: EVERY output bit for bit — points, triangles, uv and normals of
the samples; the decided array of the thinning, which holds the round of every decision, and the
round count.  Then the thinning's two invariants in fp64 numpy, and the pipeline end to end:
``register_to_mesh`` against ``refine_registration_to_mesh`` started from the true pose.
"""
import numpy as np
import pytest

import mesh_sample_restatement as R
import matcher
import m3d.mesh as M
from m3d import prep, synth
from ply import Ply

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:The given NumPy array is not writable")]

TRI_V = np.array([[0.25, -1.0, 0.5], [3.0, 0.125, 0.75], [-0.5, 2.0, 1.5]])
TRI_F = np.array([[0, 1, 2]])


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def check_samples(mesh, n, seed, what):
    got = M.sample_points(mesh, n, seed)
    ref = R.sample(mesh.vertices, mesh.triangles, n, seed)
    for k in ("triangle", "uv", "point", "normal"):
        assert same_bits(got[k], ref[k]), f"{what}: {k} differs at {np.nonzero(np.atleast_1d(got[k] != ref[k]))[0][:5]}"
    return got


def soup(F, seed):
    """test_gpu_mesh.py's soup: F well-shaped random triangles in the unit cube; here every fifth
    one (f % 5 == 4) made unusable, by turns collapsed to a point and given a NaN."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(0.0, 1.0, (F, 1, 3))
    v = c + rng.uniform(-0.1, 0.1, (F, 3, 3))
    bad = np.flatnonzero(np.arange(F) % 5 == 4)
    v[bad[0::2], 1:] = v[bad[0::2], :1]
    v[bad[1::2], 2, 1] = np.nan
    return v.reshape(-1, 3), np.arange(3 * F).reshape(F, 3), bad


# --------------------------------------------------------------------------------- sampling
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257])
def test_one_triangle(n):
    got = check_samples(M.TriangleMesh(TRI_V, TRI_F), n, 11, f"one triangle n={n}")
    assert got["point"].shape == (n, 3) and (got["triangle"] == 0).all()


@pytest.mark.parametrize("F", [1, 255, 256, 257, 1025])
def test_soup_across_the_scan_and_block_edges(F):
    v, f, bad = soup(F, 21)
    mesh = M.TriangleMesh(v, f)
    a = check_samples(mesh, 4096, 5, f"soup F={F}")
    w, cum, W = R.weights(v, f)
    assert mesh.sample_info() == {"W": W, "nonzero": int((w > 0).sum())}
    assert not np.isin(a["triangle"], bad).any()
    b = M.sample_points(mesh, 4096, 5)
    for k in a:
        assert same_bits(a[k], b[k]), f"soup F={F}: {k} differs between two calls"
    c = check_samples(mesh, 4096, 6, f"soup F={F} seed 6")
    assert not same_bits(a["point"], c["point"])
    if F > 1:
        assert (a["triangle"] != c["triangle"]).any()
        assert a["triangle"].max() >= F - 3  # the table's end is reached


def test_a_mesh_without_a_usable_triangle_is_an_error_of_the_call():
    with pytest.raises(ValueError, match="no usable triangle"):
        M.sample_points(M.TriangleMesh(np.zeros((3, 3)), TRI_F), 4)


@pytest.fixture(scope="module")
def surface():
    v, f = synth.surface_mesh(20, 40)
    return M.TriangleMesh(v, f)


def test_surface_mesh_samples_lie_on_the_surface(surface):
    got = check_samples(surface, 10000, 2, "surface_mesh(20, 40)")
    assert len(np.unique(got["triangle"])) > 0.9 * len(surface.triangles)
    d2 = M.closest_points(surface, got["point"])["d2"]
    bound = (2.0 ** -40 * float(np.abs(surface.vertices).max())) ** 2
    print("largest d² of a sample to the surface", float(d2.max()), "bound", bound)
    assert (d2 <= bound).all()
    pc = surface.sample_points_uniformly(1000, seed=2)
    assert same_bits(pc.points, got["point"][:1000]) and same_bits(pc.normals, got["normal"][:1000])


# --------------------------------------------------------------------------------- thinning
def check_thin(p, r, seed, what):
    """The device's decided array and round count against the restatement's, then the invariants."""
    idx, out = prep.thin_min_distance(p, r, seed=seed, with_details=True)
    d_ref, rounds_ref = R.thin_rounds(p, r, seed)
    bad = np.nonzero(out.decided != d_ref)[0]
    assert len(bad) == 0, f"{what}: decided differs at {bad[:5]}: {out.decided[bad[:5]]} != {d_ref[bad[:5]]}"
    assert out.rounds == rounds_ref, f"{what}: {out.rounds} rounds, the restatement {rounds_ref}"
    assert out.kept == len(idx) == int((d_ref > 0).sum())
    assert idx.dtype == np.int64 and same_bits(idx, np.flatnonzero(d_ref > 0).astype(np.int64))
    check_invariants(p, r, out.decided > 0, what)
    return idx, out


def check_invariants(p, r, kept, what):
    """Every kept pair at least r apart; every dropped point has a kept one strictly inside r."""
    k = p[kept]
    for i in range(0, len(p), 512):
        q = p[i:i + 512]
        d = q[:, None, :] - k[None, :, :]
        d2 = (d[:, :, 0] * d[:, :, 0] + d[:, :, 1] * d[:, :, 1]) + d[:, :, 2] * d[:, :, 2]
        inside = d2 < r * r
        mine = kept[i:i + 512]
        assert (inside[mine].sum(axis=1) == 1).all(), f"{what}: two kept points closer than r"  # itself only
        assert inside[~mine].any(axis=1).all(), f"{what}: a dropped point without a kept one inside r"


def by_rank(points, seed):
    out = np.empty_like(points)
    out[R.rank_order(seed, len(points))] = points
    return out


def test_thin_tiny_clouds():
    idx, out = prep.thin_min_distance(np.zeros((0, 3)), 0.5, with_details=True)
    assert len(idx) == 0 and out.rounds == 0 and out.kept == 0
    idx, out = check_thin(np.array([[1.0, 2.0, 3.0]]), 0.5, 0, "n=1")
    assert list(idx) == [0] and out.rounds == 1
    idx, _ = check_thin(np.array([[0.0, 0, 0], [1.0, 0, 0]]), 0.5, 0, "n=2 apart")
    assert list(idx) == [0, 1]
    idx, _ = check_thin(np.array([[0.0, 0, 0], [0.25, 0, 0]]), 0.5, 0, "n=2 close")
    assert len(idx) == 1


def test_thin_chain_and_ties():
    seed = 4
    order = R.rank_order(seed, 3)
    idx, out = check_thin(by_rank(np.array([[0.0, 0, 0], [0.9, 0, 0], [1.8, 0, 0]]), seed), 1.0, seed, "chain")
    assert sorted(idx) == sorted([order[0], order[2]]) and out.rounds == 3
    idx, _ = check_thin(np.array([[0.0, 0, 0], [3.0, 4.0, 0]]), 5.0, 0, "exactly r")
    assert list(idx) == [0, 1]
    for s in (0, 1, 2, 3):
        idx, _ = check_thin(np.ones((2, 3)), 0.5, s, "equal points")
        assert list(idx) == [R.rank_order(s, 2)[0]]


def test_thin_uniform_cube():
    p = np.random.default_rng(2).uniform(0.0, 1.0, (3000, 3))
    idx, out = check_thin(p, 0.08, 0, "3000 uniform")
    assert 500 < len(idx) < 3000 and 2 < out.rounds < 32
    idx7, _ = check_thin(p, 0.08, 7, "3000 uniform seed 7")
    assert not same_bits(idx, idx7)
    a, _ = prep.thin_min_distance(p, 0.08, seed=0, with_details=True)
    assert same_bits(a, idx)


def test_thin_clump_inside_one_radius():
    """200 points inside one radius (more than 64 candidates in a cell row: the chunk loop) and
    500 spread ones."""
    rng = np.random.default_rng(6)
    p = np.vstack([0.5 + rng.uniform(-0.02, 0.02, (200, 3)), rng.uniform(0.0, 1.0, (500, 3))])
    perm = rng.permutation(len(p))
    p = p[perm]
    idx, _ = check_thin(p, 0.08, 3, "clump")
    assert (perm[idx] < 200).sum() <= 1  # the clump's points are all within 0.04·√3 < r of each other


def test_thin_with_a_far_point():
    """One coordinate at 1e6: the grid's edge cells, and a coarse fp32 screen."""
    p = np.random.default_rng(8).uniform(0.0, 1.0, (3000, 3))
    p[1234, 0] = 1e6
    idx, _ = check_thin(p, 0.08, 1, "far point")
    assert 1234 in idx


def test_thin_rows_that_are_not_finite():
    p = np.random.default_rng(9).uniform(0.0, 1.0, (500, 3))
    p[7, 1] = np.nan
    p[300, 2] = np.inf
    idx, out = prep.thin_min_distance(p, 0.1, seed=2, with_details=True)
    d_ref, _ = R.thin_rounds(p, 0.1, 2)
    np.testing.assert_array_equal(out.decided > 0, d_ref > 0)
    assert out.decided[7] == -1 and out.decided[300] == -1


def test_point_cloud_and_poisson_disk_on_the_device(surface):
    pc, det = surface.sample_points_poisson_disk(500, seed=3, with_details=True)
    assert pc.points.shape == (500, 3) and pc.has_normals() and det["kept"] >= 500
    base = surface.sample_points_uniformly(2500, seed=3)
    assert same_bits(pc.points, base.points[det["indices"]])
    kept = np.zeros(2500, bool)
    kept[R.thin_min_distance(base.points, det["radius"], 3)] = True
    assert kept[det["indices"]].all()
    d = np.linalg.norm(pc.points[:, None, :] - pc.points[None, :, :], axis=2)
    assert d[np.triu_indices(500, 1)].min() >= det["radius"]
    thin, ind = base.thin_min_distance(0.5, seed=1)
    assert same_bits(ind, R.thin_min_distance(base.points, 0.5, 1)) and same_bits(thin.points, base.points[ind])


# --------------------------------------------------------------------------------- end to end
# The largest |ΔT| entry between register_to_mesh and refine_registration_to_mesh started from the true
# pose, measured on an MI355X; the two runs stop on a 1e-6 relative criterion at
# different iterations, so the test allows ten times that.
E2E_DT_MEASURED = 1.233e-13


def test_register_to_mesh_reaches_the_optimum_of_the_true_pose():
    voxel = 0.3
    v, f = synth.surface_mesh(60, 120, seed=1)
    mesh = M.TriangleMesh(v, f)
    Tm = synth.random_rigid(3)
    scan = synth.apply(Tm, R.sample(v, f, 20000, seed=17)["point"])
    true = np.linalg.inv(Tm)
    np.random.seed(12345)  # Ply adds its noise from the global RNG
    src = Ply.from_arrays(scan, voxel_size=voxel, preprocess=True)
    got = matcher.register_to_mesh(src, mesh, voxel_size=voxel, seed=0)
    best = matcher.refine_registration_to_mesh(src, mesh, true, voxel)
    dT = float(np.abs(got.transformation - best.transformation).max())
    t_err = float(np.linalg.norm((got.transformation @ Tm)[:3, 3]))
    print(f"register_to_mesh: max |dT| {dT:.3e}, translation error {t_err:.3e}, fitness {got.fitness:.4f} "
          f"against {best.fitness:.4f}, rmse {got.inlier_rmse:.3e} against {best.inlier_rmse:.3e}")
    assert t_err < voxel / 10.0
    assert dT <= 10.0 * E2E_DT_MEASURED
